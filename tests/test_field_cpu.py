"""The field at arbitrary points (bh_field_at), what can be checked without a GPU:

  * tests/field_ref.py, the numpy reference of the GPU tests, against the pinned oracle walking appended points
    (field_ref.oracle_at_points): equal term counts for every point, acceleration within the forward bound;
  * the C-ABI declaration, the export, the ctypes signature, BarnesHutEngine.field and the project.py flags;
  * the engine unit compiles for gfx950 with the side-walk kernels (field and potential) in it, none of them with scratch
    or spills;
  * the deep-chain input of the GPU tests really reaches the second tier of the kernels' lane stack."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from oracle import bh_oracle as O
import field_ref as FR
import kernel_meta as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the helper against the pinned oracle ---------------------------------------------------------------------------
def _systems(init1024):
    m, p, _ = init1024
    yield "init1024", p, m
    p2, m2 = FR.clumped(4096, 7)
    yield "clumped4096", p2, m2


@pytest.mark.parametrize("theta", [0.5, 0.2])
@pytest.mark.parametrize("max_depth,compat", [(10, True), (10, False), (21, True), (21, False)])
def test_field_ref_is_the_oracle_walk_of_appended_points(init1024, theta, max_depth, compat):
    for name, p, m in _systems(init1024):
        pts = FR.points_around(p, 1500, 3)
        nodes = O.build_tree(p, m, max_depth)
        d = FR.oracle_at_points(nodes, p, m, pts, theta=theta, compat=compat)
        n = len(p)
        plain = O.compute_forces(nodes, np.concatenate([p, pts]), np.concatenate([m, np.ones(len(pts))]), theta=theta,
                                 compat_self_skip=compat, lo=n, hi=n + len(pts))[n:]
        assert np.array_equal(d.forces, plain), name              # the diagnostic walk is the pinned walk
        assert np.isfinite(d.forces).all(), name
        r = FR.field_walk(nodes, pts, theta=theta)
        assert np.array_equal(r.counts, d.counts.astype(np.int64)), name
        err = np.linalg.norm(r.accel - d.forces, axis=1)
        assert (err <= FR.accel_bound(r.counts, r.abs_sum)).all(), (name, np.max(err / FR.accel_bound(r.counts, r.abs_sum)))
        assert (r.phi < 0).all() and np.allclose(-r.phi, r.pot_sum, rtol=1e-12), name
        outside = (pts[:, 0] < p[:, 0].min()) | (pts[:, 0] > p[:, 0].max()) | (pts[:, 1] < p[:, 1].min()) | (pts[:, 1] > p[:, 1].max())
        assert outside.sum() > 300 and (~outside).sum() > 300


def test_field_ref_edges():
    p = np.array([[0.0, 0.0], [1.0, 0.0]])
    m = np.array([2.0, 2.0])
    nodes = O.build_tree(p, m, 10)
    r = FR.field_walk(nodes, [[0.5, 0.0], [1e6, 0.0]], theta=0.5, G=1.0)
    assert r.counts[0] == 2 and abs(r.accel[0, 0]) <= FR.accel_bound(2, r.abs_sum[0]) and r.accel[0, 1] == 0.0
    assert r.phi[0] == pytest.approx(-2 * 2.0 / 0.5, rel=1e-14)
    assert r.counts[1] == 1 and r.accel[1, 0] == pytest.approx(-4.0 / (1e6 - 0.5) ** 2, rel=1e-12)
    assert np.isinf(r.margin[1]) or r.margin[1] > 0.9


# ---- the interface ---------------------------------------------------------------------------------------------------
def test_bh_field_at_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "bhgpu.h")).read()
    decl = re.search(r"int\s+bh_field_at\s*\(([^)]*)\)\s*;", hdr)
    assert decl, "include/bhgpu.h does not declare bh_field_at"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["bh_ctx *ctx", "const double *points", "int64_t n_points", "double *accel", "double *phi", "uint32_t *counts"]
    assert re.search(r"#define\s+BHGPU_ABI_VERSION\s+4\b", hdr)
    from gpu_nbody_simulation_amd import _lib
    assert _lib.ABI_VERSION == 4
    res, argtypes = _lib.SIGNATURES["bh_field_at"]
    dp = C.POINTER(C.c_double)
    assert res is C.c_int and argtypes == [C.c_void_p, dp, C.c_int64, dp, dp, C.POINTER(C.c_uint32)]
    lib = _lib.load()                                            # (raises if a declared symbol is not exported)
    assert lib.bh_field_at.argtypes == argtypes and lib.bh_abi_version() == 4


def test_engine_has_field():
    import gpu_nbody_simulation_amd as G
    sig = inspect.signature(G.BarnesHutEngine.field)
    assert list(sig.parameters) == ["self", "points", "with_counts"] and sig.parameters["with_counts"].default is False


def test_project_accepts_the_field_flags():
    from gpu_nbody_simulation_amd import project
    a, _ = project._parse(["--field-file", "map.csv", "--field-grid", "16", "8", "--field-box", "-1", "1", "-2", "2"])
    assert a.field_file == "map.csv" and list(a.field_grid) == [16, 8] and list(a.field_box) == [-1.0, 1.0, -2.0, 2.0]
    a, _ = project._parse(["--field-file", "map.csv", "--field-grid", "4", "4"])
    assert a.field_box is None
    a, _ = project._parse([])
    assert a.field_file is None and a.field_grid is None and a.field_box is None
    pts = project.field_grid_points((4, 2), (0.0, 4.0, 0.0, 2.0), None)
    assert pts.shape == (8, 2) and pts[:4, 0].tolist() == [0.5, 1.5, 2.5, 3.5] and pts[:, 1].tolist() == [0.5] * 4 + [1.5] * 4


# ---- the kernels ------------------------------------------------------------------------------------------------------
# the side walks as a family (csrc/bh_treewalk.hpp): one field_keys_kernel, field_f64_kernel<ACCEPT> and
# potential_f64_kernel<COMPAT, ACCEPT> for the three DiagAccept criteria, the two fp32 kernels
FIELD_KERNELS = ["_ZN2bh17field_keys_kernel", "_ZN2bh16field_f64_kernelILi0E", "_ZN2bh16field_f64_kernelILi1E",
                 "_ZN2bh16field_f64_kernelILi2E", "_ZN2bh16field_f32_kernel"]
POTENTIAL_KERNELS = ["_ZN2bh20potential_f64_kernelILb%dELi%dE" % (cp, acc) for cp in (0, 1) for acc in (0, 1, 2)] + [
    "_ZN2bh20potential_f32_kernel"]


def test_field_kernels_compile_for_gfx950_without_scratch_or_spills():
    text = KM.assembly("bh_engine.hip")[0]
    seen = KM.kernels(text, r"_ZN2bh1[67]field_\S+|_ZN2bh20potential_f\d\d_kernel\S+")
    for prefix in FIELD_KERNELS + POTENTIAL_KERNELS:
        assert sum(k.startswith(prefix) for k in seen) == 1, (prefix, sorted(seen))
    assert len(seen) == len(FIELD_KERNELS) + len(POTENTIAL_KERNELS)
    for name, k in seen.items():
        assert k["scratch"] == 0 and k["dynamic_stack"] == "false" and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= 64 and k["sgpr"] <= 80, (name, k)     # 8 waves per SIMD


# ---- the deep chain ---------------------------------------------------------------------------------------------------
def test_the_deep_chain_needs_the_second_tier_of_the_lane_stack():
    """The lane stack of the side walks (csrc/bh_treewalk.hpp) keeps entries 0..63 in one triple of registers and 64..127 in
    a second; tests/test_gpu_field.py and tests/test_gpu_energy.py run field_ref.deep_chain to reach the second.  Here, on
    the oracle's tree alone: the walk of the point next to the origin and of the last body holds more than 64 quads at
    once at theta 0.2 (at 0.5 it would not), and max_depth 32 caps nothing."""
    p, m = FR.deep_chain()
    assert len(m) == 172 and np.array_equal(O.root_bounds(p), [-1.2, 1.2, -1.2, 1.2])
    nodes = O.build_tree(p, m, FR.DEEP_DEPTH)
    assert len(nodes) == len(O.build_tree(p, m, 0)) == 461
    deepest, terms = FR.pending_quads(nodes, FR.DEEP_POINT[0], FR.DEEP_THETA)
    assert deepest == 85 and terms == 172
    assert terms == FR.oracle_at_points(nodes, p, m, FR.DEEP_POINT, theta=FR.DEEP_THETA, compat=False).counts[0]
    assert FR.pending_quads(nodes, FR.DEEP_POINT[0], 0.5)[0] == 57
    last = len(m) - 1
    deepest, terms = FR.pending_quads(nodes, p[last], FR.DEEP_THETA, self_index=last)
    assert deepest > 64
    assert terms == O.compute_forces_diag(nodes, p, m, theta=FR.DEEP_THETA, compat_self_skip=False).counts[last]
