"""On-device diagnostics (bh_compute_potential, bh_get_potential, bh_energy):

  * fp64 precisions: per-body term counts == the oracle's interaction counts, phi within 1e-12 of the reference walk
    (tests/potential_ref.py over the oracle's tree);
  * fp32 / mixed: per-body term counts == the force walk's bh_get_interaction_counts on the same state, phi within
    F32_TOL of the fp64 reference walk on the bodies whose counts are the oracle's;
  * reductions against math.fsum over the downloaded state, bitwise repeatable;
  * a bh_energy after every step leaves the trajectory bit for bit as it was, in every precision;
  * physics (two-body orbit, Plummer sphere), scale (1M bodies), errors, and the project.py energy file."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import _lib, initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_PORTABLE, FLAG_WALK_STATS  # noqa: E402
from gpu_nbody_simulation_amd.project import runSimulationGpu  # noqa: E402
from potential_ref import potential_walk  # noqa: E402
import field_ref as FR  # noqa: E402
import quiet_case as QC  # noqa: E402
from reduction_ref import quotient_tolerance, sum2_tolerance  # noqa: E402

P = G.Precision
F64_TOL = 1e-12
# fp32 terms (rsq of an fp32 d2 from fp32 positions and fp32 node centres) against the fp64 walk of the fp32-rounded
# positions, relative, on bodies whose fp32 acceptance equals the oracle's; twice the measured maxima:
#   1,024 sampled bodies of the 1M Plummer sphere: 1.47e-6;
#   all bodies of a 40,960-body Plummer sphere (depth-cap aggregates close to their own bodies, whose fp32 centre of
#   mass moves d by up to 2e-4 relative): 2.33e-4 (median 8e-9)
F32_TOL = 3e-6
F32_TOL_ALL = 5e-4
ERR_ARG, ERR_STATE = -1, -5


def engine(n, **kw):
    return G.BarnesHutEngine(G.BhConfig(capacity=n, **kw))


def rounded(*a):
    return [x.astype(np.float32).astype(np.float64) for x in a]


def clumped(n, seed):
    """A few Gaussian clumps of different widths: deep, uneven trees."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-1.0, 1.0, (8, 2))
    widths = 10.0 ** r.uniform(-3.0, -1.0, 8)
    k = r.integers(0, 8, n)
    p = centres[k] + r.normal(0.0, 1.0, (n, 2)) * widths[k, None]
    return r.uniform(0.1, 0.5, n), p, r.normal(0.0, 1e-4, (n, 2))


def systems():
    yield "init1024", None
    yield "random4096", lambda: IC.make("uniform", 4096, 11)
    yield "clumped40960", lambda: clumped(40960, 5)


# ---- 1. fp64 precisions against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F64_EXACT, P.F64])
@pytest.mark.parametrize("theta", [0.5, 0.2])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("name", ["init1024", "random4096", "clumped40960"])
def test_fp64_potential_against_the_reference_walk(init1024, prec, theta, compat, name):
    m, p, v = init1024 if name == "init1024" else dict(systems())[name]()
    n = len(m)
    md = 10 if compat else 32
    with engine(n, precision=prec, theta=theta, reference_compat=compat, max_depth=md) as e:
        e.upload(p, v, m)
        phi, cnt = e.potential(with_counts=True)
    nodes = O.build_tree(p, m, md if md < 32 else 0)
    d = O.compute_forces_diag(nodes, p, m, theta=theta, compat_self_skip=compat)
    assert np.array_equal(cnt, d.counts)
    ref, rcnt = potential_walk(nodes, p, theta=theta, compat=compat)
    assert np.array_equal(rcnt, d.counts.astype(np.int64))
    assert (np.abs(phi - ref) <= F64_TOL * np.abs(ref)).all(), np.max(np.abs(phi - ref) / np.abs(ref))


def test_portable_exact_walk_takes_the_same_terms(init1024):
    """BH_FLAG_WALK_PORTABLE: the nodes carry sizes, the potential walk uses size / d < theta like the force walk."""
    from gpu_nbody_simulation_amd.engine import FLAG_WALK_PORTABLE
    m, p, v = init1024
    with engine(1024, flags=FLAG_WALK_PORTABLE) as e:
        e.upload(p, v, m)
        phi, cnt = e.potential(with_counts=True)
    nodes = O.build_tree(p, m, 10)
    ref, rcnt = potential_walk(nodes, p)
    assert np.array_equal(cnt.astype(np.int64), rcnt)
    assert (np.abs(phi - ref) <= F64_TOL * np.abs(ref)).all()


def test_fp64_potential_of_the_deep_chain_uses_the_second_stack_tier():
    """field_ref.deep_chain at theta 0.2: the last body's walk holds more than 64 quads pending (tests/test_field_cpu.py), so
    its wavefront pushes past entry 64 of the lane stack.  All 172 bodies, checked as above.  (No body meets a cell whose
    size / d is closer to theta than 9.7e-3 relative -- field_ref.field_walk(...).margin --, so BH_PRECISION_F64's own
    thresholds decide as the oracle does.)"""
    p, m = FR.deep_chain()
    nodes = O.build_tree(p, m, FR.DEEP_DEPTH)
    d = O.compute_forces_diag(nodes, p, m, theta=FR.DEEP_THETA, compat_self_skip=False)
    ref, rcnt = potential_walk(nodes, p, theta=FR.DEEP_THETA, compat=False)
    assert np.array_equal(rcnt, d.counts.astype(np.int64))
    for prec, flags in [(P.F64_EXACT, 0), (P.F64_EXACT, FLAG_WALK_PORTABLE), (P.F64, 0)]:
        with engine(len(m), precision=prec, theta=FR.DEEP_THETA, reference_compat=False, max_depth=FR.DEEP_DEPTH, flags=flags) as e:
            e.upload(p, np.zeros_like(p), m)
            phi, cnt = e.potential(with_counts=True)
        assert np.array_equal(cnt, d.counts), (prec, flags)
        print(prec.name, flags, "max rel err %.3e" % np.max(np.abs(phi - ref) / np.abs(ref)))
        assert (np.abs(phi - ref) <= F64_TOL * np.abs(ref)).all(), (prec, flags, np.max(np.abs(phi - ref) / np.abs(ref)))


# ---- 2. fp32 precisions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.2])
def test_fp32_potential_takes_the_force_walks_terms(prec, compat, theta):
    m, p, v = IC.make("plummer", 40960, 3)
    n = len(m)
    md = 10 if compat else 16
    with engine(n, precision=prec, theta=theta, reference_compat=compat, max_depth=md, flags=FLAG_WALK_STATS) as e:
        e.upload(p, v, m)
        e.step(3)                                            # (a physical re-order and a bucket sort have run)
        e.compute_forces()
        fc = e.interaction_counts()
        phi, cnt = e.potential(with_counts=True)
        p1, _ = e.download()
        m1 = e.masses()
    assert np.array_equal(cnt, fc)
    pr, mr = rounded(p1, m1)
    if compat:
        ref, rcnt = potential_walk(O.build_tree(pr, mr, md), pr, theta=theta, G=6.67e-11, compat=True)
        same = rcnt == cnt
        assert same.mean() > 0.9
        err = np.abs(phi[same] - ref[same]) / np.abs(ref[same])
        print(f"fp32 potential {prec.name} theta {theta}: {same.mean():.4f} of the bodies with the oracle's terms, "
              f"max rel {err.max():.3g}, median {np.median(err):.3g}")
        assert err.max() <= F32_TOL_ALL


# ---- 3. reductions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(P))
def test_energy_reductions_against_fsum(prec):
    m, p, v = clumped(30000, 9)
    v = v * 1e3
    with engine(len(m), precision=prec) as e:
        e.upload(p, v, m)
        e.step(17)                                           # (fp32: the state is in device order after a re-order)
        a = e.energy()
        b = e.energy()
        e.potential()
        c = e.energy()
        phi = e.potential()
        x, u = e.download()
        mm = e.masses()
    assert a == b == c
    terms = {
        "mass": mm, "com0": mm * x[:, 0], "com1": mm * x[:, 1], "px": mm * u[:, 0], "py": mm * u[:, 1],
        "L": mm * (x[:, 0] * u[:, 1] - x[:, 1] * u[:, 0]), "kin": 0.5 * mm * (u ** 2).sum(axis=1),
        "pot": 0.5 * mm * phi,
    }
    got = {"mass": a.mass, "px": a.momentum[0], "py": a.momentum[1], "L": a.angular_momentum, "kin": a.kinetic,
           "pot": a.potential}
    n, ref, tol = len(mm), {}, {}
    for k, t in terms.items():
        ref[k], scale = math.fsum(t), math.fsum(np.abs(t))
        tol[k] = sum2_tolerance(ref[k], scale, n)
        if k in got:
            assert abs(got[k] - ref[k]) <= tol[k], (k, got[k], ref[k], tol[k])
    for i, k in enumerate(("com0", "com1")):                 # the host's quotient of two sums
        want = ref[k] / ref["mass"]
        bound = quotient_tolerance(ref[k], ref["mass"], tol[k], tol["mass"])
        assert abs(a.com[i] - want) <= bound, (k, a.com[i], want, bound)
    assert a.total == a.kinetic + a.potential and a.n_bodies == len(m)


# ---- 4. non-perturbation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,n_threads", [(P.F64_EXACT, 0), (P.F64, 0), (P.MIXED, 0), (P.F32, 0), (P.F32, 4096),
                                            (P.F64, 4096)])
def test_diagnostics_do_not_perturb_the_trajectory(prec, n_threads):
    m, p, v = IC.make("plummer", 24000, 4, quasi_static=True)
    runs = []
    for diag in (False, True):
        with engine(len(m), precision=prec, n_threads=n_threads) as e:
            e.upload(p, v, m)
            if diag:
                e.energy()
            for _ in range(20):
                e.step(1)
                if diag:
                    e.energy()
            st = e.stats()
            runs.append(e.download() + (st.walk_launches,))
    (x0, v0, w0), (x1, v1, w1) = runs
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)
    assert w0 == w1


@pytest.mark.parametrize("prec,n_threads", QC.CASES, ids=QC.IDS)
def test_diagnostics_do_not_perturb_the_stats_of_the_last_step(prec, n_threads):
    """tests/quiet_case.py: a first build by the LSD passes, the quiet build by the bucket sort."""
    QC.check(prec, n_threads, lambda e: e.energy())


def test_buffers_are_allocated_on_first_use_only():
    n = 5000
    m, p, v = IC.make("uniform", n, 2)
    with engine(n) as a, engine(n) as b:
        a.upload(p, v, m)
        b.upload(p, v, m)
        a.step(2)
        b.step(2)
        before = b.stats().device_bytes
        assert a.stats().device_bytes == before             # stepping alone allocates nothing new
        b.energy()
        grown = b.stats().device_bytes - before
    assert grown == n * 8 + n * 4 + 256 * 2 * 8 * 8 + 8 * 8 + 4 * 64 * 8


# ---- 5. physics ----------------------------------------------------------------------------------------------------
def test_two_body_circular_orbit_conserves_angular_momentum():
    """Equal masses 1, separation 1, G = 1: v = sqrt(1/2) each; dt = 0.01, 1,000 steps (~2.3 orbits).  Symplectic
    Euler conserves L of a central pair force exactly up to rounding; its energy error oscillates at O(dt) without
    drift (measured max |dE/E| 2.0e-4, |dL/L| 4e-15; bound 5e-4)."""
    vc = math.sqrt(0.5)
    p = np.array([[-0.5, 0.0], [0.5, 0.0]])
    v = np.array([[0.0, -vc], [0.0, vc]])
    m = np.array([1.0, 1.0])
    es = []
    with engine(2, precision=P.F64, G=1.0, dt=0.01, max_depth=32, reference_compat=False) as e:
        e.upload(p, v, m)
        es.append(e.energy())
        for _ in range(100):
            e.step(10)
            es.append(e.energy())
    L0, E0 = es[0].angular_momentum, es[0].total
    dL = max(abs(s.angular_momentum - L0) for s in es) / abs(L0)
    dE = np.array([abs(s.total - E0) / abs(E0) for s in es])
    print(f"two-body orbit: max |dL/L| {dL:.3g}, max |dE/E| {dE.max():.3g}")
    assert dL <= 1e-12
    assert dE.max() <= 5e-4
    assert dE[-30:].max() <= 1.5 * dE[:40].max() + 1e-12     # bounded: no secular growth


@pytest.mark.parametrize("prec", list(P))
def test_plummer_energy_drift_is_recorded(prec):
    """65,536-body Plummer sphere (G = 1, total mass 1, scale 0.02, cold), theta 0.5, dt 1e-8, 50 steps: |dE/E| per
    precision.  No softening: the closest pairs dominate the error, so only a loose sanity bound."""
    m, p, v = IC.plummer(65536, 21)
    with engine(len(m), precision=prec, G=1.0, dt=1e-8) as e:
        e.upload(p, v, m)
        e0 = e.energy()
        e.step(50)
        e1 = e.energy()
    drift = abs(e1.total - e0.total) / abs(e0.total)
    print(f"plummer 65536 {prec.name}: E0 {e0.total:.9g} E50 {e1.total:.9g} |dE/E| {drift:.3g} K50 {e1.kinetic:.6g}")
    assert np.isfinite(e1.total) and drift < 1.0


# ---- 6. scale ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F32, P.F64])
def test_million_body_plummer_sampled_against_the_reference_walk(prec):
    n = 1 << 20
    m, p, v = IC.plummer(n, 8)
    with engine(n, precision=prec) as e:
        e.upload(p, v, m)
        phi, cnt = e.potential(with_counts=True)
    if prec == P.F32:
        p, m = rounded(p, m)
    sample = np.random.default_rng(1).choice(n, 1024, replace=False)
    ref, rcnt = potential_walk(O.build_tree(p, m, 10), p, bodies=sample)
    err = np.abs(phi[sample] - ref) / np.abs(ref)
    if prec == P.F64:
        assert np.array_equal(cnt[sample].astype(np.int64), rcnt)
        assert err.max() <= F64_TOL
    else:
        same = cnt[sample].astype(np.int64) == rcnt
        print(f"1M plummer fp32: {same.mean():.4f} of the sample with the oracle's terms, max rel {err[same].max():.3g}")
        assert same.mean() > 0.9 and err[same].max() <= F32_TOL


# ---- 7. errors -----------------------------------------------------------------------------------------------------
def test_errors():
    lib = _lib.load()
    with engine(64) as e:
        h = e._h
        out = _lib.bh_energy_t()
        phi = np.zeros(64)
        dp = phi.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.bh_compute_potential(h) == ERR_STATE
        assert lib.bh_energy(h, C.byref(out)) == ERR_STATE
        assert lib.bh_get_potential(h, dp, None) == ERR_STATE
        m, p, v = IC.make("uniform", 64, 1)
        e.upload(p, v, m)
        assert lib.bh_get_potential(h, dp, None) == ERR_STATE     # not computed yet
        assert lib.bh_energy(h, None) == ERR_ARG
        assert lib.bh_get_potential(h, None, None) == ERR_ARG
        assert lib.bh_compute_potential(None) == ERR_ARG
        assert lib.bh_energy(h, C.byref(out)) == 0
        assert lib.bh_get_potential(h, dp, None) == 0
        e.step(1)
        assert lib.bh_get_potential(h, dp, None) == ERR_STATE     # the state moved on
    with engine(4096, precision=P.F32) as e:
        m, p, v = IC.make("uniform", 1000, 1)
        e.upload(p, v, m)
        e.let_configure(0, 2, 1024)
        with pytest.raises(G.BhError) as ex:
            e.energy()
        assert ex.value.args[0] == ERR_STATE or "distributed" in str(ex.value)


def test_project_energy_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "plain", tmp_path / "energy"
    a.mkdir()
    b.mkdir()
    pa, va, _ = runSimulationGpu(m, p, v, 7, out_dir=str(a))
    pb, vb, _ = runSimulationGpu(m, p, v, 7, out_dir=str(b), energy_file="energy.csv", energy_every=3)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    for f in ("quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / f).read_bytes() == (b / f).read_bytes()
    assert sorted(os.listdir(a)) == ["quadtree_final_gpu.txt", "quadtree_init_gpu.txt"]
    rows = [line.split(",") for line in (b / "energy.csv").read_text().splitlines()]
    assert [int(r[0]) for r in rows] == [0, 3, 6, 7]
    assert all(len(r) == 8 for r in rows)
    vals = np.array([[float(x) for x in r] for r in rows])
    assert np.array_equal(vals[:, 1], vals[:, 0] * 1.0)                   # t = step * dt (dt = 1)
    assert np.array_equal(vals[:, 4], vals[:, 2] + vals[:, 3])             # (%.17g round-trips the doubles)
