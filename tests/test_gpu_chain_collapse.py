"""The fp32 / mixed step build links past single-child cell chains (nodes_fast_kernel, COLLAPSE; BH_CHAIN_COLLAPSE=0 keeps
every link): a slot whose cell Z_1 is the top of a chain Z_1 > Z_2 > ... > Z_k of cells with one and the same body range
carries Z_k's quad and Z_k's threshold, so no walk visits the quads in between.  Every case here runs the same input on
two contexts, one with the switch on and one with it off, and asserts what DESIGN.md section 4.5 claims:

  * no lane's node set moves: the per-body interaction counts and `interactions` are identical;
  * the waves do less: `wave_quads` and `wave_nodes` are strictly smaller with the switch on wherever the input has
    chains, and equal where it has none;
  * the accelerations agree to fp32 summation order -- the bound of test_split_walk_equals_the_one_wave_walk (relative
    L2 error per body: median < 5e-7, every body < 1e-4).  NOT bitwise: the two-entries-per-iteration machine pairs
    stack entries differently once the chain quads are gone;
  * with the switch on the hand-scheduled walk still equals the C++ loop bit for bit;
  * the exported tree is the reference's tree either way, element for element;
  * no bucket-sort or tree counter changes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd.engine import (FLAG_LDS_STACK, FLAG_WALK_NO_SPLIT, FLAG_WALK_PORTABLE,  # noqa: E402
                                             FLAG_WALK_STATS)

TOL_MEDIAN, TOL_MAX = 5e-7, 1e-4            # test_split_walk_equals_the_one_wave_walk (tests/test_gpu_fp32.py)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def walk(monkeypatch, collapse, inputs, export=False, **cfg):
    """One context, one force evaluation.  -> accelerations, per-body counts (FLAG_WALK_STATS only), stats, exported tree."""
    m, p, v = inputs
    monkeypatch.setenv("BH_CHAIN_COLLAPSE", "1" if collapse else "0")
    cfg.setdefault("precision", G.Precision.F32)
    with G.BarnesHutEngine(G.BhConfig(capacity=len(m), **cfg)) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a = e.accelerations()
        counts = e.interaction_counts() if cfg.get("flags", 0) & FLAG_WALK_STATS else None
        st = e.stats()
        tree = e.export_tree() if export else None           # (after the walk: the export re-runs the node kernel)
    return a, counts, st, tree


def same_forces_to_summation_order(a_on, a_off):
    assert np.isfinite(a_on).all() and np.isfinite(a_off).all()
    norm = np.linalg.norm(a_off, axis=1)
    still = norm == 0
    assert np.array_equal(a_on[still], a_off[still])
    if (~still).any():
        r = np.linalg.norm(a_on[~still] - a_off[~still], axis=1) / norm[~still]
        print("relative difference on / off: median %.3g, max %.3g" % (np.median(r), r.max()))
        assert np.median(r) < TOL_MEDIAN and r.max() < TOL_MAX, (np.median(r), r.max())


def same_trees(t_on, t_off):
    (n1, d1), (n0, d0) = t_on, t_off
    assert len(n1) == len(n0) and np.array_equal(d1, d0)
    for f in n1.dtype.names:
        assert np.array_equal(n1[f], n0[f], equal_nan=True), f


def check_on_against_off(monkeypatch, inputs, chains, export=True, **cfg):
    """The counting walk (FLAG_WALK_STATS) with the switch on and off; -> the two stats records."""
    cfg["flags"] = cfg.get("flags", 0) | FLAG_WALK_STATS
    a1, c1, s1, t1 = walk(monkeypatch, True, inputs, export=export, **cfg)
    a0, c0, s0, t0 = walk(monkeypatch, False, inputs, export=export, **cfg)
    print("on : interactions %d wave_quads %d wave_nodes %d" % (s1.interactions, s1.wave_quads, s1.wave_nodes))
    print("off: interactions %d wave_quads %d wave_nodes %d" % (s0.interactions, s0.wave_quads, s0.wave_nodes))
    assert np.array_equal(c1, c0)
    assert s1.interactions == s0.interactions and s1.interactions == int(c1.sum(dtype=np.int64))
    if chains:
        assert s1.wave_quads < s0.wave_quads and s1.wave_nodes < s0.wave_nodes
    else:
        assert s1.wave_quads == s0.wave_quads and s1.wave_nodes == s0.wave_nodes
    same_forces_to_summation_order(a1, a0)
    if export:
        same_trees(t1, t0)
    assert (s1.n_nodes, s1.n_internal, s1.sort_spill_buckets, s1.sort_rerun_buckets, s1.walk_launches) == \
           (s0.n_nodes, s0.n_internal, s0.sort_spill_buckets, s0.sort_rerun_buckets, s0.walk_launches)
    return s1, s0


def check_asm_equals_portable(monkeypatch, inputs, **cfg):
    """Switch on: the hand-scheduled loop of this launch size against the C++ statement of the same machine, bitwise."""
    flags = cfg.pop("flags", 0)
    a_asm = walk(monkeypatch, True, inputs, flags=flags, **cfg)[0]
    a_cxx = walk(monkeypatch, True, inputs, flags=flags | FLAG_WALK_PORTABLE, **cfg)[0]
    assert np.array_equal(a_asm, a_cxx)
    return a_asm


def with_tight_pairs(n, pairs, seed):
    """n bodies in [-1, 1]^2, the last `pairs` of them 2.4e-6 (1e-6 of the padded box's width) from one of the others."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n - pairs, 2))
    partner = rng.choice(n - pairs, pairs, replace=False)
    ang = rng.uniform(0, 2 * np.pi, pairs)
    p = f32(np.concatenate([p, p[partner] + 2.4e-6 * np.stack([np.cos(ang), np.sin(ang)], axis=1)]))
    return f32(rng.uniform(0.5, 1.5, n)), p, np.zeros((n, 2))


@pytest.mark.parametrize("hilbert", ["1", "0"])
@pytest.mark.parametrize("precision", [G.Precision.F32, G.Precision.MIXED])
def test_tight_pairs(monkeypatch, precision, hilbert):
    """4,096 uniform bodies and 64 pairs at 1e-6 of the box width, max_depth 21: a pair leaves its neighbours around depth 6
    and splits around depth 19 or 20 (or shares its depth-cap cell) -- chains of a dozen cells, on either curve."""
    monkeypatch.setenv("BH_HILBERT", hilbert)
    inputs = with_tight_pairs(4096 + 128, 64, 41)
    cfg = dict(max_depth=21, reference_compat=False, precision=precision)
    check_on_against_off(monkeypatch, inputs, chains=True, flags=FLAG_WALK_NO_SPLIT, **cfg)
    check_asm_equals_portable(monkeypatch, inputs, flags=FLAG_WALK_NO_SPLIT, **cfg)


@pytest.mark.parametrize("compat", [True, False])
def test_chain_that_ends_at_the_depth_cap(monkeypatch, compat):
    """max_depth 6 (cells down to depth 5).  Four corner bodies pin the root box to [-1.2, 1.2]^2; two clumps of five bodies
    sit in the middle of one depth-5 cell each (width 0.075) at (-0.2625, -+0.2625), and everything else lies at x > 0.1.  A
    clump is alone in its cell from depth 2 on: the chain is the cells of depth 2, 3 and 4, and the last one's quad holds
    the depth-cap cell -- an aggregate (reference_compat) or a bucket -- which is still reached through that quad."""
    rng = np.random.default_rng(43)
    corners = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])
    back = np.stack([rng.uniform(0.1, 0.9, 64), rng.uniform(-0.9, 0.9, 64)], axis=1)
    clumps = [np.array([-0.2625, s * 0.2625]) + rng.uniform(-1e-3, 1e-3, (5, 2)) for s in (-1.0, 1.0)]
    p = f32(np.concatenate([corners, back] + clumps))
    inputs = (f32(rng.uniform(0.5, 1.5, len(p))), p, np.zeros((len(p), 2)))
    cfg = dict(max_depth=6, reference_compat=compat)
    s1, s0 = check_on_against_off(monkeypatch, inputs, chains=True, flags=FLAG_WALK_NO_SPLIT, **cfg)
    nodes, depth = walk(monkeypatch, True, inputs, export=True, **cfg)[3]
    cap = (depth == 5) & (nodes["mass"] > 0) & (nodes["particle"] == -1.0)       # depth-cap cells of several bodies
    assert cap.sum() >= 2
    check_asm_equals_portable(monkeypatch, inputs, flags=FLAG_WALK_NO_SPLIT, **cfg)


def test_lattice_without_chains(monkeypatch):
    """A 64 x 64 lattice of spacing a, jittered by 5 % of a, without the 4 x 4 points of each corner.  The root box is padded
    by a tenth of the extent, 6.3 a, and a depth-3 cell is 9.46 a wide: the corner cell of a FULL lattice holds the 4 x 4
    corner points in its inner child alone -- a chain that every input filling its bounding box has, four times.  With those
    points gone (the bounding box stays) the corner cells are empty, and nothing else has a single non-empty child: a cell
    at least 2 a wide has a lattice point in every child that reaches into the lattice, a cell on the lattice's edge has two
    such children along the edge, and a narrower cell (1.18 a at depth 6) holds at most 2 x 2 points with its 0.59 a
    children holding at most one each.  So the switch changes no link, no counter and no bit of the result."""
    rng = np.random.default_rng(47)
    a = 2.0 / 64
    k = np.arange(64)
    g = -1.0 + (k + 0.5) * a
    ix, iy = np.meshgrid(k, k)
    corner = (((ix < 4) | (ix >= 60)) & ((iy < 4) | (iy >= 60))).reshape(-1)
    p = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2) + rng.uniform(-0.05 * a, 0.05 * a, (4096, 2))
    p = p[~corner]
    inputs = (f32(rng.uniform(0.5, 1.5, len(p))), f32(p), np.zeros((len(p), 2)))
    cfg = dict(max_depth=21, reference_compat=False)
    a1 = walk(monkeypatch, True, inputs, flags=FLAG_WALK_NO_SPLIT, **cfg)[0]
    a0 = walk(monkeypatch, False, inputs, flags=FLAG_WALK_NO_SPLIT, **cfg)[0]
    assert np.array_equal(a1, a0)                                # the same links: the same machine, bit for bit
    check_on_against_off(monkeypatch, inputs, chains=False, flags=FLAG_WALK_NO_SPLIT, **cfg)


@pytest.mark.parametrize("compat", [True, False])
def test_root_chain(monkeypatch, compat):
    """The root box is the bodies' bounding box padded by a tenth of its larger extent on every side, so the bodies
    straddle the middle of every axis they extend along: the root has a single non-empty child only when ALL bodies
    coincide (both extents zero, the box padded by 1e-6).  That input can be constructed and is the one here: five bodies at
    one place, max_depth 6 -- every key equal, a chain from the root (depth 0) to depth 4 and one depth-cap cell.  The
    root record links to the depth-4 quad: the wave that holds the bodies loads the root quad and that one instead of the root
    quad and the five of depth 0 .. 4 (the workgroup's three idle waves load the root quad either way).  Coincident bodies
    exert no force."""
    p = np.tile(f32(np.array([[0.3, 0.4]])), (5, 1))
    inputs = (f32(np.linspace(0.5, 1.5, 5)), p, np.zeros((5, 2)))
    cfg = dict(max_depth=6, reference_compat=compat)
    s1, s0 = check_on_against_off(monkeypatch, inputs, chains=True, flags=FLAG_WALK_NO_SPLIT, **cfg)
    assert s0.wave_quads - s1.wave_quads == 4 and s0.wave_nodes - s1.wave_nodes == 4      # the quads of depth 0 .. 3
    a = check_asm_equals_portable(monkeypatch, inputs, flags=FLAG_WALK_NO_SPLIT, **cfg)
    assert np.array_equal(a, np.zeros((5, 2)))


_LAUNCH_INPUTS = {}


def launch_inputs(n):
    if n not in _LAUNCH_INPUTS:
        _LAUNCH_INPUTS[n] = with_tight_pairs(n, n // 64, 53 + n)
    return _LAUNCH_INPUTS[n]


@pytest.mark.parametrize("variant", ["split", "lds_stack", "portable", "n_threads"])
@pytest.mark.parametrize("n", [5000, 70000])
def test_launch_sizes_and_variants(monkeypatch, n, variant):
    """5,000 bodies walk level by level with 8 wavefronts per group, 70,000 with 4 (the frontier of a level then holds the
    chains' last quads instead of their first); the LDS-stack walk, the C++ loop and passes of n_threads = 1,000 bodies
    run one wavefront per group.  All of them through the counting kernels, switch on against switch off; the split walk's
    hand-scheduled chunk loop also against its C++ statement with the switch on, and against itself with it off."""
    inputs = launch_inputs(n)
    cfg = dict(max_depth=21, reference_compat=False)
    if variant == "n_threads":
        cfg["n_threads"] = 1000
    flags = {"split": 0, "lds_stack": FLAG_LDS_STACK, "portable": FLAG_WALK_PORTABLE, "n_threads": 0}[variant]
    check_on_against_off(monkeypatch, inputs, chains=True, export=(n == 5000 and variant == "split"), flags=flags, **cfg)
    if variant in ("split", "n_threads"):
        a1 = check_asm_equals_portable(monkeypatch, inputs, flags=flags, **cfg)
        same_forces_to_summation_order(a1, walk(monkeypatch, False, inputs, flags=flags, **cfg)[0])
