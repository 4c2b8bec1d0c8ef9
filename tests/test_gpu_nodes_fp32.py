"""Every node record of the fp32 and mixed builds (nodes_fast_kernel and the prefix sums behind it: prep_kernel,
scan_apply2<FOLD or not, TSRC or not>, scan_top2) against exact sums over the oracle's cells, at the edges of the kernel's
search paths.  upload; build_tree; export_tree; then tests/nodes_ref.py's Twin.check for EVERY exported node: length, depth,
boxes and has-child flags == the oracle's, particle == the oracle's where a leaf holds one body and -1 elsewhere (depth-cap
leaves of several bodies included), one-body records == the body's fp32 copies, mass and centre of every larger cell inside the
bound derived in tests/nodes_ref.py (H additions between a term and a prefix sum, counted from the code; no tolerance here comes
from a device run).  Each case prints its largest error / bound ratios; a failure shows them with the offending node.

The base input (nodes_ref.cluster_case): 6,000 uniform bodies, the four box corners (first and last of the sorted order on
both curves: i == 0 and i + 8 >= n), and clusters of 2 ... 2,049 bodies that straddle the 8-key fast path (8 | 9), the 768-key
halo of the LDS window, 4 * kCoarse = 1,024 with the gallop's 2 * kCoarse stop, and kMaxBucket.  tests/test_nodes_ref_cpu.py
checks on the CPU that the construction gives cells of exactly these populations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
import nodes_ref as R  # noqa: E402

PRECISIONS = [pytest.param(False, id="f32"), pytest.param(True, id="mixed")]
_twins = {}


def inputs(p, m, mixed, cluster=True):
    """What the device holds: fp32 values for Precision.F32, fp64 values off the fp32 grid for Precision.MIXED."""
    if mixed:
        p = R.off_grid(p) if cluster else p
        assert not np.array_equal(p, R.f32(p))
        return p, m
    return R.f32(p), R.f32(m)


def twin(key, p, m, md):
    if key not in _twins:
        _twins[key] = R.Twin(p, m, md)
    return _twins[key]


def export(p, m, mixed, md, compat=False, builds=1):
    n = len(m)
    cfg = G.BhConfig(capacity=n, precision=G.Precision.MIXED if mixed else G.Precision.F32, max_depth=md, reference_compat=compat)
    with G.BarnesHutEngine(cfg) as e:
        e.upload(p, np.zeros((n, 2)), m)
        for _ in range(builds):
            e.build_tree()
        return e.export_tree()


def compare(tw, nodes, depth, mixed, label):
    res = tw.check(nodes, depth, mixed)
    print(f"{label} {'mixed' if mixed else 'f32'}: n = {tw.n}, H = {tw.H}, error / bound: {res}")
    return res


def cluster(w, md, mixed, straddle=False, mass=None):
    p, m = R.cluster_case(w, straddle)
    if mass is not None:
        m = mass(len(m))
    p, m = inputs(p, m, mixed)
    return p, m, twin((w, md, mixed, straddle, mass), p, m, md)


@pytest.mark.parametrize("mixed", PRECISIONS)
def test_a_subdividing_clusters(mixed):
    """max_depth 21, w = 1e-4: the clusters subdivide -- cells of every intermediate size at depths 14 ... 20, chains of nested
    cells that start at the same body."""
    p, m, tw = cluster(1e-4, 21, mixed)
    res = compare(tw, *export(p, m, mixed, 21), mixed, "a")
    assert res["nodes"] == len(tw.ref) and res["undecided"] == 0 and res["unresolved"] == 0


@pytest.mark.parametrize("mixed", PRECISIONS)
@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("w,straddle", [(2e-5, False), (1e-4, True)])
def test_b_clusters_in_depth_cap_cells(w, straddle, compat, mixed):
    """max_depth 12.  w = 2e-5: every cluster sits in ONE depth-cap cell of exactly its population under ancestors that hold the
    same bodies (compat off: a bucket up to kMaxBucket = 1,024 bodies and an aggregate above; compat on: aggregates).
    w = 1e-4 about a cell corner: the clusters spill over four cap cells."""
    p, m, tw = cluster(w, 12, mixed, straddle)
    res = compare(tw, *export(p, m, mixed, 12, compat), mixed, f"b w={w} compat={compat}")
    assert res["nodes"] == len(tw.ref)


@pytest.mark.parametrize("mixed", PRECISIONS)
@pytest.mark.parametrize("var,val", [("BH_HILBERT", "0"), ("BH_BUILD_ITEMS", "2"), ("BH_BUILD_ITEMS", "4"), ("BH_BUILD_ITEMS", "8")])
def test_c_other_curve_and_tile_sizes_give_the_same_tree(monkeypatch, var, val, mixed):
    """Case a in child-index key order (BH_HILBERT=0) and with 512-, 1,024- and 2,048-key scan tiles: the exported tree is the same tree."""
    monkeypatch.setenv(var, val)
    p, m, tw = cluster(1e-4, 21, mixed)
    res = compare(tw, *export(p, m, mixed, 21), mixed, f"c {var}={val}")
    assert res["nodes"] == len(tw.ref)


@pytest.mark.parametrize("mixed", PRECISIONS)
def test_d_reordered_state_and_bucket_sorted_builds(monkeypatch, mixed):
    """Case a under BH_REORDER_EVERY=2 after three build_tree() calls: the state is physically re-ordered, the second and third
    builds take the bucket sort; `particle` still speaks the caller's indices."""
    monkeypatch.setenv("BH_REORDER_EVERY", "2")
    p, m, tw = cluster(1e-4, 21, mixed)
    res = compare(tw, *export(p, m, mixed, 21, builds=3), mixed, "d")
    assert res["nodes"] == len(tw.ref)


def masses_six_decades(n):
    return 10.0 ** np.random.default_rng(5).uniform(-4, 2, n)


def masses_with_dust(n):
    m = masses_six_decades(n)
    m[::9] = 1e-16
    return m


@pytest.mark.parametrize("mixed", PRECISIONS)
@pytest.mark.parametrize("mass", [masses_six_decades, masses_with_dust])
def test_e_mass_range_and_the_cut_off(mass, mixed):
    """Case a with masses 10^U(-4, 2), and with every 9th body at 1e-16: one-body records below the 1e-15f cut-off are stored as
    (0, 0, 0), and so is a pair of 1e-16 bodies alone in a cell -- as far as the prefix sums resolve it (tests/nodes_ref.py,
    PRUNING: the twin follows the export where the bound cannot decide, and says how often)."""
    p, m, tw = cluster(1e-4, 21, mixed, mass=mass)
    if mass is masses_with_dust:
        assert (tw.has & (tw.cnt == 2) & (tw.M < 1e-15)).any()                      # the pair, alone in a subdivided cell
    compare(tw, *export(p, m, mixed, 21), mixed, f"e {mass.__name__}")


@pytest.mark.parametrize("mixed", PRECISIONS)
@pytest.mark.parametrize("compat", [False, True])
def test_f_tiny_and_root_only_trees(compat, mixed):
    """n = 1, n = 2, two coincident bodies, and max_depth = 1 (no subdivided cell: the `total == 0` path) with a handful of
    bodies and with more than kMaxBucket."""
    rng = np.random.default_rng(31)
    for label, p, md in (("n=1", np.array([[0.3, -0.7]]), 21), ("n=2", rng.uniform(-1, 1, (2, 2)), 21),
                         ("coincident", np.array([[0.3, 0.3], [0.3, 0.3]]), 21), ("n=1 depth 1", np.array([[0.3, -0.7]]), 1),
                         ("n=5 depth 1", rng.uniform(-1, 1, (5, 2)), 1), ("n=2 depth 2", rng.uniform(-1, 1, (2, 2)), 2)):
        m = rng.uniform(0.1, 0.5, len(p))
        pp, mm = inputs(p, m, mixed, cluster=False)
        tw = R.Twin(pp, mm, md)
        compare(tw, *export(pp, mm, mixed, md, compat), mixed, f"f {label} compat={compat}")
    p, m, tw = cluster(1e-4, 1, mixed)
    res = compare(tw, *export(p, m, mixed, 1, compat), mixed, f"f root of {len(m)} compat={compat}")
    assert res["nodes"] == 1


@pytest.mark.parametrize("mixed", PRECISIONS)
@pytest.mark.parametrize("case,cells", [(R.CELLS_256, 256), (R.CELLS_257, 257)])
def test_f_full_and_ragged_last_workgroup(case, cells, mixed):
    """256 subdivided cells fill the node kernel's one workgroup; 257 leave a second one with a single cell."""
    p, m = R.uniform_case(*case)
    p, m = inputs(p, m, mixed, cluster=False)
    tw = twin(("cells", cells, mixed), p, m, 21)
    assert tw.has.sum() == cells
    compare(tw, *export(p, m, mixed, 21), mixed, f"f {cells} cells")


@pytest.mark.parametrize("mixed", PRECISIONS)
def test_g_more_than_2048_tiles(monkeypatch, mixed):
    """The path that does not pre-sum the tile totals (scan_top2 + scan_apply2<..., FOLD = false>) needs more than 8 * 256 tiles:
    512-key tiles (BH_BUILD_ITEMS=2) and n = 2,048 * 512 + 513 uniform bodies.  Every node, vectorised."""
    monkeypatch.setenv("BH_BUILD_ITEMS", "2")
    n = 2048 * 512 + 513
    p, m = R.uniform_case(n, 7)
    p, m = inputs(p, m, mixed, cluster=False)
    tw = R.Twin(p, m, 21)
    assert tw.H == 45
    res = compare(tw, *export(p, m, mixed, 21), mixed, "g")
    assert res["nodes"] == len(tw.ref)
