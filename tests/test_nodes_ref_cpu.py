"""tests/nodes_ref.py can fail: the device path of the fp32 / mixed node records emulated in numpy -- bodies in the oracle's
DFS leaf order, fp64 cumsum of (m, m x, m y), differences at the cell boundaries, fp32 cast -- stays inside the derived bound,
and the three ways a node kernel or a scan goes subtly wrong leave it: a child boundary off by one body, a tile's carry
dropped from the prefix sums, and (through the same comparison) any topology difference.  cumsum is sequential, so H = n here
and only here.  No GPU."""
import numpy as np
import pytest

import nodes_ref as R

CASES = {"a": (1e-4, 21, False), "b": (2e-5, 12, False), "spill": (1e-4, 12, True)}


@pytest.fixture(scope="module")
def twins():
    cache = {}

    def get(case, mixed):
        if (case, mixed) not in cache:
            w, md, straddle = CASES[case]
            p, m = R.cluster_case(w, straddle)
            cache[case, mixed] = R.Twin(R.off_grid(p), m, md) if mixed else R.Twin(R.f32(p), R.f32(m), md)
        return cache[case, mixed]

    return get


def cluster_cells(tw):
    """One reference cell per population: the deepest subdivided cell that holds exactly that many bodies (the one whose children share
    the cluster out)."""
    cells = []
    for k in R.POPULATIONS:
        hit = np.flatnonzero((tw.cnt == k) & tw.has)
        assert hit.size, k
        cells.append(int(hit[np.argmax(tw.depth[hit])]))
    return cells


def parent_of(tw, k):
    """Pre-order: the last subdivided node of the depth above, before k."""
    cand = np.flatnonzero(tw.has & (tw.depth == tw.depth[k] - 1))
    return int(cand[np.searchsorted(cand, k) - 1])


def test_chain_length():
    assert R.prefix_chain(17644) == 44 and R.prefix_chain(2048 * 512 - 1) == 44
    assert R.prefix_chain(2048 * 512 + 513) == 45                               # 2,050 tiles of 512: nine chunks in scan_top2
    assert R.prefix_chain((1 << 30) - 1) == 36 + 8192


@pytest.mark.parametrize("mixed", [False, True])
def test_the_construction_gives_the_populations(twins, mixed):
    n = R.N_UNIFORM + 4 + sum(R.POPULATIONS)
    assert n == 17644
    a, b = twins("a", mixed), twins("b", mixed)
    assert a.n == b.n == n
    # a: every cluster is a cell of its own that subdivides, down to depth 14 ... 20
    for c in cluster_cells(a):
        assert a.has[c]
    big = a.has & (a.cnt >= 9) & (a.depth >= 14)
    assert big.any() and a.depth.max() == 20
    # ... with chains of nested cells that start at the same body
    assert (a.lo[a.kids[a.has, 0]] == a.lo[a.has]).any()
    # b: every cluster is ONE depth-cap cell of exactly its population, under ancestors that hold the same bodies
    caps = b.cnt[~b.has & (b.depth == 11)]
    assert sorted(caps[caps >= 7].tolist()) == sorted(k for k in R.POPULATIONS if k >= 7)      # no other body in them
    for k in R.POPULATIONS:
        cap = np.flatnonzero((b.cnt == k) & ~b.has & (b.depth == 11))
        assert cap.size >= 1 and any(b.cnt[parent_of(b, c)] == k for c in cap)
    # the corners are the first and the last bodies of the DFS order (and of the Hilbert order: the curve starts and ends there)
    corners = set(range(R.N_UNIFORM, R.N_UNIFORM + 4))
    assert int(a.order[0]) in corners and int(a.order[-1]) in corners


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_the_emulation_stays_inside_the_bound(twins, case, mixed):
    tw = twins(case, mixed)
    nodes, depth = tw.emulate_export()
    res = tw.check(nodes, depth, mixed, H=tw.n)
    assert res["nodes"] == len(tw.ref) and res["unresolved"] == 0 and res["undecided"] == 0
    # and the oracle's own fp64 records are these sums to its rounding: (levels + bodies of a cap cell) * 2^-53 of the cell's sums
    big = tw.cnt >= 2
    # (three additions per level, and the running sum of the largest depth-cap cell below)
    units = (3 * (tw.depth.max() - tw.depth) + tw.cnt[~tw.has].max() + 4) * R.U53
    M, X, Y = (a.astype(np.float64) for a in (tw.M, tw.X, tw.Y))
    assert (np.abs(tw.ref["mass"] - M)[big] <= (units * M)[big]).all()
    # (positive masses: the sum of |m x| over a cell is at most M * max |x|)
    assert (np.abs(tw.ref["comx"] - X)[big] <= (4 * units * 1.2)[big]).all()
    assert (np.abs(tw.ref["comy"] - Y)[big] <= (4 * units * 1.2)[big]).all()


@pytest.mark.parametrize("mixed", [False, True])
def test_the_cut_off_and_cells_the_prefix_sums_do_not_resolve(mixed):
    """Masses over six decades with every 9th body at 1e-16 (case e of tests/test_gpu_nodes_fp32.py): one-body records under the
    1e-15f cut-off are (0, 0, 0); a pair of such bodies alone in a cell is lighter than the prefix sums resolve, the twin
    follows the export there, counts the cell -- and still refuses a record under the cut-off that is not (0, 0, 0)."""
    p, m = R.cluster_case(1e-4)
    m = 10.0 ** np.random.default_rng(5).uniform(-4, 2, len(m))
    m[::9] = 1e-16
    tw = R.Twin(R.off_grid(p), m, 21) if mixed else R.Twin(R.f32(p), R.f32(m), 21)
    pair = np.flatnonzero(tw.has & (tw.cnt == 2) & (tw.M < 1e-15))
    assert pair.size >= 1
    nodes, depth = tw.emulate_export()
    res = tw.check(nodes, depth, mixed, H=tw.n)
    assert res["undecided"] >= 1 and res["nodes"] < len(tw.ref), res
    k = int(np.flatnonzero((nodes["mass"] == 0) & (nodes["particle"] >= 0) & (nodes["particle"] % 9 == 0))[0])
    assert nodes["comx"][k] == 0 and nodes["comy"][k] == 0
    bad = nodes.copy()
    bad["comx"][k] = 0.25                                                       # a record under the cut-off keeps no centre
    with pytest.raises(AssertionError):
        tw.check(bad, depth, mixed, H=tw.n)


@pytest.mark.parametrize("mixed", [False, True])
def test_a_topology_difference_fails(twins, mixed):
    tw = twins("a", mixed)
    nodes, depth = tw.emulate_export()
    with pytest.raises(AssertionError):
        tw.check(nodes[:-4], depth[:-4], mixed, H=tw.n)
    bad = nodes.copy()
    k = int(np.flatnonzero(tw.cnt == 1)[7])
    bad["particle"][k] += 1
    with pytest.raises(AssertionError):
        tw.check(bad, depth, mixed, H=tw.n)
    bad = nodes.copy()
    bad["comx"][k] = np.nextafter(np.float32(bad["comx"][k]), np.float32(9))    # a one-body record: ==, not a bound
    with pytest.raises(AssertionError):
        tw.check(bad, depth, mixed, H=tw.n)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", ["a", "b"])
def test_a_child_boundary_off_by_one_body_breaks_the_bound(twins, case, mixed):
    """In every cluster cell (case b: the cell above the cluster's depth-cap cell, whose boundaries cut the cluster out), each
    of the three child boundaries moved by one body either way: both children next to it leave the mass bound."""
    tw = twins(case, mixed)
    P = tw.prefix()
    cells = cluster_cells(tw)
    if case == "b":
        cells = [parent_of(tw, int(np.flatnonzero((tw.cnt == k) & ~tw.has & (tw.depth == 11))[-1])) for k in R.POPULATIONS]
    for cell in cells:
        kids = tw.kids[cell]
        moved = 0
        for c in (1, 2, 3):
            for s in (-1, 1):
                lo, hi = tw.lo[kids].copy(), tw.hi[kids].copy()
                lo[c] += s
                hi[c - 1] += s
                if (hi - lo < 0).any():
                    continue                                                    # the neighbour is empty: nothing to move
                pair = [c - 1, c]
                m, cx, cy = tw.records(P, kids[pair], lo[pair], hi[pair])
                rm, _, _ = tw.judge(kids[pair], m, cx, cy, mixed, H=tw.n)
                assert (rm > 1.0).all(), (cell, c, s, rm)
                moved += 1
        # (unmoved, the same records pass)
        m, cx, cy = tw.records(P, kids)
        assert (np.array(tw.judge(kids, m, cx, cy, mixed, H=tw.n)) <= 1.0).all()
        assert moved >= 1, cell


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("tile", [1, 17, 34])
def test_a_dropped_tile_carry_breaks_the_bound(twins, tile, mixed):
    """scan_apply2 adds a carry (the sum of all earlier tiles) to its tile's local prefix sums.  Without it -- dcarry zeroed for
    one 512-body tile -- every cell that spans the tile's leading edge leaves the mass bound, and the comparison says so."""
    tw = twins("a", mixed)
    t = tw.terms()
    P = tw.prefix()
    e0, e1 = 512 * tile, min(512 * (tile + 1), tw.n + 1)
    assert e1 <= tw.n + 1
    local = np.zeros((e1 - e0, 3))
    local[1:] = np.cumsum(t[e0:e1 - 1], axis=0)
    P[e0:e1] = local
    k = np.flatnonzero((tw.lo < e0) & (tw.hi > e0) & (tw.hi < e1))
    assert k.size >= 1
    rm, _, _ = tw.judge(k, *tw.records(P, k), mixed, H=tw.n)
    assert (rm > 1.0).all()
    with pytest.raises(AssertionError):
        tw.check(*tw.emulate_export(P), mixed, H=tw.n)
