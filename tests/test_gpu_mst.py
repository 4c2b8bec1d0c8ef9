"""bh_spanning_tree, bh_spanning_tree_subsets and mass_segregation on the device, held to the brute-force twin tests/mst_ref.py: lo,
hi and d2 are compared with np.array_equal, on the state DOWNLOADED from the engine (in F32 that is the fp32 state as the device
holds it).  The tree is unique under the edge order (d2, lo, hi), so there is one right answer.

  1. the edges of the definition: one body, two, ties decided by index (three collinear bodies, a square), a lattice of ties;
  2. degenerate boxes: coincident bodies, a line, two clumps 1e12 apart (the last edge is the bridge);
  3. launch edges: sizes around a leaf, a wave, a workgroup and a second level of boxes;
  4. all four precisions on a Plummer sphere with outliers, and after steps (caller indices after a physical re-order);
  5. at size, where the twin is too big: groups_at(b) of the tree against groups(b) of the device -- two independent device
     algorithms -- on a spiral of 20,000 bodies and a uniform square of 50,000, with n - 1 edges, the order and acyclicity;
  6. the work counters;
  7. subsets: k around a wave and at the maximum, no set, one, 300; rows that share bodies, a row of coincident bodies; the mass
     segregation ratio;
  8. the errors of include/bhgpu.h (but BH_ERR_CAPACITY: more than 2^24 bodies are too many for a test);
  9. the run is not perturbed;
 10. project.py --mst-file and --segregation-file."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
import groups_ref as R  # noqa: E402
import mst_ref as M  # noqa: E402
import neighbours_ref as NR  # noqa: E402
import quiet_case as Q  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]
_TWINS = {}


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def upload(e, pos, vel=None, mass=None):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    e.upload(pos, np.zeros_like(pos) if vel is None else vel, np.full(len(pos), 1e-14) if mass is None else mass)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def twin_tree(pos):
    """the twin's tree of a state, computed once per state (F32 and MIXED, F64 and F64_EXACT hold the same positions)"""
    key = pos.tobytes()
    if key not in _TWINS:
        _TWINS[key] = M.tree(pos)
    return _TWINS[key]


def same_as_twin(e, what=""):
    """spanning_tree() of the engine's own state against the twin; returns the BhSpanningTree"""
    pos = e.download()[0]
    n = len(pos)
    lo, hi, d2 = twin_tree(pos)
    t = e.spanning_tree(with_stats=True)
    print(f"{what} n={n}: stats {t.stats}, total length {t.total_length!r}")
    assert t.n == n and t.lo.dtype == np.int64 and t.hi.dtype == np.int64 and t.d2.dtype == np.float64
    assert t.lo.shape == t.hi.shape == t.d2.shape == (max(n - 1, 0),)
    bad = np.nonzero((t.lo != lo) | (t.hi != hi) | (t.d2 != d2))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} edges differ; first {bad[0]}: got {(t.lo[bad[0]], t.hi[bad[0]], t.d2[bad[0]])}, "
                           f"twin {(lo[bad[0]], hi[bad[0]], d2[bad[0]])}")
    assert np.array_equal(t.lo, lo) and np.array_equal(t.hi, hi) and np.array_equal(t.d2, d2)
    assert np.array_equal(t.length, np.sqrt(d2)) and t.total_length == math.fsum(np.sqrt(d2).tolist())
    assert t.stats[3] == max(n - 1, 0) and t.stats[0] <= max(n - 1, 0).bit_length()
    return t


# ---- 1. the edges of the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_one_body_two_and_ties_decided_by_index(precision):
    with engine(4, precision) as e:
        upload(e, [[0.25, -3.0]])
        t = same_as_twin(e, "one body")
        assert len(t.lo) == 0 and t.stats == (0, 0, 0, 0) and t.total_length == 0.0 and list(t.groups_at(1.0)) == [0]
        upload(e, [[1.0, 2.0], [1.75, 3.0]])                       # 3-4-5: d2 = 1.5625 exactly
        t = same_as_twin(e, "two bodies")
        assert (list(t.lo), list(t.hi), list(t.d2)) == ([0], [1], [1.5625]) and t.stats[0] == 1
        assert list(t.n_groups_at([1.25, float(np.nextafter(1.25, 0.0))])) == [1, 2]
        upload(e, [[2.0, 0.0], [0.0, 0.0], [1.0, 0.0]])            # collinear, equidistant: two edges of d2 = 1, ordered by index
        t = same_as_twin(e, "three collinear")
        assert (list(t.lo), list(t.hi), list(t.d2)) == ([0, 1], [2, 2], [1.0, 1.0])
        upload(e, [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])  # a square: four edges tie, the last in the order is left out
        t = same_as_twin(e, "square")
        assert (list(t.lo), list(t.hi)) == ([0, 0, 1], [1, 3, 2])


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_lattice_of_ties(precision):
    h = 0.125
    with engine(256, precision) as e:
        upload(e, NR.lattice(16) * h)
        t = same_as_twin(e, "lattice")
        assert (t.d2 == h * h).all() and list(t.n_groups_at([h, float(np.nextafter(h, 0.0))])) == [1, 256]


# ---- 2. degenerate boxes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_degenerate_boxes(precision):
    rng = np.random.default_rng(31)
    with engine(400, precision) as e:
        upload(e, np.tile([[0.5, -0.125]], (100, 1)))              # thirteen one-point leaves
        t = same_as_twin(e, "coincident")
        assert (t.d2 == 0.0).all() and (t.lo == 0).all() and list(t.hi) == list(range(1, 100))     # the star on body 0
        upload(e, np.stack([f32(rng.normal(size=300)), np.full(300, 0.25)], axis=1))
        same_as_twin(e, "line")
        clumps = np.concatenate([f32(rng.normal(size=(150, 2))), f32(1e12 + rng.uniform(0.0, 4e6, size=(150, 2)))])
        order = rng.permutation(300)
        upload(e, clumps[order])
        t = same_as_twin(e, "two clumps")
        far = order >= 150                                         # (caller index c holds clumps[order[c]])
        assert far[t.lo[-1]] != far[t.hi[-1]] and (far[t.lo[:-1]] == far[t.hi[:-1]]).all()       # the last edge is the bridge
        assert t.d2[-1] > 1e23 and t.d2[-1] == twin_tree(e.download()[0])[2][-1]


# ---- 3. launch edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_launch_edges(precision, n):
    with engine(n, precision) as e:
        upload(e, f32(R.uniform_square(n, n)))
        same_as_twin(e, f"{precision.name} uniform")


# ---- 4. all four precisions, and caller indices after a physical re-order -----------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_all_precisions_before_and_after_steps(precision):
    n = 2000
    m, p, v = NR.plummer_with_outliers(n)
    with engine(n, precision) as e:
        e.upload(p, v, m)
        same_as_twin(e, f"{precision.name} plummer")
        e.step(21)
        t = same_as_twin(e, f"{precision.name} plummer after 21 steps")
        b = float(np.median(t.length))
        assert np.array_equal(t.groups_at(b), e.groups(b).label)


# ---- 5. the cross-check at size -------------------------------------------------------------------------------------------------
def exact_root(d2, around):
    """an index near `around` whose d2 is the exact square of its rounded root, and that root"""
    for k in range(around, len(d2)):
        b = float(np.sqrt(d2[k]))
        if b * b == d2[k] and (k + 1 == len(d2) or d2[k + 1] > d2[k]):
            return k, b
    raise AssertionError("no edge with an exact root")


def check_against_groups(e, what):
    n = e.n
    t = e.spanning_tree(with_stats=True)
    print(what, "stats", t.stats, "times", e.spanning_tree_times())
    assert len(t.lo) == n - 1 and t.stats[3] == n - 1 and 1 <= t.stats[0] <= (n - 1).bit_length()
    assert ((0 <= t.lo) & (t.lo < t.hi) & (t.hi < n)).all()
    # strictly ascending in the edge order
    d, a, c = t.d2, t.lo, t.hi
    later = (d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & ((a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (c[1:] > c[:-1]))))
    assert later.all()
    # n - 1 edges without a cycle: a spanning tree (labels_at asserts that no edge closes a cycle)
    label, left = M.labels_at(n, t.lo, t.hi, t.d2, float("inf"))
    assert left == 1 and (label == 0).all()
    k, b_at = exact_root(t.d2, (n - 1) // 2)
    below = float(np.nextafter(b_at, 0.0))
    assert t.n_groups_at(b_at) == n - 1 - k and t.n_groups_at(below) > n - 1 - k
    for b in (0.0, float(t.length[(n - 1) // 10]), below, b_at, float(t.length[-(n // 100)]), 2.0 * float(t.length[-1])):
        g = e.groups(b, 1)
        at = t.groups_at(b)
        bad = np.nonzero(at != g.label)[0]
        assert len(bad) == 0, f"{what} b={b!r}: {len(bad)} labels differ; first body {bad[0]}: tree {at[bad[0]]}, groups {g.label[bad[0]]}"
        assert t.n_groups_at(b) == g.n_groups, (what, b)
    return t


def test_spiral_of_twenty_thousand_against_groups():
    """long thin components: many rounds of chain merging"""
    n, b = 20000, 1.0 / 64
    pos, place = R.spiral(n, b)
    with engine(n, P.F32) as e:
        upload(e, pos)
        t = check_against_groups(e, "spiral F32")
        # the tree is the arm itself: every edge joins neighbours along it
        assert (np.abs(place[t.lo] - place[t.hi]) == 1).all() and t.length.max() <= 0.9 * b * (1 + 1e-4)


def test_uniform_square_of_fifty_thousand_against_groups():
    n = 50000
    with engine(n, P.F64) as e:
        upload(e, R.uniform_square(n, 7))
        check_against_groups(e, "uniform F64")


# ---- 6. the work counters -------------------------------------------------------------------------------------------------------
def test_stats_and_repeatability():
    n = 4096
    m, p, v = NR.uniform(n)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        a = e.spanning_tree(with_stats=True)
        again = e.spanning_tree(with_stats=True)
        print("stats", a.stats, again.stats, "times", e.spanning_tree_times())
        for x in ("lo", "hi", "d2"):
            assert np.array_equal(getattr(a, x), getattr(again, x)), x
        assert a.stats[0] <= 12 and a.stats[3] == n - 1
        assert a.stats == again.stats                             # the header declares all four counters deterministic
        assert n - 1 <= a.stats[1] <= 512 * n                      # the traversal prunes (the bound of the neighbour search's mean)
        bt, rt, st = e.spanning_tree_times()
        assert bt > 0.0 and rt > 0.0 and st >= 0.0
        before = e.stats().device_bytes
        e.spanning_tree()
        assert e.stats().device_bytes == before                    # the buffers are kept


# ---- 7. subsets -----------------------------------------------------------------------------------------------------------------
def subsets_same_as_twin(e, members, what):
    pos = e.download()[0]
    lo, hi, d2 = e.subset_spanning_trees(members)
    sets, k = members.shape
    assert lo.shape == hi.shape == d2.shape == (sets, k - 1) and lo.dtype == np.int64 and hi.dtype == np.int64
    tlo, thi, td2 = M.subset_trees(pos, members)
    for r in range(sets):
        assert np.array_equal(lo[r], tlo[r]) and np.array_equal(hi[r], thi[r]) and np.array_equal(d2[r], td2[r]), (what, r)
    print(what, members.shape, "times", e.spanning_tree_times())
    return lo, hi, d2


def test_subsets_against_the_twin_after_a_reorder():
    n = 2000
    m, p, v = NR.plummer_with_outliers(n)
    rng = np.random.default_rng(77)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        e.step(21)                                                 # (a physical re-order: caller indices are not slots any more)
        for k, sets in ((2, 300), (3, 300), (63, 1), (64, 40), (65, 1), (512, 1), (512, 3), (7, 0)):
            members = np.stack([rng.choice(n, k, replace=False) for _ in range(sets)]) if sets else np.zeros((0, k), dtype=np.int64)
            subsets_same_as_twin(e, members, f"F32 k={k}")
        # rows that share bodies: the same row twice, reversed, and a row that overlaps it
        row = rng.choice(n, 65, replace=False)
        other = np.concatenate([row[:30], np.setdiff1d(np.arange(n), row)[:35]])
        lo, hi, d2 = subsets_same_as_twin(e, np.stack([row, row[::-1], other]), "shared bodies")
        assert np.array_equal(lo[0], lo[1]) and np.array_equal(hi[0], hi[1]) and np.array_equal(d2[0], d2[1])
    # a row of coincident bodies; and all n <= 512 bodies as one set is the whole tree
    with engine(300, P.F64) as e:
        pos = f32(rng.normal(size=(300, 2)))
        pos[100:120] = pos[100]                                    # twenty coincident bodies
        upload(e, pos)
        members = np.stack([np.arange(100, 120)[::-1], rng.choice(300, 20, replace=False)])
        lo, hi, d2 = subsets_same_as_twin(e, members, "coincident row")
        assert (d2[0] == 0.0).all() and (lo[0] == 100).all() and list(hi[0]) == list(range(101, 120))
        t = e.spanning_tree()
        lo, hi, d2 = e.subset_spanning_trees(rng.permutation(300)[None, :])
        assert np.array_equal(lo[0], t.lo) and np.array_equal(hi[0], t.hi) and np.array_equal(d2[0], t.d2)


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_mass_segregation_equals_the_twin(precision):
    n = 1500
    m, p, v = NR.plummer_with_outliers(n)
    m = f32(m * np.random.default_rng(5).uniform(0.5, 2.0, size=n))
    with engine(n, precision) as e:
        e.upload(p, v, m)
        e.step(3)
        pos, mass = e.download()[0], e.masses()
        got = e.mass_segregation(10, 40, seed=3)
        ratio, sigma, l_massive, l_random, members = M.mass_segregation(pos, mass, 10, 40, 3)
        print(precision.name, "ratio", got.ratio, "sigma", got.sigma)
        assert np.array_equal(got.members, members) and got.n_massive == 10
        assert (got.ratio, got.sigma, got.l_massive) == (ratio, sigma, l_massive) and np.array_equal(got.l_random, l_random)
        # other weights: the bodies nearest the centre are "massive" -- segregated by construction
        w = -np.hypot(pos[:, 0], pos[:, 1])
        seg = e.mass_segregation(10, 40, seed=3, weights=w)
        assert seg.ratio == M.mass_segregation(pos, w, 10, 40, 3)[0] and seg.ratio > 1.0


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------
def code_and_text(f, *a, **kw):
    try:
        f(*a, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_errors():
    rng = np.random.default_rng(61)
    pos = f32(rng.normal(size=(1000, 2)) * 0.05)
    rows = np.stack([rng.choice(1000, 8, replace=False) for _ in range(4)])
    i64 = C.POINTER(C.c_int64)
    with engine(1000, P.F64) as e:
        assert code_and_text(e.spanning_tree)[0] == ERR_STATE        # before upload
        assert code_and_text(e.subset_spanning_trees, rows)[0] == ERR_STATE
        upload(e, pos)
        assert code_and_text(e.spanning_tree)[0] == 0 and code_and_text(e.subset_spanning_trees, rows)[0] == 0
        lib, h = e._lib, e._h
        lo, hi, d2 = np.zeros(999, dtype=np.int64), np.zeros(999, dtype=np.int64), np.zeros(999)
        plo, phi, pd2 = lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), d2.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.bh_spanning_tree(h, plo, phi, pd2, None) == 0
        for args in ((None, phi, pd2), (plo, None, pd2), (plo, phi, None)):
            assert lib.bh_spanning_tree(h, *args, None) == ERR_ARG
        assert lib.bh_spanning_tree(None, plo, phi, pd2, None) == ERR_ARG
        assert lib.bh_spanning_tree_times(h, None, None, None) == ERR_ARG
        pm = rows.ctypes.data_as(i64)
        assert lib.bh_spanning_tree_subsets(h, pm, 4, 8, plo, phi, pd2) == 0
        assert lib.bh_spanning_tree_subsets(h, None, 4, 8, plo, phi, pd2) == ERR_ARG
        assert lib.bh_spanning_tree_subsets(h, pm, 4, 8, None, phi, pd2) == ERR_ARG
        assert lib.bh_spanning_tree_subsets(h, pm, -1, 8, plo, phi, pd2) == ERR_ARG
        assert lib.bh_spanning_tree_subsets(h, pm, 0, 8, None, None, None) == 0
        for k in (0, 1, 513):
            assert lib.bh_spanning_tree_subsets(h, pm, 1, k, plo, phi, pd2) == ERR_ARG, k
        for bad, word in ((-1, "outside"), (1000, "outside"), (int(rows[2, 0]), "twice")):
            r = rows.copy()
            r[2, 5] = bad
            code, text = code_and_text(e.subset_spanning_trees, r)
            assert code == ERR_ARG and word in text and "set 2" in text, (bad, code, text)
        with pytest.raises(ValueError):
            e.mass_segregation(1)
        with pytest.raises(ValueError):
            e.mass_segregation(513)
        # a position that is not finite: found by the bounds pass; in a subset, of a member only
        for bad in (float("nan"), float("inf")):
            p = pos.copy()
            p[517, 0] = bad
            upload(e, p)
            code, text = code_and_text(e.spanning_tree)
            assert code == ERR_ARG and "non-finite position" in text and "bounds pass" in text, (code, text)
            assert code_and_text(e.subset_spanning_trees, np.array([[1, 2, 3]]))[0] == 0
            code, text = code_and_text(e.subset_spanning_trees, np.array([[1, 517, 3]]))
            assert code == ERR_ARG and "non-finite position" in text, (code, text)
        upload(e, pos)
        assert code_and_text(e.spanning_tree)[0] == 0
        upload(e, pos[:0])                                         # no bodies
        t = e.spanning_tree(with_stats=True)
        assert t.n == 0 and len(t.lo) == 0 and t.stats == (0, 0, 0, 0) and t.groups_at(1.0).shape == (0,)
        assert code_and_text(e.subset_spanning_trees, np.array([[0, 1]]))[0] == ERR_ARG


def test_a_let_context_has_no_spanning_tree():
    pos = f32(np.random.default_rng(62).normal(size=(1000, 2)) * 0.05)
    with engine(1000, P.F32) as e:
        upload(e, pos)
        e.let_configure(0, 2, 1024)
        code, text = code_and_text(e.spanning_tree)
        assert code == ERR_STATE and "single GPU" in text, (code, text)
        assert code_and_text(e.subset_spanning_trees, np.array([[0, 1]]))[0] == ERR_STATE
    with engine(1000, P.F32) as e:                                 # the replicated scheme: world > 1
        upload(e, pos)
        e.set_owned_fraction(0, 2)
        assert code_and_text(e.spanning_tree)[0] == ERR_STATE


# ---- 9. non-perturbation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_spanning_trees_between_two_steps_change_nothing(precision, n_threads):
    cfg = dict(max_depth=21, reference_compat=False) if precision in (P.F32, P.MIXED) else {}
    rows = np.stack([np.random.default_rng(r).choice(Q.N, 33, replace=False) for r in range(9)])
    Q.check(precision, n_threads, lambda e: (e.spanning_tree(), e.subset_spanning_trees(rows), e.mass_segregation(6, 20)), **cfg)


# ---- 10. the CLI ----------------------------------------------------------------------------------------------------------------
def test_project_mst_and_segregation_files(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), mst_file="mst.csv", segregation_file="seg.csv",
                                         segregation_massive=8, segregation_random=30, segregation_seed=2, **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flags nothing changes
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and not (b / "mst.csv").exists() and not (b / "seg.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name

    def check(mst, seg, k, rnd, seed):
        lines = open(mst).read().splitlines()
        assert lines[0] == "# i,j,length"
        rows = [l.split(",") for l in lines[1:]]
        lo, hi, d2 = twin_tree(pa)
        assert [int(r[0]) for r in rows] == list(lo) and [int(r[1]) for r in rows] == list(hi)
        assert np.array_equal(np.array([float(r[2]) for r in rows]), np.sqrt(d2))
        lines = open(seg).read().splitlines()
        assert lines[0] == "# k,ratio,sigma,l_massive,l_random_mean" and len(lines) == 2
        ratio, sigma, l_massive, l_random, _ = M.mass_segregation(pa, m, k, rnd, seed)
        got = lines[1].split(",")
        assert int(got[0]) == k and [float(x) for x in got[1:]] == [ratio, sigma, l_massive, math.fsum(l_random.tolist()) / rnd]

    check(a / "mst.csv", a / "seg.csv", 8, 30, 2)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--mst-file", "main_mst.csv",
                             "--segregation-file", "main_seg.csv", "--segregation-massive", "5", "--segregation-random", "12"]) == 0
    finally:
        os.chdir(cwd)
    check(tmp_path / "main_mst.csv", tmp_path / "main_seg.csv", 5, 12, 0)
