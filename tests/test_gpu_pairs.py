"""bh_pair_counts on the device, held to the brute-force numpy twin tests/pairs_ref.py: every comparison is np.array_equal on
the int64 counts, computed from the state DOWNLOADED from the engine (in F32 that is the fp32 state as the device holds it).

  1. sizes around every edge: leaves and waves that are not full, a hierarchy of one node; auto and cross mode; 1 to 1,024
     bins; edges from 0, wholly beyond every distance, and one bin that holds every pair;
  2. all four precisions, Plummer with far outliers and uniform, right after upload and after 20 steps (the fp32 and mixed
     states have been physically re-ordered by then);
  3. ties: an integer lattice in a shuffled caller order with d2 on an inclusive edge, and 100 coincident bodies;
  4. degenerate boxes: a line, a point, two bodies 1e12 apart;
  5. points: far outside, on bodies, on the corners of the box, a call across the launch edge;
  6. identities at n = 16,384 without the twin: the sum, count_within at every edge, the bodies as their own points, and a
     cap on the distances computed;
  7. the run is not perturbed;
  8. the errors and trivial cases of include/bhgpu.h (but BH_ERR_CAPACITY: more than 2^24 bodies are too many for a test);
  9. project.py --pairs-file with and without --pairs-randoms;
 10. distributed.LetStepper.pair_counts on 1, 2 and 3 ranks."""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
import neighbours_ref as NR  # noqa: E402
import pairs_ref as R  # noqa: E402
import quiet_case as Q  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
P = G.Precision
ERR_ARG, ERR_STATE = -1, -5
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def upload(e, pos, mass=None):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    e.upload(pos, np.zeros_like(pos), np.full(len(pos), 1e-14) if mass is None else mass)


def raw_of(pc):
    return np.concatenate([[pc.below], pc.counts, [pc.beyond]]).astype(np.int64)


def same_as_twin(e, edges, points=None, what=""):
    """pair_counts(edges[, points]) of the engine's own state against the twin"""
    pos = e.download()[0]
    pc = e.pair_counts(edges, points, with_evals=True)
    want = R.pair_counts(pos, edges, points)
    got = raw_of(pc)
    nb = len(edges) - 1
    assert pc.counts.shape == (nb,) and pc.counts.dtype == np.int64 and pc.cumulative.shape == (nb + 1,)
    assert np.array_equal(got, want), f"{what}: bins {np.nonzero(got != want)[0][:6].tolist()} differ: got " \
                                      f"{got[got != want][:6].tolist()}, twin {want[got != want][:6].tolist()}"
    n = len(pos)
    q = None if points is None else len(np.asarray(points).reshape(-1, 2))
    assert pc.total == (n * (n - 1) // 2 if q is None else q * n) and pc.n_bodies == n and pc.n_points == q
    assert np.array_equal(pc.cumulative, np.cumsum(want[:-1])) and 0 <= pc.evals <= pc.total
    return pc


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------
EDGE_SETS = {"nb1": np.array([0.01, 0.1]), "nb2": np.array([0.005, 0.05, 0.2]), "nb33": G.radial_edges(1e-3, 0.5, 33),
             "nb1024": G.radial_edges(0.0, 0.4, 1024, "linear"), "from-zero": np.array([0.0, 0.02, 0.1]),
             "beyond-everything": np.array([1e3, 2e3, 4e3]), "one-bin-holds-all": np.array([0.0, 1e3])}


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_sizes_around_every_edge(precision, n):
    pos = f32(np.random.default_rng(n).normal(size=(n, 2)) * 0.05)
    if n >= 9:
        pos[5] = pos[2]                                           # a coincident pair: "below" even from edges[0] = 0
    pts = f32(np.random.default_rng(n + 1).normal(size=(67, 2)) * 0.08)
    with engine(n, precision) as e:
        upload(e, pos)
        for name, edges in EDGE_SETS.items():
            a = same_as_twin(e, edges, what=f"{precision.name} n={n} {name}")
            c = same_as_twin(e, edges, pts, what=f"{precision.name} n={n} {name} points")
            if name == "beyond-everything":
                assert a.below == a.total and c.below == c.total and a.evals == 0 and c.evals == 0   # whole nodes only
            if name == "one-bin-holds-all":
                assert a.counts[0] == a.total - (1 if n >= 9 else 0) and a.beyond == 0 and c.counts[0] == c.total


# ---- 2. precisions, before and after steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plummer", "uniform"])
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_all_precisions_after_upload_and_after_twenty_steps(precision, kind):
    n = 4096
    m, p, v = NR.plummer_with_outliers(n) if kind == "plummer" else NR.uniform(n)
    edges = G.radial_edges(1e-3, 0.25, 16)
    pts = f32(np.random.default_rng(61).uniform(-0.12, 0.12, size=(300, 2)))
    with engine(n, precision) as e:
        e.upload(p, v, m)
        same_as_twin(e, edges, what=f"{precision.name} {kind} after upload")
        same_as_twin(e, edges, pts, what=f"{precision.name} {kind} points after upload")
        e.step(20)
        same_as_twin(e, edges, what=f"{precision.name} {kind} after 20 steps")
        same_as_twin(e, edges, pts, what=f"{precision.name} {kind} points after 20 steps")
        same_as_twin(e, G.radial_edges(0.0, 0.3, 64, "linear"), what=f"{precision.name} {kind} linear")


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_lattice_ties_on_an_inclusive_edge(precision):
    pos = NR.lattice(32)
    edges = np.array([1.0, 2.0, 3.0, 5.0])
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(len(pos), 1)]
    with engine(len(pos), precision) as e:
        upload(e, pos)
        pc = same_as_twin(e, edges, what="lattice")
        assert (d2 == 25.0).sum() > 0 and pc.beyond == (d2 > 25.0).sum() and pc.counts[2] == ((d2 > 9.0) & (d2 <= 25.0)).sum()
        assert pc.below == (d2 <= 1.0).sum() == 2 * 32 * 31
        same_as_twin(e, edges, pos[::7], what="lattice, sites as points")
        same_as_twin(e, np.arange(0.0, 46.0), what="lattice, every integer edge")


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_a_hundred_coincident_bodies(precision):
    pos = np.tile(f32([[0.3, -0.7]]), (100, 1))
    with engine(100, precision) as e:
        upload(e, pos)
        for edges in ([0.0, 1.0], [0.5, 1.0, 2.0]):
            pc = same_as_twin(e, np.array(edges), what="coincident")
            assert pc.below == 4950 and pc.total == 4950 and not pc.counts.any()
    rng = np.random.default_rng(21)                                # and among others
    pos = f32(rng.normal(size=(1000, 2)) * 0.05)
    where = rng.permutation(1000)[:100]
    pos[where] = pos[where[0]]
    with engine(1000, precision) as e:
        upload(e, pos)
        assert same_as_twin(e, np.array([0.0, 0.01, 0.1]), what="coincident among others").below == 4950


# ---- 4. degenerate boxes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_degenerate_boxes(precision):
    rng = np.random.default_rng(31)
    line = np.stack([f32(rng.normal(size=300)), np.full(300, 0.25)], axis=1)         # the key box has no height
    point = np.tile([[0.5, -0.125]], (70, 1))                                         # nor width
    pair = np.array([[0.0, 0.0], [1e12, 1e12]])
    far = np.concatenate([[[0.0, 0.0]], f32(1e12 + rng.uniform(0.0, 4e6, size=(40, 2))), [[1e12, 1e12]]])
    pts = np.array([[0.0, 0.25], [0.5, -0.125], [1e12, 0.0], [-3.0, 7.0]])
    for name, pos in (("line", line), ("point", point), ("pair", pair), ("far", far)):
        with engine(len(pos), precision) as e:
            upload(e, pos)
            for edges in (np.array([0.0, 0.3, 5e6, 2e12]), G.radial_edges(1e-3, 3e12, 40)):
                same_as_twin(e, edges, what=name)
                same_as_twin(e, edges, pts, what=name + " points")


# ---- 5. points ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thousand():
    pos = f32(np.random.default_rng(41).normal(size=(1000, 2)) * 0.05)
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_points_outside_on_bodies_and_on_corners(precision):
    pos = thousand()
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    size = float((hi - lo).max())
    far = np.array([[1e6 * size, 0.0], [-1e6 * size, 1e6 * size], [0.0, -1e6 * size], [3e6 * size, 3e6 * size]])
    corners = np.array([[lo[0], lo[1]], [lo[0], hi[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], 0.0], [0.0, hi[1]]])
    inside = f32(np.random.default_rng(42).uniform(lo, hi, size=(200, 2)))
    with engine(1000, precision) as e:
        upload(e, pos)
        for edges in (G.radial_edges(1e-3, 0.3, 24), np.array([0.0, 0.01])):
            assert same_as_twin(e, edges, far, what="far points").beyond == 4000
            on = same_as_twin(e, edges, pos[::37], what="points on bodies")
            assert on.below >= len(pos[::37])                      # d2 = 0: nobody is left out
            same_as_twin(e, edges, corners, what="corners")
            same_as_twin(e, edges, np.concatenate([far, pos[::37], corners, inside]), what="all points")


def test_a_call_across_the_launch_edge():
    """2^20 + 3 points in one call: two launches that add into one histogram.  Against the twin on 65 bodies, and the sum of two
    calls that stay inside one launch each."""
    q = (1 << 20) + 3
    pts = np.random.default_rng(44).uniform(-0.2, 0.2, size=(q, 2))
    edges = G.radial_edges(0.01, 0.3, 9)
    with engine(65, P.F32) as e:
        upload(e, thousand()[:65])
        got = raw_of(same_as_twin(e, edges, pts, what="2^20 + 3 points"))
        parts = raw_of(e.pair_counts(edges, pts[:1 << 20])) + raw_of(e.pair_counts(edges, pts[1 << 20:]))
        assert np.array_equal(got, parts)


# ---- 6. identities ------------------------------------------------------------------------------------------------------------
def test_identities_at_sixteen_thousand_bodies():
    n = 16384
    pos = f32(np.random.default_rng(1).random((n, 2)))            # the unit square
    edges = G.radial_edges(0.01, 0.08, 8)
    with engine(n, P.F32) as e:
        upload(e, pos)
        auto = e.pair_counts(edges, with_evals=True)
        b_ms, q_ms = e.pair_counts_times()
        assert auto.total == n * (n - 1) // 2 == auto.below + int(auto.counts.sum()) + auto.beyond
        for k, edge in enumerate(edges):
            assert auto.cumulative[k] == int(e.count_within(float(edge)).sum(dtype=np.int64)) // 2, k
        own = e.pair_counts(edges, e.download()[0], with_evals=True)
        assert np.array_equal(own.counts, 2 * auto.counts) and own.below == 2 * auto.below + n and own.beyond == 2 * auto.beyond
        again = e.pair_counts(edges, with_evals=True)
    share = auto.evals / (n * (n - 1) / 2)
    print(f"evals {auto.evals} = {share:.4f} of n (n - 1) / 2 ({auto.evals / n:.1f} per body); points {own.evals}; "
          f"build {b_ms:.3f} ms, query {q_ms:.3f} ms")
    assert b_ms > 0.0 and q_ms > 0.0
    assert again.evals == auto.evals and np.array_equal(again.counts, auto.counts)      # deterministic
    assert auto.evals <= n * (n - 1) // 2 // 8, auto.evals         # not a brute force in disguise


# ---- 7. non-perturbation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_a_call_between_two_steps_changes_nothing(precision, n_threads):
    cfg = dict(max_depth=21, reference_compat=False) if precision in (P.F32, P.MIXED) else {}
    edges = G.radial_edges(1e-3, 0.1, 12)
    pts = np.random.default_rng(71).uniform(-0.05, 0.05, size=(100, 2))
    Q.check(precision, n_threads, lambda e: (e.pair_counts(edges), e.pair_counts(edges, pts)), **cfg)


# ---- 8. errors and trivial cases ----------------------------------------------------------------------------------------------
def code_and_text(f, *a, **kw):
    try:
        f(*a, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_errors_and_trivial_cases():
    pos = thousand()
    nan, inf = float("nan"), float("inf")
    good = np.array([0.01, 0.02, 0.05])
    with engine(1000, P.F64) as e:
        assert code_and_text(e.pair_counts, good)[0] == ERR_STATE   # before upload
        assert code_and_text(e.pair_counts, good, pos[:3])[0] == ERR_STATE
        upload(e, pos)
        assert code_and_text(e.pair_counts, good)[0] == 0
        for bad in ([0.01], [], [0.02, 0.01], [0.01, 0.01], [-0.01, 0.02], [0.01, nan], [0.01, inf], [nan, 0.02],
                    [0.0, 1e-200, 2e-200],                         # the squares are not strictly ascending
                    [1.0, 1e200],                                  # nor finite
                    list(np.linspace(0.1, 1.0, 1026))):            # 1,025 bins
            assert code_and_text(e.pair_counts, np.array(bad))[0] == ERR_ARG, bad
            assert code_and_text(e.pair_counts, np.array(bad), pos[:3])[0] == ERR_ARG, bad
        assert code_and_text(e.pair_counts, np.linspace(0.1, 1.0, 1025))[0] == 0
        for bad in (nan, inf, -inf):
            pts = pos[:5].copy()
            pts[3, 1] = bad
            code, text = code_and_text(e.pair_counts, good, pts)
            assert code == ERR_ARG and "point 3" in text, (code, text)
        # on the C-ABI itself: null arrays, n_points < 0, no points with n_points != n
        lib, h = e._lib, e._h
        ed = (C.c_double * 3)(*good)
        cnt, ev = (C.c_int64 * 4)(), C.c_int64()
        pts = (C.c_double * 8)(*pos[:4].reshape(-1))
        assert lib.bh_pair_counts(h, None, 1000, ed, 2, cnt, None) == 0 and sum(cnt) == 1000 * 999 // 2
        assert lib.bh_pair_counts(h, None, 1000, ed, 2, cnt, C.byref(ev)) == 0 and ev.value >= 0
        assert lib.bh_pair_counts(h, None, 1000, ed, 2, None, None) == ERR_ARG
        assert lib.bh_pair_counts(h, None, 1000, None, 2, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(h, None, 999, ed, 2, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(h, None, 0, ed, 2, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(h, pts, -1, ed, 2, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(h, pts, 4, ed, 0, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(None, pts, 4, ed, 2, cnt, None) == ERR_ARG
        assert lib.bh_pair_counts(h, pts, 4, ed, 2, cnt, None) == 0 and sum(cnt) == 4000
        assert lib.bh_pair_counts(h, pts, 0, ed, 2, cnt, C.byref(ev)) == 0 and sum(cnt) == 0 and ev.value == 0   # trivial
        assert lib.bh_pair_counts_times(h, None, None) == ERR_ARG
        # a body that is not finite: found by the bounds pass
        for bad in (nan, inf):
            p = pos.copy()
            p[517, 0] = bad
            upload(e, p)
            for a in ((good,), (good, pos[:3])):
                code, text = code_and_text(e.pair_counts, *a)
                assert code == ERR_ARG and "non-finite position" in text and "bounds pass" in text, (code, text)
        upload(e, pos)
        assert code_and_text(e.pair_counts, good)[0] == 0
        # one body: no pair; no bodies: nothing at all
        upload(e, pos[:1])
        one = e.pair_counts(good, with_evals=True)
        assert one.total == 0 and not one.counts.any() and one.evals == 0 and one.n_bodies == 1
        assert e.pair_counts(good, pos[:6]).total == 6
        upload(e, pos[:0])
        for pc in (e.pair_counts(good), e.pair_counts(good, pos[:6]), e.pair_counts(good, pos[:0])):
            assert pc.total == 0 and pc.below == 0 and pc.beyond == 0 and not pc.counts.any() and not pc.cumulative.any()


def test_a_let_context_counts_its_own_bodies():
    pos = thousand()
    edges = G.radial_edges(1e-3, 0.3, 10)
    with engine(1000, P.F32) as e:
        upload(e, pos)
        e.let_configure(0, 2, 1024)
        same_as_twin(e, edges, what="LET mode")
        same_as_twin(e, edges, pos[:50] + 0.001, what="LET mode points")
    with engine(1000, P.F32) as e:                                 # the replicated scheme: world > 1
        upload(e, pos)
        e.set_owned_fraction(0, 2)
        same_as_twin(e, edges, what="world 2")


def test_correlation_of_a_clustered_state():
    n = 4096
    m, p, v = NR.plummer_with_outliers(n)
    edges = G.radial_edges(2e-3, 0.05, 6)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        pos = e.download()[0]
        rnd = project.pairs_random_points(pos[:n - 8], 2000, 5)     # the box of the sphere, not of the outliers
        xi, dd, dr = e.correlation(edges, rnd)
    assert np.array_equal(raw_of(dd), R.pair_counts(pos, edges)) and np.array_equal(raw_of(dr), R.pair_counts(pos, edges, rnd))
    assert np.array_equal(xi, G.correlation_from(dd.counts, dr.counts, n, 2000), equal_nan=True)
    assert xi[0] > xi[-1] and xi[0] > 1.0                          # clustered: most at small separations


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------
def read_rows(path):
    lines = open(path).read().splitlines()
    return lines[0], np.array([[float(t) for t in l.split(",")] for l in lines[1:]])


def test_project_pairs_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    size = float(np.ptp(np.asarray(p).reshape(-1, 2), axis=0).max())
    rng = (0.01 * size, 0.5 * size)
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), pairs_file="dd.csv", pairs_bins=7, pairs_range=rng, **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flag nothing changes
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and not (b / "dd.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    head, rows = read_rows(a / "dd.csv")
    edges = G.radial_edges(*rng, 7)
    assert head == "# r_lo,r_hi,dd" and rows.shape == (7, 3)
    assert np.array_equal(rows[:, 0], edges[:-1]) and np.array_equal(rows[:, 1], edges[1:])
    assert np.array_equal(rows[:, 2].astype(np.int64), R.pair_counts(pa, edges)[1:-1]) and rows[:, 2].sum() > 0
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        base = ["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--pairs-bins", "5", "--pairs-range", repr(rng[0]),
                repr(rng[1])]
        assert project.main(base + ["--pairs-file", "lin.csv", "--pairs-spacing", "linear"]) == 0
        assert project.main(base + ["--pairs-file", "xi.csv", "--pairs-randoms", "3000", "--pairs-seed", "9"]) == 0
        for bad in (["--pairs-bins", "5"], ["--pairs-file", "x.csv", "--pairs-bins", "5"], ["--pairs-file", "x.csv", "--pairs-range", "1", "2"],
                    ["--pairs-file", "x.csv", "--pairs-bins", "5", "--pairs-range", "0", "2"],
                    ["--pairs-file", "x.csv", "--pairs-bins", "5", "--pairs-range", "1", "2", "--pairs-seed", "3"],
                    ["--pairs-file", "x.csv", "--pairs-bins", "1025", "--pairs-range", "1", "2"]):
            with pytest.raises(SystemExit):
                project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files"] + bad)
    finally:
        os.chdir(cwd)
    head, rows = read_rows(tmp_path / "lin.csv")
    edges = G.radial_edges(*rng, 5, "linear")
    assert head == "# r_lo,r_hi,dd" and np.array_equal(rows[:, 2].astype(np.int64), R.pair_counts(pa, edges)[1:-1])
    head, rows = read_rows(tmp_path / "xi.csv")
    edges = G.radial_edges(*rng, 5)
    rnd = project.pairs_random_points(pa, 3000, 9)
    lo, hi = pa.min(axis=0), pa.max(axis=0)
    assert np.array_equal(rnd, lo + (hi - lo) * np.random.default_rng(9).random((3000, 2)))
    assert head == "# r_lo,r_hi,dd,dr,xi" and rows.shape == (5, 5)
    assert np.array_equal(rows[:, 2].astype(np.int64), R.pair_counts(pa, edges)[1:-1])
    assert np.array_equal(rows[:, 3].astype(np.int64), R.pair_counts(pa, edges, rnd)[1:-1])
    assert np.array_equal(rows[:, 4], G.correlation_from(rows[:, 2], rows[:, 3], 1024, 3000), equal_nan=True)


# ---- 10. distributed --------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2, 3])
def test_let_stepper_pair_counts(tmp_path, world):
    """World processes over gloo on the one GPU (with this one: at most four with the device open), each with its own timeout.
    After two steps and a rebalance() every rank's counts are the twin's of the gathered bodies."""
    port = _free_port()
    script = os.path.join(HERE, "pairs_ranks.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), str(tmp_path)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{o[-3000:]}"
    import pairs_ranks as PR
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([x["ids"] for x in ranks])
    assert sorted(ids.tolist()) == list(range(PR.N))
    if world > 1:
        assert all(len(x["ids"]) > 0 for x in ranks)
    assert all(int(x["raised"]) == (2 if world > 1 else 0) for x in ranks)    # (one rank cannot disagree with itself)
    pos = np.concatenate([x["pos"] for x in ranks])
    edges = PR.edges_of(PR.bodies()[0])
    want = R.pair_counts(pos, edges)
    assert want[1:-1].all() and want.sum() == PR.N * (PR.N - 1) // 2
    for r, x in enumerate(ranks):
        assert np.array_equal(x["raw"], want), r
        assert int(x["total"]) == want.sum() and int(x["n_bodies"]) == PR.N and bool(x["same"])
        assert np.array_equal(x["cumulative"], np.cumsum(want[:-1]))
