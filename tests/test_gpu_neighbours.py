"""bh_neighbours and bh_count_within on the device, held to the brute-force numpy twin tests/neighbours_ref.py: every
comparison is np.array_equal on the caller indices, the d2 and the counts, computed from the state DOWNLOADED from the engine
(in F32 that is the fp32 state as the device holds it).

  1. sizes around every edge: padding with -1 / +inf, leaves and waves that are not full, a hierarchy of one node;
  2. all four precisions, Plummer with far outliers and uniform, right after upload and after 20 steps (the fp32 and mixed
     states have been physically re-ordered by then: idx must still be caller indices), F32 also without re-ordering;
  3. ties: an integer lattice in a shuffled caller order, and more coincident bodies than a leaf holds;
  4. degenerate boxes: a line, a point, two bodies 1e12 apart;
  5. points: far outside, on bodies, on the corners of the box, subsets in another order, a call across the launch edge;
  6. count_within: radius 0, inclusive at equality, just below, everything, three radii in all precisions;
  7. the run is not perturbed, and the buffers are allocated once;
  8. the errors of include/bhgpu.h (but BH_ERR_CAPACITY: more than 2^24 bodies are too many for a test);
  9. local_density, density_centre and project.py --neighbours-file;
 10. the algorithmic cost: evaluations per body at N = 65,536."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
import neighbours_ref as R  # noqa: E402
import quiet_case as Q  # noqa: E402

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


def same_as_twin(e, k, points=None, rows=None, what=""):
    """neighbours(k[, points]) of the engine's own state against the twin (on `rows` of the queries only, if given)"""
    pos = e.download()[0]
    idx, d2 = e.neighbours(k, points)
    q = len(pos) if points is None else len(np.asarray(points).reshape(-1, 2))
    assert idx.shape == (q, k) and idx.dtype == np.int64 and d2.shape == (q, k) and d2.dtype == np.float64
    want_idx, want_d2 = R.neighbours(pos, k, points, rows)
    if rows is not None:
        idx, d2 = idx[rows], d2[rows]
    bad = np.argwhere((idx != want_idx) | (d2 != want_d2))
    assert len(bad) == 0, f"{what} k={k}: {len(bad)} entries differ; first (row, entry) = {bad[0].tolist()}: got " \
                          f"({idx[tuple(bad[0])]}, {d2[tuple(bad[0])]!r}), twin ({want_idx[tuple(bad[0])]}, {want_d2[tuple(bad[0])]!r})"
    return idx, d2


def counts_as_twin(e, radius, points=None, what=""):
    got = e.count_within(radius, points)
    want = R.count_within(e.download()[0], radius, points)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (what, radius, np.argwhere(got != want)[:4].tolist())
    return got


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_sizes_around_every_edge(precision, n):
    pos = f32(np.random.default_rng(n).normal(size=(n, 2)) * 0.05)
    pts = f32(np.random.default_rng(n + 1).normal(size=(67, 2)) * 0.08)
    with engine(n, precision) as e:
        upload(e, pos)
        for k in (1, 8, 32):
            idx, d2 = same_as_twin(e, k, what=f"{precision.name} n={n}")
            if n:
                assert (idx[:, min(k, n - 1):] == -1).all() and np.isinf(d2[:, min(k, n - 1):]).all()
                assert (idx[:, :min(k, n - 1)] >= 0).all()
            idx, d2 = same_as_twin(e, k, pts, what=f"{precision.name} n={n} points")
            assert (idx[:, min(k, n):] == -1).all() and (idx[:, :min(k, n)] >= 0).all()
        for radius in (0.0, 0.02, 0.1, 10.0):
            counts_as_twin(e, radius)
            counts_as_twin(e, radius, pts)


# ---- 2. precisions, before and after steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plummer", "uniform"])
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_all_precisions_after_upload_and_after_twenty_steps(precision, kind):
    n = 4096
    m, p, v = R.plummer_with_outliers(n) if kind == "plummer" else R.uniform(n)
    with engine(n, precision) as e:
        e.upload(p, v, m)
        for k in (1, 6, 32):
            same_as_twin(e, k, what=f"{precision.name} {kind} after upload")
        e.step(20)
        for k in (1, 6, 32):
            same_as_twin(e, k, what=f"{precision.name} {kind} after 20 steps")
        counts_as_twin(e, 0.004)


def test_fp32_without_reordering(monkeypatch):
    monkeypatch.setenv("BH_REORDER_EVERY", "0")
    n = 4096
    m, p, v = R.plummer_with_outliers(n)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        e.step(20)
        for k in (1, 6, 32):
            same_as_twin(e, k, what="F32 BH_REORDER_EVERY=0")


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_lattice_ties_fall_to_the_smaller_caller_index(precision):
    pos = R.lattice(32)
    with engine(len(pos), precision) as e:
        upload(e, pos)
        idx, d2 = same_as_twin(e, 8, what="lattice")
        i = int(np.nonzero((pos == [16.0, 16.0]).all(axis=1))[0][0])
        assert list(d2[i]) == [1.0] * 4 + [2.0] * 4
        assert list(idx[i, :4]) == sorted(idx[i, :4]) and list(idx[i, 4:]) == sorted(idx[i, 4:])
        corner = int(np.nonzero((pos == [0.0, 0.0]).all(axis=1))[0][0])
        assert list(d2[corner]) == [1.0, 1.0, 2.0, 4.0, 4.0, 5.0, 5.0, 8.0]
        same_as_twin(e, 32, what="lattice")


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_more_coincident_bodies_than_a_leaf_holds(precision):
    rng = np.random.default_rng(21)
    pos = f32(rng.normal(size=(1000, 2)) * 0.05)
    where = rng.permutation(1000)[:100]
    pos[where] = pos[where[0]]
    with engine(1000, precision) as e:
        upload(e, pos)
        idx, d2 = same_as_twin(e, 32, what="coincident")
        assert (d2[where] == 0.0).all()                            # 99 others at d2 = 0: the 32 smallest caller indices
        first = np.sort(where)
        for i in where[:5]:
            assert list(idx[i]) == [j for j in first if j != i][:32]
        assert counts_as_twin(e, 0.0)[where].tolist() == [99] * 100


# ---- 4. degenerate boxes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_degenerate_boxes(precision):
    rng = np.random.default_rng(31)
    line = np.stack([f32(rng.normal(size=300)), np.full(300, 0.25)], axis=1)         # the key box has no height
    point = np.tile([[0.5, -0.125]], (70, 1))                                         # nor width
    pair = np.concatenate([[[0.0, 0.0]], f32(1e12 + rng.uniform(0.0, 4e6, size=(40, 2))), [[1e12, 1e12]]])
    pts = np.array([[0.0, 0.25], [0.5, -0.125], [1e12, 0.0], [-3.0, 7.0]])
    for name, pos in (("line", line), ("point", point), ("pair", pair)):
        with engine(len(pos), precision) as e:
            upload(e, pos)
            for k in (1, 8, 32):
                same_as_twin(e, k, what=name)
                same_as_twin(e, k, pts, what=name + " points")
            for radius in (0.0, 0.3, 5e6, 2e12):
                counts_as_twin(e, radius, what=name)
                counts_as_twin(e, radius, pts, what=name)


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
    pts = np.concatenate([far, pos[::37], corners, inside])
    with engine(1000, precision) as e:
        upload(e, pos)
        for k in (1, 8, 32):
            idx, d2 = same_as_twin(e, k, pts, what="points")
            on = slice(len(far), len(far) + len(pos[::37]))
            assert (d2[on, 0] == 0.0).all() and list(idx[on, 0]) == list(range(0, 1000, 37))     # nobody is left out
        # a query's rows do not depend on the other queries, their order or their number
        full_idx, full_d2 = e.neighbours(8, pts)
        sub = np.random.default_rng(43).permutation(len(pts))[:50]
        idx, d2 = e.neighbours(8, pts[sub])
        assert np.array_equal(idx, full_idx[sub]) and np.array_equal(d2, full_d2[sub])
        idx, d2 = e.neighbours(8, pts[7:8])
        assert np.array_equal(idx, full_idx[7:8]) and np.array_equal(d2, full_d2[7:8])
        assert np.array_equal(e.count_within(0.03, pts[sub]), e.count_within(0.03, pts)[sub])
        counts_as_twin(e, 0.03, pts)


def test_a_call_across_the_launch_edge():
    """2^20 + 3 points in one call: two launches.  The twin runs on a strided sample of 4,096 rows and on the three rows past
    the edge."""
    pos = thousand()
    q = (1 << 20) + 3
    rng = np.random.default_rng(44)
    pts = rng.uniform(-0.2, 0.2, size=(q, 2))
    rows = np.concatenate([np.arange(0, 1 << 20, 256), [1 << 20, (1 << 20) + 1, (1 << 20) + 2]])
    with engine(1000, P.F32) as e:
        upload(e, pos)
        same_as_twin(e, 2, pts, rows, what="2^20 + 3 points")
        got = e.count_within(0.01, pts)
        assert np.array_equal(got[rows], R.count_within(e.download()[0], 0.01, pts, rows))


# ---- 6. count_within ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_count_bounds_are_inclusive(precision):
    pos = R.lattice(32)
    n = len(pos)
    i = int(np.nonzero((pos == [16.0, 16.0]).all(axis=1))[0][0])
    below = float(np.nextafter(5.0, 0.0))
    assert 5.0 * 5.0 == 25.0 and below * below < 25.0
    with engine(n, precision) as e:
        upload(e, pos)
        at, under = counts_as_twin(e, 5.0), counts_as_twin(e, below)
        # d2 <= 25 around an inner site: 81 sites, itself left out; 12 of them have d2 = 25 exactly
        assert at[i] == 80 and under[i] == 68
        pts = np.array([[16.0, 16.0], [15.5, 16.0], [-5.0, 0.0]])
        assert counts_as_twin(e, 5.0, pts).tolist()[0] == 81
        counts_as_twin(e, below, pts)
        assert (counts_as_twin(e, 0.0) == 0).all() and counts_as_twin(e, 0.0, pts).tolist() == [1, 0, 0]
        # everything: n - 1 for a body, n for a point -- whole nodes taken without opening them
        assert (counts_as_twin(e, 1e9) == n - 1).all() and (counts_as_twin(e, 1e9, pts) == n).all()
        # most of the system: whole nodes inside, opened nodes at the rim
        for radius in (12.0, 20.5, 31.0):
            counts_as_twin(e, radius)
            counts_as_twin(e, radius, pts)


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_counts_on_plummer_at_three_radii(precision):
    n = 4096
    m, p, v = R.plummer_with_outliers(n)
    with engine(n, precision) as e:
        e.upload(p, v, m)
        for radius in (0.0005, 0.01, 0.2):
            got = counts_as_twin(e, radius)
        assert got.max() >= n - 10 and got.min() == 0               # 0.2 holds the whole sphere; an outlier holds nobody


# ---- 7. non-perturbation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_a_query_between_two_steps_changes_nothing(precision, n_threads):
    cfg = dict(max_depth=21, reference_compat=False) if precision in (P.F32, P.MIXED) else {}
    Q.check(precision, n_threads, lambda e: (e.neighbours(8), e.count_within(0.1)), **cfg)


def test_the_buffers_are_allocated_on_first_use_and_kept():
    pos = thousand()
    with engine(1000, P.F32) as e:
        upload(e, pos)
        b0 = e.stats().device_bytes
        e.neighbours(8)
        b1 = e.stats().device_bytes
        e.neighbours(8)
        e.count_within(0.1)
        e.neighbours(4, pos[:10])
        assert b1 > b0 and e.stats().device_bytes == b1
        e.neighbours(32)                                           # a longer list grows the launch block, once
        b2 = e.stats().device_bytes
        e.neighbours(32)
        assert b2 > b1 and e.stats().device_bytes == b2


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------
def code_and_text(f, *a, **kw):
    try:
        f(*a, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_errors():
    pos = thousand()
    nan, inf = float("nan"), float("inf")
    with engine(1000, P.F64) as e:
        assert code_and_text(e.neighbours, 4)[0] == ERR_STATE       # before upload
        assert code_and_text(e.count_within, 0.1)[0] == ERR_STATE
        upload(e, pos)
        assert code_and_text(e.neighbours, 4)[0] == 0
        for k in (0, -1, 33, 1 << 20):
            assert code_and_text(e.neighbours, k)[0] == ERR_ARG, k
            assert code_and_text(e.neighbours, k, pos[:3])[0] == ERR_ARG, k
        assert code_and_text(e.neighbours, 32)[0] == 0 and code_and_text(e.neighbours, 1)[0] == 0
        for bad in (nan, inf, -inf):
            pts = pos[:5].copy()
            pts[3, 1] = bad
            code, text = code_and_text(e.neighbours, 4, pts)
            assert code == ERR_ARG and "point 3" in text, (code, text)
            assert code_and_text(e.count_within, 0.1, pts)[0] == ERR_ARG
        for radius in (-1.0, -1e-300, nan, inf, -inf):
            assert code_and_text(e.count_within, radius)[0] == ERR_ARG, radius
            assert code_and_text(e.count_within, radius, pos[:3])[0] == ERR_ARG, radius
        assert code_and_text(e.count_within, 0.0)[0] == 0 and code_and_text(e.count_within, 1e200)[0] == 0
        # on the C-ABI itself: null outputs, n_points < 0, no points with n_points != n
        lib, h = e._lib, e._h
        idx, d2 = (C.c_int64 * 4000)(), (C.c_double * 4000)()
        cnt = (C.c_uint32 * 1000)()
        pts = (C.c_double * 8)(*pos[:4].reshape(-1))
        assert lib.bh_neighbours(h, None, 1000, 4, None, None, cnt) == ERR_ARG
        assert lib.bh_neighbours(h, None, 1000, 4, idx, None, None) == 0
        assert lib.bh_neighbours(h, None, 1000, 4, None, d2, None) == 0
        assert lib.bh_neighbours(h, None, 999, 4, idx, d2, None) == ERR_ARG
        assert lib.bh_neighbours(h, None, 0, 4, idx, d2, None) == ERR_ARG
        assert lib.bh_neighbours(h, pts, -1, 4, idx, d2, None) == ERR_ARG
        assert lib.bh_neighbours(h, pts, 0, 4, idx, d2, None) == 0                  # valid and trivial
        assert lib.bh_neighbours(None, pts, 4, 4, idx, d2, None) == ERR_ARG
        assert lib.bh_count_within(h, None, 1000, 0.1, None) == ERR_ARG
        assert lib.bh_count_within(h, None, 1001, 0.1, cnt) == ERR_ARG
        assert lib.bh_count_within(h, pts, -2, 0.1, cnt) == ERR_ARG
        assert lib.bh_count_within(h, pts, 0, 0.1, cnt) == 0
        assert lib.bh_count_within(h, pts, 4, 0.1, cnt) == 0
        assert lib.bh_neighbours_times(h, None, None) == ERR_ARG
        b, q = e.neighbours_times()
        assert b > 0.0 and q > 0.0
        # a body that is not finite: found by the bounds pass
        for bad in (nan, inf):
            p = pos.copy()
            p[517, 0] = bad
            upload(e, p)
            for f, a in ((e.neighbours, (4,)), (e.neighbours, (4, pos[:3])), (e.count_within, (0.1,))):
                code, text = code_and_text(f, *a)
                assert code == ERR_ARG and "non-finite position" in text and "bounds pass" in text, (code, text)
        upload(e, pos)
        assert code_and_text(e.neighbours, 4)[0] == 0
        # no bodies: nobody is near
        upload(e, pos[:0])
        idx, d2, ev = e.neighbours(3, pos[:6], with_evals=True)
        assert (idx == -1).all() and np.isinf(d2).all() and idx.shape == (6, 3) and not ev.any()
        assert e.neighbours(3)[0].shape == (0, 3) and not e.count_within(1.0, pos[:6]).any()


def test_a_let_context_has_no_neighbours():
    pos = thousand()
    with engine(1000, P.F32) as e:
        upload(e, pos)
        e.let_configure(0, 2, 1024)
        for f, a in ((e.neighbours, (4,)), (e.neighbours, (4, pos[:3])), (e.count_within, (0.1,))):
            code, text = code_and_text(f, *a)
            assert code == ERR_STATE and "single GPU" in text, (code, text)
    with engine(1000, P.F32) as e:                                 # the replicated scheme: world > 1
        upload(e, pos)
        e.set_owned_fraction(0, 2)
        assert code_and_text(e.neighbours, 4)[0] == ERR_STATE


# ---- 9. derived quantities and the CLI ----------------------------------------------------------------------------------------
def test_local_density_and_density_centre():
    n = 4096
    m, p, v = R.plummer_with_outliers(n)
    m = f32(m * np.random.default_rng(51).uniform(0.5, 2.0, size=n))
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        pos, mass = e.download()[0], e.masses()
        for k in (2, 6):
            sigma, r_k = e.local_density(k)
            idx, d2 = R.neighbours(pos, k)
            want_s, want_r = R.local_density(idx, d2, mass)
            assert np.array_equal(sigma, want_s, equal_nan=True) and np.array_equal(r_k, want_r)
        assert np.isfinite(sigma).all() and sigma.max() / sigma.min() > 1e6      # the core against an outlier
        centre = e.density_centre(6)
        assert np.array_equal(centre, R.density_centre(want_s, pos))
        assert np.hypot(*centre) < 0.005                           # in the core, although the outliers pull the centre of mass away
        with pytest.raises(ValueError):
            e.local_density(1)
    with engine(4, P.F64) as e:                                    # fewer than k neighbours: NaN, no centre
        upload(e, p[:4])
        sigma, r_k = e.local_density(6)
        assert np.isnan(sigma).all() and np.isinf(r_k).all() and np.isnan(e.density_centre(6)).all()


def read_rows(path):
    lines = open(path).read().splitlines()
    return lines[0], [l.split(",") for l in lines[1:]]


def test_project_neighbours_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), neighbours_file="nb.csv", **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flag nothing changes
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and not (b / "nb.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name

    def check(path, pos, k):
        head, rows = read_rows(path)
        assert head == "# i,x,y,r_k,sigma" and len(rows) == 1024
        assert [int(r[0]) for r in rows] == list(range(1024))
        got = np.array([[float(t) for t in r[1:]] for r in rows])
        want_s, want_r = R.local_density(*R.neighbours(pos, k), m)
        assert np.array_equal(got[:, :2], pos) and np.array_equal(got[:, 2], want_r) and np.array_equal(got[:, 3], want_s)

    check(a / "nb.csv", pa, 6)
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--neighbours-file", "main.csv",
                             "--neighbours-k", "3"]) == 0
    finally:
        os.chdir(cwd)
    check(tmp_path / "main.csv", pa, 3)


# ---- 10. algorithmic cost -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "plummer"])
def test_evaluations_per_body_stay_small(kind):
    """N = 65,536, F32, k = 8, every body: mean evals <= 512 and maximum <= 4,096 (a seeded, pruning search measures a mean
    of about a hundred; one that does not seed or does not prune thousands).  Correctness on a strided sample of 2,048."""
    n = 65536
    m, p, v = R.uniform(n) if kind == "uniform" else R.plummer_with_outliers(n)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        idx, d2, ev = e.neighbours(8, with_evals=True)
        pos = e.download()[0]
        b_ms, q_ms = e.neighbours_times()
        again = e.neighbours(8, with_evals=True)[2]
    print(f"{kind}: evals mean {ev.mean():.1f} max {ev.max()} min {ev.min()}; build {b_ms:.3f} ms, query {q_ms:.3f} ms")
    assert ev.dtype == np.uint32 and np.array_equal(ev, again)      # deterministic
    rows = np.arange(0, n, 32)
    want_idx, want_d2 = R.neighbours(pos, 8, rows=rows)
    assert np.array_equal(idx[rows], want_idx) and np.array_equal(d2[rows], want_d2)
    assert ev.min() >= 8
    assert ev.mean() <= 512.0, ev.mean()
    assert ev.max() <= 4096, ev.max()
