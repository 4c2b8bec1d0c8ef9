"""The Barnes-Hut field at arbitrary points on the device (bh_field_at, BarnesHutEngine.field):

  1. fp64 precisions against the pinned oracle walking appended points (tests/field_ref.py): term counts, and
     acceleration and potential within the forward bound (count + 16) * 2^-52 * sum |term|;
  2. F32 / MIXED by class (tests/parity_classes.py) against the oracle's diagnostic walk of the same points;
  3. fp32 self-consistency: the field at the bodies' own positions takes the force walk's terms;
  4. a point's result does not depend on the rest of the call, bit for bit;
  5. a call does not perturb the run;
  6. edges and errors;  7. the project.py field file."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import _lib, initial_conditions as IC, project  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_PORTABLE, FLAG_WALK_STATS  # noqa: E402
import field_ref as FR  # noqa: E402
import parity_classes as PC  # noqa: E402
import quiet_case as QC  # noqa: E402

P = G.Precision
ALL = [P.F64_EXACT, P.F64, P.MIXED, P.F32]
ERR_ARG, ERR_STATE = -1, -5
MARGIN = 1e-12          # BH_PRECISION_F64 forms its own d2 thresholds: a decision closer than this to theta may turn
K_POINTS = 3000
# Seeds of the point sets of test 1 (field_ref.points_around(pos, K_POINTS, seed)).  With these, tests/field_ref.py alone finds NO
# point whose smallest |size/d - theta| / theta is below MARGIN on any of the four inputs at theta 0.5 and 0.2 and max_depth 10
# and 21: the smallest margins met are 1.1e-7 (init1024), 1.3e-6 (random4096), 1.6e-7 (clumped8192) and 1.2e-7 (golden40960),
# so BH_PRECISION_F64 is held to equal counts on every point here.
POINT_SEED = {"init1024": 3, "random4096": 4, "clumped8192": 5, "golden40960": 6}


def engine(n, **kw):
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), **kw))


def fp64_input(name, init1024, gold):
    if name == "init1024":
        m, p, _ = init1024
        return p, m
    if name == "random4096":
        m, p, _ = IC.make("uniform", 4096, 11)
        return p, m
    if name == "clumped8192":
        return FR.clumped(8192, 7)
    g = gold("ref_project_40960")
    return g["pos"], g["mass"]


# ---- 1. fp64 precisions against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("max_depth", [10, 21])
@pytest.mark.parametrize("theta", [0.5, 0.2])
@pytest.mark.parametrize("name", list(POINT_SEED))
def test_fp64_field_against_the_oracle(init1024, gold, name, theta, max_depth, compat):
    p, m = fp64_input(name, init1024, gold)
    n = len(m)
    pts = FR.points_around(p, K_POINTS, POINT_SEED[name])
    lo, hi = p.min(axis=0), p.max(axis=0)
    outside = ((pts < lo) | (pts > hi)).any(axis=1)
    assert outside.sum() > K_POINTS // 5 and (~outside).sum() > K_POINTS // 5 and (pts[:, 0] == lo[0]).any()
    nodes = O.build_tree(p, m, max_depth)
    d = FR.oracle_at_points(nodes, p, m, pts, theta=theta, compat=compat)
    r = FR.field_walk(nodes, pts, theta=theta)
    assert np.array_equal(r.counts, d.counts.astype(np.int64))
    close = r.margin < MARGIN
    assert close.sum() <= 1e-3 * len(pts), (int(close.sum()), float(r.margin.min()))
    ba, bp = FR.accel_bound(d.counts, r.abs_sum), FR.accel_bound(d.counts, r.pot_sum)
    for label, prec, flags in [("exact", P.F64_EXACT, 0), ("portable", P.F64_EXACT, FLAG_WALK_PORTABLE), ("f64", P.F64, 0)]:
        with engine(n, precision=prec, theta=theta, max_depth=max_depth, reference_compat=compat, flags=flags) as e:
            e.upload(p, np.zeros_like(p), m)
            acc, phi, cnt = e.field(pts, with_counts=True)
        sel = ~close if prec == P.F64 else np.ones(len(pts), dtype=bool)
        bad = np.flatnonzero(cnt[sel] != d.counts[sel])
        print(label, "count mismatches", len(bad), "min margin %.3e" % r.margin.min())
        assert len(bad) == 0, (label, bad[:8], cnt[sel][bad[:8]], d.counts[sel][bad[:8]])
        eq = cnt == d.counts                                      # (a point with other terms has another sum)
        ea = np.linalg.norm(acc - d.forces, axis=1)
        ep = np.abs(phi - r.phi)
        print(label, "max err / bound: accel %.3f phi %.3f" % ((ea / ba)[eq].max(), (ep / bp)[eq].max()))
        assert (ea[eq] <= ba[eq]).all(), (label, float((ea / ba)[eq].max()))
        assert (ep[eq] <= bp[eq]).all(), (label, float((ep / bp)[eq].max()))
        assert np.isfinite(acc).all() and np.isfinite(phi).all()


def test_fp64_field_of_the_deep_chain_uses_the_second_stack_tier():
    """field_ref.deep_chain at theta 0.2: the point next to the origin holds 85 quads pending (tests/test_field_cpu.py), so
    its wavefront pushes past entry 64 of the lane stack.  That point and the eight corner and edge points of the bounding
    box, checked as above; the two corners that are the anchor bodies' own places get the non-finite acceleration the
    oracle gets there (inf * 0), so the acceleration bound is held on the other seven points and the potential bound on all."""
    p, m = FR.deep_chain()
    pts = np.concatenate([FR.DEEP_POINT, FR.points_around(p, 24, 0)[16:24]])     # (of 24 points, 16..23 are the corners and edges)
    nodes = O.build_tree(p, m, FR.DEEP_DEPTH)
    d = FR.oracle_at_points(nodes, p, m, pts, theta=FR.DEEP_THETA, compat=False)
    r = FR.field_walk(nodes, pts, theta=FR.DEEP_THETA)
    assert np.array_equal(r.counts, d.counts.astype(np.int64)) and d.counts[0] == 172
    assert r.margin.min() >= MARGIN                               # (no decision BH_PRECISION_F64 could turn: 1.5e-2 at the least)
    fin = np.isfinite(d.forces).all(axis=1)
    assert fin.sum() == 7 and fin[0]
    ba, bp = FR.accel_bound(d.counts, r.abs_sum), FR.accel_bound(d.counts, r.pot_sum)
    for label, prec, flags in [("exact", P.F64_EXACT, 0), ("portable", P.F64_EXACT, FLAG_WALK_PORTABLE), ("f64", P.F64, 0)]:
        with engine(len(m), precision=prec, theta=FR.DEEP_THETA, max_depth=FR.DEEP_DEPTH, reference_compat=False, flags=flags) as e:
            e.upload(p, np.zeros_like(p), m)
            acc, phi, cnt = e.field(pts, with_counts=True)
        assert np.array_equal(cnt, d.counts), (label, cnt, d.counts)
        ea = np.linalg.norm(acc - d.forces, axis=1)
        ep = np.abs(phi - r.phi)
        print(label, "max err / bound: accel %.3f phi %.3f" % ((ea / ba)[fin].max(), (ep / bp).max()))
        assert (ea[fin] <= ba[fin]).all(), (label, float((ea / ba)[fin].max()))
        assert (ep <= bp).all(), (label, float((ep / bp).max()))
        assert np.array_equal(np.isfinite(acc).all(axis=1), fin) and np.isfinite(phi).all()


# ---- 2. F32 and MIXED by class ---------------------------------------------------------------------------------------
def class_terms(d, k):
    """(err model, flip budget) per point as parity_classes.classify forms them, unit masses."""
    model = 2.0 ** -24 * ((1.5 * np.sqrt(d.counts[:k]) + 8.0) * d.abs_sum[:k] + 4.0 * d.coord[:k])
    return model, d.flip[:k]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("theta", [0.5, 0.3])
def test_fp32_field_by_class(seed, theta):
    n, k = 65536, 8192
    p, m = FR.plummer_disc(n, seed)
    pts = FR.class_points(p, k, seed)
    tree = O.build_tree(p, m, 0)
    d = FR.oracle_at_points(tree, p, m, pts, theta=theta, compat=False, pos_rounded=True, cap_depth=21)
    ones = np.ones(k)
    for prec in (P.F32, P.MIXED):
        with engine(n, precision=prec, theta=theta, max_depth=21, reference_compat=False) as e:
            e.upload(p, np.zeros_like(p), m)
            acc, _, cnt = e.field(pts, with_counts=True)
        rep = PC.classify(acc, cnt, ones, pts, theta, k, diag=d)
        print(prec.name, rep)
        assert rep.clean_fraction >= 0.995, rep
        assert rep.clean_count_mismatches == 0, rep
        assert rep.clean_model_max <= PC.MODEL_MAX, rep
        assert rep.nonfinite <= 1e-3 * k, rep
        ok = np.isfinite(d.forces).all(axis=1)
        model, flip = class_terms(d, k)
        err = np.linalg.norm(acc - d.forces, axis=1)
        b = ok & (flip > 0)
        assert (err[b] <= flip[b] + model[b]).all(), (prec.name, float((err[b] / (flip[b] + model[b])).max()))
        assert rep.cap_affected == 0, rep


# ---- 3. fp32 self-consistency ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat", [True, False])
def test_fp32_field_at_the_bodies_takes_the_force_walks_terms(compat):
    n, theta = 32768, 0.5
    p, m = FR.plummer_disc(n, 4)
    with engine(n, precision=P.F32, theta=theta, max_depth=21, reference_compat=compat, flags=FLAG_WALK_STATS) as e:
        e.upload(p, np.zeros_like(p), m)
        e.compute_forces()
        fc = e.interaction_counts()
        a_walk = e.accelerations()
        acc, _, cnt = e.field(e.download()[0], with_counts=True)
    assert np.array_equal(cnt, fc)
    d = O.compute_forces_diag(O.build_tree(p, m, 0), p, m, theta=theta, compat_self_skip=False, pos_rounded=True, cap_depth=21)
    model = 2.0 ** -24 * ((1.5 * np.sqrt(d.counts) + 8.0) * d.abs_sum + 4.0 * d.coord) / m
    ok = np.isfinite(d.forces).all(axis=1)
    err = np.linalg.norm(acc - a_walk, axis=1)
    print("max err / (2 model): %.3f" % (err[ok] / (2.0 * model[ok])).max())
    assert (err[ok] <= 2.0 * model[ok]).all(), float((err[ok] / (2.0 * model[ok])).max())


# ---- 4. independence, bit for bit per point --------------------------------------------------------------------------
def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("prec", ALL)
def test_a_points_field_does_not_depend_on_the_rest_of_the_call(prec):
    n = 4096
    p, m = FR.clumped(n, 9)
    if prec == P.F32:
        p, m = p.astype(np.float32).astype(np.float64), m.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(21)
    a = FR.points_around(p, 5000, 8)
    with engine(n, precision=prec, max_depth=21, reference_compat=False) as e:
        e.upload(p, np.zeros_like(p), m)
        full = e.field(a, with_counts=True)
        assert np.isfinite(full[0]).all() and (full[2] > 0).all()
        perm = rng.permutation(len(a))
        assert same(e.field(a[perm], with_counts=True), [x[perm] for x in full])
        h1, h2 = e.field(a[:1777], with_counts=True), e.field(a[1777:], with_counts=True)
        assert same([np.concatenate([x, y]) for x, y in zip(h1, h2)], full)
        dup = np.concatenate([a[:100], a[7:8], a[100:], a[7:8]])
        r = e.field(dup, with_counts=True)
        assert same([x[[100, -1]] for x in r], [x[[7, 7]] for x in full])
        assert same([np.concatenate([x[:100], x[101:-1]]) for x in r], full)
        # 2^20 + 65 points: two launches, the last 2,500 points of `a` across the boundary
        total = (1 << 20) + 65
        lo, hi = p.min(axis=0), p.max(axis=0)
        filler = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (total - len(a), 2))
        big = np.concatenate([a[:2500], filler, a[2500:]])
        r = e.field(big, with_counts=True)
        assert same([np.concatenate([x[:2500], x[-2500:]]) for x in r], full)
        only = e.field(a, with_counts=False)
        assert len(only) == 2 and same(only, full[:2])


# ---- 5. non-perturbation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,n_threads", [(P.F64_EXACT, 0), (P.F64, 4096), (P.MIXED, 0), (P.F32, 4096)])
def test_field_calls_do_not_perturb_the_run(prec, n_threads):
    n, steps = 24000, 20
    m, p, v = IC.make("plummer", n, 4, quasi_static=True)
    pts = FR.points_around(p, 4000, 2)

    def run(with_field, flags=0, k=steps):
        with engine(n, precision=prec, n_threads=n_threads, flags=flags) as e:
            e.upload(p, v, m)
            for _ in range(k):
                e.step(1)
                if with_field:
                    e.field(pts)
            return e.download()

    (p0, v0), (p1, v1) = run(False), run(True)
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
    flags = 0 if prec == P.F64_EXACT else FLAG_WALK_STATS
    with engine(n, precision=prec, n_threads=n_threads, flags=flags) as e:
        e.upload(p, v, m)
        e.step(3)
        e.compute_forces()
        f0, s0 = e.forces(), e.stats()
        c0 = e.interaction_counts() if flags else None
        e.field(pts, with_counts=True)
        f1, s1 = e.forces(), e.stats()
        assert np.array_equal(f0, f1)
        assert s1.walk_launches == s0.walk_launches and s1.walk_launches == (1 if n_threads == 0 else -(-n // 4096))
        assert (s1.visits, s1.interactions, s1.wave_nodes, s1.wave_quads, s1.wave_accepts) == \
               (s0.visits, s0.interactions, s0.wave_nodes, s0.wave_quads, s0.wave_accepts)
        # (the same events read twice: the runtime's tick-to-time conversion may differ in the last digits between two reads --
        # 1e-6 relative was seen --, while a walk or build of the field call recorded into them would show at the 1e-2 level)
        assert (s1.last_step_ms, s1.walk_ms, s1.build_ms) == pytest.approx((s0.last_step_ms, s0.walk_ms, s0.build_ms), rel=1e-4)
        if flags:
            assert np.array_equal(c0, e.interaction_counts())


@pytest.mark.parametrize("prec,n_threads", QC.CASES, ids=QC.IDS)
def test_field_calls_do_not_perturb_the_stats_of_the_last_step(prec, n_threads):
    """tests/quiet_case.py: a first build by the LSD passes, the field's quiet build by the bucket sort; the walk counters are
    the force walk's (BH_FLAG_WALK_STATS)."""
    pts = FR.points_around(QC.bodies()[1], 500, 2)
    QC.check(prec, n_threads, lambda e: e.field(pts, with_counts=True), flags=0 if prec == P.F64_EXACT else FLAG_WALK_STATS)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ALL)
def test_edges(prec):
    g = 6.67e-11
    f64 = prec in (P.F64_EXACT, P.F64)
    with engine(16, precision=prec) as e:
        with pytest.raises(G.BhError) as ei:                      # before upload
            e.field([[0.0, 0.0]])
        assert ei.value.code == ERR_STATE
        # zero bodies
        e.upload(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        acc, phi, cnt = e.field([[0.0, 0.0], [1.0, 2.0]], with_counts=True)
        assert not acc.any() and not phi.any() and not cnt.any() and acc.shape == (2, 2)
        # one body
        e.upload([[0.25, 0.5]], [[0.0, 0.0]], [2.0])
        acc, phi, cnt = e.field([[1.25, 0.5], [0.25, -1.5]], with_counts=True)
        assert cnt.tolist() == [1, 1]
        tol = 1e-14 if f64 else 1e-6
        assert np.allclose(acc, [[-2.0 * g, 0.0], [0.0, 2.0 * g / 4.0]], rtol=tol, atol=0.0)
        assert np.allclose(phi, [-2.0 * g, -2.0 * g / 2.0], rtol=tol, atol=0.0)
        # n_points = 0
        acc, phi, cnt = e.field(np.zeros((0, 2)), with_counts=True)
        assert acc.shape == (0, 2) and phi.shape == (0,) and cnt.shape == (0,)
        # a NaN / inf coordinate
        for bad in (np.nan, np.inf):
            with pytest.raises(G.BhError) as ei:
                e.field([[0.0, 0.0], [bad, 1.0]])
            assert ei.value.code == ERR_ARG
        # all outputs NULL, n_points < 0, null points
        assert e._lib.bh_field_at(e._h, None, 0, None, None, None) == ERR_ARG
        out = np.zeros(2)
        dp = out.ctypes.data_as(_lib._dp)
        assert e._lib.bh_field_at(e._h, dp, -1, dp, None, None) == ERR_ARG
        assert e._lib.bh_field_at(e._h, None, 1, dp, None, None) == ERR_ARG
        assert e._lib.bh_field_at(e._h, None, 0, dp, None, None) == 0


@pytest.mark.parametrize("prec", ALL)
def test_far_point_and_midpoint(prec, init1024):
    m, p, v = init1024
    if prec == P.F32:
        m, p = m.astype(np.float32).astype(np.float64), p.astype(np.float32).astype(np.float64)
    gconst = 6.67e-11
    with engine(1024, precision=prec) as e:
        e.upload(p, v, m)
        e.build_tree()
        root = e.export_tree()[0][0]
        size = max(root["xmax"] - root["xmin"], root["ymax"] - root["ymin"])
        far = np.array([[root["comx"] + 1e6 * size, root["comy"] - 0.5e6 * size]])
        acc, phi, cnt = e.field(far, with_counts=True)
    assert cnt.tolist() == [1]
    dx, dy = root["comx"] - far[0, 0], root["comy"] - far[0, 1]
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2) + 1e-15
    term = np.array([gconst * root["mass"] / d2 * (dx / d), gconst * root["mass"] / d2 * (dy / d)])
    if prec in (P.F64_EXACT, P.F64):
        assert np.linalg.norm(acc[0] - term) <= FR.accel_bound(1, np.linalg.norm(term))
        assert abs(phi[0] + gconst * root["mass"] / d) <= FR.accel_bound(1, gconst * root["mass"] / d)
    else:                                                         # (fp32 centre of mass, fp32 terms)
        assert np.allclose(acc[0], term, rtol=1e-5, atol=0.0) and phi[0] == pytest.approx(-gconst * root["mass"] / d, rel=1e-5)
    # two equal masses: nothing at their midpoint, phi = -2 G M / d
    mm, sep = 3.0, 0.5
    with engine(2, precision=prec) as e:
        e.upload([[-0.25, 0.125], [0.25, 0.125]], np.zeros((2, 2)), [mm, mm])
        acc, phi, cnt = e.field([[0.0, 0.125]], with_counts=True)
    assert cnt.tolist() == [2]
    one = gconst * mm / (sep / 2) ** 2
    if prec in (P.F64_EXACT, P.F64):
        assert np.linalg.norm(acc[0]) <= FR.accel_bound(2, 2 * one)
        assert abs(phi[0] + 2 * gconst * mm / (sep / 2 + 1e-15)) <= FR.accel_bound(2, 2 * gconst * mm / (sep / 2))
    else:
        assert np.linalg.norm(acc[0]) <= 2.0 ** -22 * 2 * one and phi[0] == pytest.approx(-2 * gconst * mm / (sep / 2), rel=1e-6)


def test_let_mode_has_no_field():
    with engine(1024, precision=P.F32) as e:
        m, p, v = IC.make("uniform", 1000, 1)
        e.upload(p, v, m)
        e.let_configure(0, 2, 1024)
        with pytest.raises(G.BhError) as ei:
            e.field([[0.0, 0.0]])
        assert ei.value.code == ERR_STATE


def test_device_bytes_count_the_field_buffers():
    m, p, v = IC.make("uniform", 1024, 3)
    with engine(1024) as e:
        e.upload(p, v, m)
        b0 = e.stats().device_bytes
        e.field(p[:10] + 1e-3)
        b1 = e.stats().device_bytes
        e.field(p[:100] + 1e-3)
        assert b1 > b0 and e.stats().device_bytes == b1
        e.field(np.tile(p, (3, 1)) + 1e-3)                       # more points than the first block holds
        assert e.stats().device_bytes > b1


# ---- 7. CLI ------------------------------------------------------------------------------------------------------------
def test_project_field_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), positions_file="pos.txt", field_file="field.csv",
                                         field_grid=(16, 8))
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), positions_file="pos.txt")
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    assert (a / "pos.txt").read_bytes() == (b / "pos.txt").read_bytes()
    assert not (b / "field.csv").exists()
    lines = (a / "field.csv").read_text().splitlines()
    assert lines[0] == "# x,y,ax,ay,phi" and len(lines) == 1 + 128
    rows = np.array([[float(t) for t in l.split(",")] for l in lines[1:]])
    x0, x1, y0, y1 = pa[:, 0].min(), pa[:, 0].max(), pa[:, 1].min(), pa[:, 1].max()
    xs = x0 + (np.arange(16) + 0.5) * ((x1 - x0) / 16)
    ys = y0 + (np.arange(8) + 0.5) * ((y1 - y0) / 8)
    assert np.array_equal(rows[:, 0], np.tile(xs, 8)) and np.array_equal(rows[:, 1], np.repeat(ys, 16))
    with engine(1024) as e:
        e.upload(p, v, m)
        e.build_tree(); e.step(1); e.build_tree(); e.step(1)      # (as runSimulationGpu steps)
        acc, phi = e.field(rows[:, :2])
    assert np.array_equal(rows[:, 2:4], acc) and np.array_equal(rows[:, 4], phi)
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["--n-bodies", "1024", "--n-simulations", "2", "--init", "files", "--field-file", "main.csv",
                             "--field-grid", "16", "8"]) == 0
    finally:
        os.chdir(cwd)
    assert (tmp_path / "main.csv").read_text() == (a / "field.csv").read_text()
