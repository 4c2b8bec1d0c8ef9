"""On-device direct-sum forces (bh_direct_forces) and the Barnes-Hut force check (bh_force_check, force_error):

  * the direct sum is main_approach_1.cpp:53-75 bit for bit -- the reference's own binary's forces on init1024, the
    oracle's direct sum of the state the device holds (widened) in all four precisions, also after the fp32 / mixed
    state has been re-ordered physically, and tests/direct_ref.py on sampled targets of a 1M Plummer sphere;
  * targets: any order, repeats, subsets; the error cases;
  * the check does not perturb the run, and its tree forces are the precision's force walk;
  * physics: the error grows with theta; the project.py force-error file."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import _lib, initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_STATS, force_error_stats  # noqa: E402
from gpu_nbody_simulation_amd.project import runSimulationGpu  # noqa: E402
from direct_ref import direct_ref, same_bits  # noqa: E402
import quiet_case as QC  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5


def engine(n, **kw):
    return G.BarnesHutEngine(G.BhConfig(capacity=n, **kw))


def rounded(*a):
    return [x.astype(np.float32).astype(np.float64) for x in a]


def clumped_with_duplicates(n, seed):
    """Gaussian clumps of different widths, and a few bodies placed exactly on others (inf / NaN in the direct sum)."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-1.0, 1.0, (8, 2))
    widths = 10.0 ** r.uniform(-3.0, -1.0, 8)
    k = r.integers(0, 8, n)
    p = centres[k] + r.normal(0.0, 1.0, (n, 2)) * widths[k, None]
    p = p.astype(np.float32).astype(np.float64)            # (so that the duplicates stay duplicates in fp32)
    for a, b in ((10, 11), (200, 4000), (4000, 8000 % n), (n - 1, 3)):
        p[b] = p[a]
    return r.uniform(0.1, 0.5, n), p, r.normal(0.0, 1e-4, (n, 2))


# ---- 1. the reference's binary ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(P))
def test_init1024_direct_forces_are_the_reference_binarys(gold, init1024, prec):
    m, p, v = init1024
    with engine(1024, precision=prec) as e:
        e.upload(p, v, m)
        f = e.direct_forces()
    if prec == P.F32:
        pr, mr = rounded(p, m)
        assert np.array_equal(f, O.direct_forces(pr, mr))
    else:
        assert np.array_equal(f, gold("ref_ma1_1024")["forces_0"])


# ---- 2. bit for bit in all four precisions, after re-ordering -----------------------------------------------------
@pytest.mark.parametrize("prec", list(P))
@pytest.mark.parametrize("name", ["random4096", "clumped8192"])
def test_direct_forces_are_the_oracles_of_the_device_state(prec, name):
    if name == "random4096":
        m, p, v = IC.make("uniform", 4096, 11)
    else:
        m, p, v = clumped_with_duplicates(8192, 5)
    n = len(m)
    # fp32 / mixed: dt = 0 keeps the state where it is while 17 steps re-order it physically twice (builds 0 and 16);
    # the fp32 walk lets a coincident pair contribute nothing, so the duplicates' accelerations stay finite
    with engine(n, precision=prec, dt=0.0 if prec in (P.F32, P.MIXED) else 1.0) as e:
        e.upload(p, v, m)
        if prec in (P.F32, P.MIXED):
            e.step(17)
        x, _ = e.download()
        mm = e.masses()
        f = e.direct_forces()
    assert same_bits(f, O.direct_forces(x, mm))
    if name == "clumped8192":
        assert np.isnan(f[[10, 11, 200, 4000, 3]]).all()
        assert np.isfinite(f).all(axis=1).sum() == n - 7


# ---- 3. targets and errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F64_EXACT, P.F32])
def test_targets_select_rows_of_the_all_targets_call(prec):
    m, p, v = IC.make("plummer", 5000, 2)
    with engine(5000, precision=prec, dt=0.0) as e:
        e.upload(p, v, m)
        e.step(17)
        full = e.direct_forces()
        r = np.random.default_rng(4)
        shuffled = r.permutation(5000)
        repeated = np.concatenate([r.integers(0, 5000, 3000), [0, 0, 4999, 4999]])   # more targets than capacity
        repeated = np.concatenate([repeated, repeated])
        subset = np.array([17, 3, 4999])
        for t in (shuffled, repeated, subset):
            assert np.array_equal(e.direct_forces(t), full[t])
        assert e.direct_forces([]).shape == (0, 2)
        tree, direct = e.force_check(subset)
        assert np.array_equal(direct, full[subset]) and tree.shape == (3, 2)
        tree0, direct0 = e.force_check([])
        assert tree0.shape == direct0.shape == (0, 2)


def test_errors_and_edge_cases():
    lib = _lib.load()
    out = np.zeros((8, 2))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    tg = (C.c_int64 * 2)(0, 1)
    with engine(64) as e:
        h = e._h
        assert lib.bh_direct_forces(h, tg, 2, dp) == ERR_STATE             # before upload
        assert lib.bh_force_check(h, tg, 2, dp, dp) == ERR_STATE
        m, p, v = IC.make("uniform", 64, 1)
        e.upload(p, v, m)
        assert lib.bh_direct_forces(None, tg, 2, dp) == ERR_ARG
        assert lib.bh_direct_forces(h, tg, 2, None) == ERR_ARG
        assert lib.bh_force_check(h, tg, 2, dp, None) == ERR_ARG
        assert lib.bh_force_check(h, tg, 2, None, dp) == ERR_ARG
        assert lib.bh_direct_forces(h, tg, -1, dp) == ERR_ARG
        assert lib.bh_force_check(h, tg, -1, dp, dp) == ERR_ARG
        assert lib.bh_direct_forces(h, None, 8, dp) == ERR_ARG              # NULL takes all n = 64
        for bad in ((C.c_int64 * 2)(0, 64), (C.c_int64 * 2)(-1, 0)):
            assert lib.bh_direct_forces(h, bad, 2, dp) == ERR_ARG
            assert lib.bh_force_check(h, bad, 2, dp, dp) == ERR_ARG
        assert lib.bh_direct_forces(h, tg, 0, dp) == 0
        assert lib.bh_force_check(h, tg, 0, dp, dp) == 0
    with engine(4, precision=P.F64) as e:                                     # n = 1: the force is zero
        e.upload([[0.3, -0.2]], [[0.0, 0.0]], [2.0])
        assert np.array_equal(e.direct_forces(), np.zeros((1, 2)))
        tree, direct = e.force_check()
        assert np.array_equal(direct, np.zeros((1, 2))) and np.array_equal(tree, np.zeros((1, 2)))
        e.upload(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))            # n = 0
        assert e.direct_forces().shape == (0, 2)
    with engine(4096, precision=P.F32) as e:
        m, p, v = IC.make("uniform", 1000, 1)
        e.upload(p, v, m)
        e.let_configure(0, 2, 1024)
        with pytest.raises(G.BhError) as ex:
            e.direct_forces()
        assert ex.value.code == ERR_STATE
        with pytest.raises(G.BhError) as ex:
            e.force_error()
        assert ex.value.code == ERR_STATE


# ---- 4. scale -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F32, P.F64])
def test_million_body_plummer_sampled_against_direct_ref(prec):
    n = 1 << 20
    m, p, v = IC.plummer(n, 8)
    t = np.random.default_rng(2).choice(n, 64, replace=False)
    with engine(n, precision=prec) as e:
        e.upload(p, v, m)
        f = e.direct_forces(t)
    if prec == P.F32:
        p, m = rounded(p, m)
    assert np.array_equal(f, direct_ref(p, m, t))


# ---- 5. non-perturbation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,n_threads", [(P.F64_EXACT, 0), (P.F64, 0), (P.MIXED, 0), (P.F32, 0), (P.F32, 4096),
                                            (P.F64, 4096)])
def test_force_check_does_not_perturb_the_run(prec, n_threads):
    m, p, v = IC.make("plummer", 24000, 4, quasi_static=True)
    flags = 0 if prec == P.F64_EXACT else FLAG_WALK_STATS
    runs = []
    for check in (False, True):
        with engine(len(m), precision=prec, n_threads=n_threads, flags=flags) as e:
            e.upload(p, v, m)
            for _ in range(20):
                e.step(1)
                if check:
                    f0, s0 = e.forces(), e.stats()
                    c0 = e.interaction_counts() if flags else None
                    r = e.force_error(sample=4096, seed=3)
                    assert r.n == 4096
                    s1 = e.stats()
                    assert np.array_equal(e.forces(), f0)
                    assert (s1.walk_launches, s1.visits, s1.interactions, s1.wave_nodes) == \
                        (s0.walk_launches, s0.visits, s0.interactions, s0.wave_nodes)
                    if flags:
                        assert np.array_equal(e.interaction_counts(), c0)
            runs.append(e.download() + (e.forces(), e.stats().walk_launches))
    (x0, v0, f0, w0), (x1, v1, f1, w1) = runs
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)
    assert np.array_equal(f0, f1) and w0 == w1


@pytest.mark.parametrize("prec,n_threads", QC.CASES, ids=QC.IDS)
def test_force_check_does_not_perturb_the_stats_of_the_last_step(prec, n_threads):
    """tests/quiet_case.py: a first build by the LSD passes, the check's quiet build by the bucket sort; the walk counters are
    the force walk's (BH_FLAG_WALK_STATS), which the check's own walk counts into as well."""
    def check_forces(e):
        f0 = e.forces()
        assert e.force_error(sample=1024, seed=3).n == 1024
        assert np.array_equal(e.forces(), f0)
    QC.check(prec, n_threads, check_forces, flags=0 if prec == P.F64_EXACT else FLAG_WALK_STATS)


# ---- 6. the check's tree forces are the force walk's ---------------------------------------------------------------
@pytest.mark.parametrize("prec", list(P))
def test_check_tree_forces_are_the_force_walks(init1024, prec):
    if prec == P.F64_EXACT:
        m, p, v = init1024
    else:
        m, p, v = IC.make("plummer", 20000, 6)
    n = len(m)
    t = np.random.default_rng(1).permutation(n)[: n // 2]
    # (max_depth 20 outside the exact mode: no two bodies share a key, so the re-ordered state and a fresh upload of it
    # sort into the same order, and every fp32 bucket leaf sums its bodies in the same order)
    md = 10 if prec == P.F64_EXACT else 20
    with engine(n, precision=prec, max_depth=md) as e:
        e.upload(p, v, m)
        e.step(17)                                           # (fp32 / mixed: a physically re-ordered state)
        tree, direct = e.force_check(t)
        r = e.force_error(targets=t)
        x, u = e.download()
        mm = e.masses()
        walk = e.compute_forces()                           # (the same state, the same root box: the last walk's)
    assert np.array_equal(tree, walk[t])
    if prec in (P.F64_EXACT, P.F64):
        # a fresh upload of the downloaded state (fp32 / mixed: that engine's root box comes from the positions pass, not
        # from the bounds the last integrating walk folded, and can differ from it in the last bits)
        with engine(n, precision=prec, max_depth=md) as e:
            e.upload(x, u, mm)
            fresh = e.compute_forces()
        assert np.array_equal(tree, fresh[t])
    assert same_bits(direct, O.direct_forces(x, mm)[t])
    if prec == P.F64_EXACT:
        ob = O.compute_forces(O.build_tree(x, mm, 10), x, mm)
        assert np.array_equal(tree, ob[t])
        assert r == force_error_stats(ob[t], O.direct_forces(x, mm)[t], t)


# ---- 7. physics ---------------------------------------------------------------------------------------------------
def test_error_grows_with_theta_on_a_plummer_sphere():
    """max_depth 21 (the benchmark's): at the reference's default depth of 10 the core of the sphere shares depth-capped
    cells, whose aggregates dominate the error whatever theta."""
    m, p, v = IC.plummer(65536, 12)
    med = {}
    for theta in (0.3, 0.5, 1.0):
        with engine(len(m), precision=P.F64, theta=theta, max_depth=21) as e:
            e.upload(p, v, m)
            r = e.force_error()
        assert r.n + r.n_zero + r.n_nonfinite == len(m)
        med[theta] = r.median
        print(f"plummer 65536 F64 theta {theta}: median {r.median:.3g} p99 {r.p99:.3g} max {r.max:.3g}")
    assert med[0.3] < med[0.5] < med[1.0]
    assert med[0.5] < 3e-2                                  # (loose: measured 0.0130)


# ---- 8. project.py ------------------------------------------------------------------------------------------------
def test_project_force_error_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "plain", tmp_path / "ferr"
    a.mkdir()
    b.mkdir()
    pa, va, _ = runSimulationGpu(m, p, v, 7, out_dir=str(a), positions_file="traj.txt")
    pb, vb, _ = runSimulationGpu(m, p, v, 7, out_dir=str(b), positions_file="traj.txt", force_error_file="ferr.csv",
                                 force_error_every=3, force_error_sample=500)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    for f in ("traj.txt", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / f).read_bytes() == (b / f).read_bytes()
    rows = [line.split(",") for line in (b / "ferr.csv").read_text().splitlines()]
    assert [int(r[0]) for r in rows] == [0, 3, 6, 7]
    assert all(len(r) == 9 for r in rows)
    assert all(int(r[2]) == 500 for r in rows)
    vals = np.array([[float(x) for x in r[3:8]] for r in rows])
    assert (np.diff(vals, axis=1) >= 0).all() and (vals > 0).all()          # median <= p90 <= p99 <= p999 <= max
    with engine(1024) as e:                                                  # the first line is force_error of the start
        e.upload(p, v, m)
        r0 = e.force_error(sample=500)
    assert [float(x) for x in rows[0][3:8]] == [r0.median, r0.p90, r0.p99, r0.p999, r0.max]
    assert int(rows[0][8]) == r0.worst
