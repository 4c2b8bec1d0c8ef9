"""Potential and energy of the distributed (LET) step: bh_let_potential, bh_let_get_potential, bh_let_energy and what
distributed.LetStepper.potential() / energy() do with them, on one GPU through emulated ranks (tests/let_energy_ranks.py).

  1. the forest potential walk takes exactly the forest force walk's terms: per-body counts == bh_get_interaction_counts
     of the same forest, for every body of every rank, whatever shape the force walk runs;
  2. phi against the fp64 forest reference (tests/forest_potential_ref.py) on the bodies whose counts are the reference's;
  3. each rank's eight sums and the combined energy against math.fsum, bitwise repeatable;
  4. energy() + potential() around every step leave trajectory, ownership, ORB cuts and walk launches bit for bit;
  5. the total potential energy against the exact pair sum;
  6. errors, an outgrown let_cap, allocation on first use."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import forest_potential_ref as FP  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import _lib  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.distributed import partition_orb  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_STATS  # noqa: E402
from let_energy_ranks import EnergyRanks  # noqa: E402
from let_ranks import expected_split  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5

# Relative error of phi against the fp64 forest reference on the sampled bodies of "plummer-orb4" whose term counts are
# the reference's (test 2): 2 x the maximum measured on MI355X.
#   measured: F32 9.85e-8, MIXED 9.85e-8 (the uploaded state is fp32-representable: both precisions walk the same numbers)
# -- two thousand times below the single tree's all-bodies 2.33e-4 (tests/test_gpu_energy.py: F32_TOL_ALL), which comes from
# depth-cap aggregates close to their own bodies; this state runs uncapped (max_depth 21), its value sits beside the
# single tree's sampled 1.47e-6 (F32_TOL).
FOREST_TOL = 2e-7
# Relative difference of the total potential energy from the exact fp64 pair sum, 4,096-body Plummer sphere on 4 ranks at
# theta 0.3 (test 5): 2 x the value measured on MI355X.
#   measured: forest 1.289e-3 (pair sum -23.6736474, forest -23.6431242), the single-GPU engine on the same state 1.347e-3
#   (-23.6417594): a Barnes-Hut truncation error, the forest's as large as the single tree's.
PAIR_SUM_TOL = 2.6e-3


def round_robin(p, w):
    """Every rank's boxes cover everything: correctness may not depend on compact domains."""
    return [np.arange(r, len(p), w) for r in range(w)]


def random_deal(p, w):
    """Every body dealt at random to one of w - 1 ranks: rank 1 stays empty; rank 3 keeps fewer than 64 bodies."""
    rng = np.random.default_rng(23)
    live = np.array([r for r in range(w) if r != 1])
    owner = live[rng.integers(0, len(live), len(p))]
    few = np.flatnonzero(owner == 3)
    owner[few[40:]] = 0
    return [np.flatnonzero(owner == r) for r in range(w)]


def odd_rank(p, w):
    """ORB on two ranks with the cut moved so that rank 0 holds 64 k + 1 bodies."""
    a, b = partition_orb(p, 2)
    k = (len(a) // 64) * 64 + 1
    order = np.argsort(p[np.concatenate([a, b]), 0], kind="stable")
    ix = np.concatenate([a, b])[order]
    return [ix[:k], ix[k:]]


def clumped(n, seed):
    """tests/test_gpu_let_parity.py::clumped: a few tight clusters over a sparse background -- with max_depth = 8 most
    bodies sit in depth-cap cells."""
    r = np.random.default_rng(seed)
    c = r.uniform(-1, 1, (6, 2))
    p = c[r.integers(0, 6, n)] + r.normal(0, 2e-2, (n, 2))
    p[: n // 6] = r.uniform(-1, 1, (n // 6, 2))
    p = p.astype(np.float32).astype(np.float64)
    m = (10.0 ** r.uniform(-2, 0, n)).astype(np.float32).astype(np.float64)
    return m, p, np.zeros((n, 2))


# name: (state, partition, world, config, waves per group of the force walk or None)
TERM_CASES = {
    "uniform4099-orb3": (lambda: IC.make("uniform", 4099, 1, quasi_static=True), partition_orb, 3, {}, 8),
    "uniform4099-round-robin3": (lambda: IC.make("uniform", 4099, 1, quasi_static=True), round_robin, 3, {}, 8),
    "random-deal5": (lambda: IC.make("uniform", 3000, 2, quasi_static=True), random_deal, 5, {}, None),
    "world1": (lambda: IC.make("plummer", 5000, 3, quasi_static=True), partition_orb, 1, {}, 8),
    "rank-of-64k+1": (lambda: IC.make("plummer", 6000, 4, quasi_static=True), odd_rank, 2, {}, 8),
    "clumped30000-depth8": (lambda: clumped(30000, 5), partition_orb, 3, {"max_depth": 8, "reference_compat": False}, 8),
    "plummer200000-four-waves": (lambda: IC.make("plummer", 200000, 2, quasi_static=True), partition_orb, 3, {}, 4),
}


@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
@pytest.mark.parametrize("case", list(TERM_CASES))
def test_forest_potential_takes_the_forest_force_walks_terms(case, prec):
    make, partition, world, cfg, waves = TERM_CASES[case]
    m, p, v = make()
    er = EnergyRanks(m, p, v, world, None, partition=partition, precision=prec, flags=FLAG_WALK_STATS, **cfg)
    try:
        sizes = [len(ix) for ix in er.parts]
        if waves is not None:
            assert {expected_split(s, world=world) for s in sizes} == {waves}, sizes
        if case == "random-deal5":
            assert sizes[1] == 0 and 0 < sizes[3] < 64, sizes
        if case == "rank-of-64k+1":
            assert sizes[0] % 64 == 1, sizes
        er.step(integrate=False)
        direct = []
        for e in er.engs:
            if e.n == 0:                                     # (a rank without bodies launches no walk and has no counts)
                phi, cnt = e.let_potential(with_counts=True)
                assert len(phi) == 0 and len(cnt) == 0
                direct.append((phi, cnt))
                continue
            fc = e.interaction_counts()
            phi, cnt = e.let_potential(with_counts=True)     # the forest the step left
            assert np.array_equal(cnt, fc), (case, int((cnt != fc).sum()))
            assert np.isfinite(phi).all() and (phi < 0).all()
            assert np.array_equal(e.interaction_counts(), fc)              # (the force walk's counts are left alone)
            direct.append((phi, cnt))
        # the diagnostic's own (quiet) forest of the same state: the same bits, and again
        for again in range(2):
            for (phi, cnt), (phi2, cnt2) in zip(direct, er.potential(with_counts=True)):
                assert np.array_equal(phi, phi2) and np.array_equal(cnt, cnt2)
    finally:
        er.close()


# ---- 2. against the fp64 forest reference --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plummer_orb4():
    """The "plummer-orb4" state of tests/test_gpu_let_parity.py, a seeded sample of 4,096 bodies and the reference."""
    m, p, v = IC.make("plummer", 65536, 1, quasi_static=True)
    m, p = (x.astype(np.float32).astype(np.float64) for x in (m, p))
    parts = partition_orb(p, 4)
    sample = np.sort(np.random.default_rng(5).choice(len(m), 4096, replace=False))
    ref, rcnt = FP.forest_potential(m, p, parts, theta=0.5, bodies=sample)
    return m, p, v, parts, sample, ref, rcnt


@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
def test_forest_potential_against_the_fp64_forest_reference(plummer_orb4, prec):
    """Measured on MI355X, F32 and MIXED alike: 0.99976 of the sample with the reference's terms; on those bodies max
    9.85e-8 and median 8.94e-9 relative (over the whole sample, other terms included: 8.5e-6)."""
    m, p, v, parts, sample, ref, rcnt = plummer_orb4
    er = EnergyRanks(m, p, v, 4, None, partition=lambda pp, w: parts, theta=0.5, precision=prec, max_depth=21,
                     reference_compat=False)                  # (the configuration of the parity case: nothing is capped)
    try:
        out = er.potential(with_counts=True)
        phi = er.gather1(lambda e: out[er.engs.index(e)][0], dtype=np.float64)
        cnt = er.gather1(lambda e: out[er.engs.index(e)][1])
    finally:
        er.close()
    same = cnt[sample] == rcnt
    err = np.abs(phi[sample] - ref) / np.abs(ref)
    print(f"forest potential {prec.name}: {same.mean():.5f} of the sample with the reference's terms, "
          f"max rel {err[same].max():.4g}, median {np.median(err[same]):.3g}, max over all {err.max():.4g}")
    assert same.mean() >= 0.99
    assert err[same].max() <= FOREST_TOL


# ---- 3. reductions -------------------------------------------------------------------------------------------------
def _terms(mm, x, u, phi):
    return [mm, mm * x[:, 0], mm * x[:, 1], mm * u[:, 0], mm * u[:, 1], mm * (x[:, 0] * u[:, 1] - x[:, 1] * u[:, 0]),
            mm * (u ** 2).sum(axis=1), mm * phi]


@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
def test_rank_sums_and_combined_energy_against_fsum(prec):
    m, p, _ = clumped(30000, 5)
    v = np.random.default_rng(9).normal(0.0, 1e-4, p.shape)
    er = EnergyRanks(m, p, v, 3, None, headroom=2.0, precision=prec)
    try:
        for s in range(17):                                  # (a physical re-order has run; the state is in device order)
            er.step()
            if s == 8:
                er.rebalance()
        a = er.energy()
        rows = er.energy_rows()
        b = er.energy()
        assert a == b and rows == er.energy_rows()           # the same bits, call after call
        state = []
        for e, row in zip(er.engs, rows):
            phi = e.let_potential()
            x, u = e.download()
            mm = e.masses()
            state.append((mm, x, u, phi))
            for k, t in enumerate(_terms(mm, x, u, phi)):
                ref, scale = math.fsum(t), math.fsum(np.abs(t))
                assert abs(row[k] - ref) <= 1e-13 * scale, (k, row[k], ref)
            assert row[8] == e.n
    finally:
        er.close()
    mm, x, u, phi = (np.concatenate([s[k] for s in state]) for k in range(4))
    S = [math.fsum(t) for t in _terms(mm, x, u, phi)]
    A = [math.fsum(np.abs(t)) for t in _terms(mm, x, u, phi)]
    got = [a.mass, a.com[0] * a.mass, a.com[1] * a.mass, a.momentum[0], a.momentum[1], a.angular_momentum,
           2.0 * a.kinetic, 2.0 * a.potential]
    for k in range(8):
        assert abs(got[k] - S[k]) <= 1e-13 * A[k], (k, got[k], S[k])
    assert a.total == a.kinetic + a.potential and a.n_bodies == len(m)


# ---- 4. non-perturbation -------------------------------------------------------------------------------------------
def moving(n, seed):
    """clumped() with velocities that carry bodies across cells and ORB cuts within a few steps (the quasi-static
    Plummer state hardly moves in fp32: its case pins the bookkeeping, this one the trajectory)."""
    m, p, _ = clumped(n, seed)
    return m, p, np.random.default_rng(seed + 1).normal(0.0, 2e-3, p.shape).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("two", [False, True], ids=["one-launch", "two-launch"])
@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
@pytest.mark.parametrize("state", ["plummer24000", "moving30000"])
def test_diagnostics_do_not_perturb_the_distributed_run(state, prec, two):
    m, p, v = IC.make("plummer", 24000, 4, quasi_static=True) if state == "plummer24000" else moving(30000, 5)
    runs = []
    for diag in (False, True):
        er = EnergyRanks(m, p, v, 3, None, headroom=2.0, precision=prec)
        try:
            def look():
                if diag:
                    e = er.energy()
                    assert np.isfinite(e.total) and e.n_bodies == len(m)
                    er.potential()
            look()
            cuts = None
            for s in range(20):
                er.step(two_launches=two)
                look()
                if s == 9:
                    cuts, _ = er.rebalance()
                    look()
            runs.append((er.gather(lambda e: e.download()[0]), er.gather(lambda e: e.download()[1]), er.ids(),
                         cuts.value.copy(), cuts.axis.copy(), [e.stats().walk_launches for e in er.engs]))
        finally:
            er.close()
    (x0, v0, i0, c0, a0, w0), (x1, v1, i1, c1, a1, w1) = runs
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)
    assert all(np.array_equal(a, b) for a, b in zip(i0, i1))
    assert np.array_equal(c0, c1) and np.array_equal(a0, a1)
    assert w0 == w1
    if state == "moving30000":
        assert (x0 != p).any(axis=1).all() and any(not np.array_equal(np.sort(a), np.sort(ix)) for a, ix in zip(i0, er.parts))


# ---- 5. physics ----------------------------------------------------------------------------------------------------
def test_total_potential_energy_against_the_exact_pair_sum():
    """Measured on MI355X: forest 1.289e-3, single GPU 1.347e-3 relative (PAIR_SUM_TOL has the values)."""
    n, theta = 4096, 0.3
    m, p, v = IC.plummer(n, 21)
    U = 0.0
    for i in range(n - 1):                                   # U = -G sum_{i<j} m_i m_j / d_ij, G = 1, fp64
        d = np.sqrt(((p[i + 1:] - p[i]) ** 2).sum(axis=1))
        U -= m[i] * math.fsum(m[i + 1:] / d)
    cfg = dict(G=1.0, theta=theta, precision=P.F32, max_depth=21, reference_compat=False)
    er = EnergyRanks(m, p, v, 4, None, **cfg)
    try:
        e = er.energy()
    finally:
        er.close()
    with G.BarnesHutEngine(G.BhConfig(capacity=n, **cfg)) as one:
        one.upload(p, v, m)
        single = one.energy().potential
    rel, rel1 = abs(e.potential - U) / abs(U), abs(single - U) / abs(U)
    print(f"plummer {n} theta {theta}: pair sum {U:.9g}, forest {e.potential:.9g} (rel {rel:.4g}), "
          f"single GPU {single:.9g} (rel {rel1:.4g})")
    assert e.kinetic == 0.0 and e.n_bodies == n
    assert rel <= PAIR_SUM_TOL


# ---- 6. errors and state -------------------------------------------------------------------------------------------
def test_errors_and_state():
    lib = _lib.load()
    phi = np.zeros(4096)
    dp = phi.ctypes.data_as(C.POINTER(C.c_double))
    q = np.zeros(8)
    dq = q.ctypes.data_as(C.POINTER(C.c_double))
    m, p, v = IC.make("uniform", 1000, 1)
    assert lib.bh_let_potential(None) == ERR_ARG
    for prec in (P.F32, P.F64):                              # not in LET mode (a precision without LET never is)
        with G.BarnesHutEngine(G.BhConfig(capacity=1000, precision=prec)) as e:
            e.upload(p, v, m)
            assert lib.bh_let_potential(e._h) == ERR_STATE
            assert lib.bh_let_get_potential(e._h, dp, None) == ERR_STATE
            assert lib.bh_let_energy(e._h, dq) == ERR_STATE
    with G.BarnesHutEngine(G.BhConfig(capacity=1000, precision=P.F32)) as e:
        e.upload(p, v, m)
        e.let_configure(0, 1, 2048)
        h = e._h
        assert lib.bh_let_potential(h) == ERR_STATE          # before bh_let_build
        assert lib.bh_let_energy(h, dq) == ERR_STATE
        assert lib.bh_let_get_potential(h, None, None) == ERR_ARG and lib.bh_let_energy(h, None) == ERR_ARG
        e.let_bounds()
        lb, ab, *_ = e.let_pointers()
        import torch
        from gpu_nbody_simulation_amd.distributed import wrap_device
        dev = torch.device("cuda", 0)
        e.sync()
        wrap_device(ab, 32, "<f8", dev).copy_(wrap_device(lb, 32, "<f8", dev))
        torch.cuda.synchronize()
        e.let_build()
        assert lib.bh_let_get_potential(h, dp, None) == ERR_STATE     # not computed yet
        assert lib.bh_let_potential(h) == 0 and lib.bh_let_get_potential(h, dp, None) == 0
        assert lib.bh_let_energy(h, dq) == 0 and q[0] > 0
        # the single-context diagnostics still refuse a LET context
        assert lib.bh_compute_potential(h) == ERR_STATE and lib.bh_get_potential(h, dp, None) == ERR_STATE
        e.let_walk()                                         # an integrating walk: the state moved on
        assert lib.bh_let_get_potential(h, dp, None) == ERR_STATE
        assert lib.bh_let_potential(h) == ERR_STATE          # the tree in place is the old state's


def test_an_outgrown_let_cap_completes_is_reported_and_raises():
    m, p, v = IC.make("uniform", 4099, 1, quasi_static=True)
    er = EnergyRanks(m, p, v, 3, None)
    try:
        er.step(integrate=False)
        largest = er.check()
        assert largest > 16
        er.configure(16)                                     # far smaller than the largest LET of this state
        er.forest()
        for e in er.engs:
            phi = e.let_potential()                          # completes: links past the block are cut by the packer
            assert np.isfinite(phi).all()
        looks = [e.let_counts(with_overflow=True) for e in er.engs]
        # (the counters hold the sizes the LETs would have had: the diagnostic's build is counted like a step's)
        assert any(ov for _, ov in looks) and max(max(c) for c, _ in looks) > 16
        with pytest.raises(RuntimeError):
            er.potential()
        with pytest.raises(RuntimeError):
            er.energy()
    finally:
        er.close()


def test_buffers_are_allocated_at_the_first_call_only():
    m, p, v = IC.make("uniform", 5000, 2, quasi_static=True)
    er = EnergyRanks(m, p, v, 2, None)
    try:
        er.step()
        er.step(integrate=False)
        for e in er.engs:
            cap = e.cfg.capacity
            before = e.stats().device_bytes
            e.let_potential()
            grown = e.stats().device_bytes - before
            assert grown == cap * 8 + cap * 4 + 256 * 2 * 8 * 8 + 8 * 8      # phi, counts, the reduction records
            e.let_energy_sums()
            e.let_potential(with_counts=True)
            assert e.stats().device_bytes == before + grown
    finally:
        er.close()
