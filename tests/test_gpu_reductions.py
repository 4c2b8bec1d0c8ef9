"""The two-pass reductions behind energy() / let_energy_sums() (csrc/bh_diag.hpp) and timestep() (csrc/bh_split.hpp) beyond
one grid-stride trip.  Both run 256 workgroups of 256 threads, so a thread takes a second body from n = 65,537 on; the
sizes, the nearly cancelling state and the derived bound are those of tests/reduction_ref.py, and
tests/test_reductions_cpu.py shows that the bound tells the compensated tree from its broken variants.

  * the eight sums of every precision against math.fsum over the downloaded state, within sum2_tolerance, bit for bit
    the same on a second call; a 300-body system on the context that has just reduced 196,909;
  * the same after a physical re-order (F32 / MIXED: device order is not caller order);
  * each emulated rank's let_energy_sums() over its own bodies;
  * the time-step argmax with the worst body in the first and last slot of a trip, through orig[] past 65,536;
  * ties between records of different trips, workgroups and waves: the smallest caller index wins."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from let_energy_ranks import EnergyRanks  # noqa: E402
import reduction_ref as R  # noqa: E402

P = G.Precision
PRECISIONS = [P.F64_EXACT, P.F64, P.MIXED, P.F32]
IDS = [x.name for x in PRECISIONS]
ENERGY_SIZES = [65536] + R.SIZES
N2 = 131079                          # two whole trips and seven bodies of a third
ETA, LENGTH = 0.02, 1e-3


def conditioned(tt, full=True):
    """The input condition of tests/test_reductions_cpu.py on the downloaded state."""
    for k in (3, 4):
        assert R.condition(tt[k]) >= R.MIN_CONDITION, (R.NAMES[k], R.condition(tt[k]))
    for k in (1, 2) if full else ():
        assert R.condition(tt[k]) >= R.MIN_CONDITION_POSITION, (R.NAMES[k], R.condition(tt[k]))


def reduce_and_check(e, n, what, cancelling=True):
    """energy() twice, then the state it was taken of; the sums against math.fsum.  Returns the first BhEnergy."""
    a = e.energy()
    b = e.energy()
    phi = e.potential()
    x, u = e.download()
    mm = e.masses()
    assert len(mm) == n and np.isfinite(phi).all()
    tt = R.terms(mm, x, u, phi)
    if cancelling:
        conditioned(tt)
    assert a == b, (what, a, b)                              # the same bits twice
    R.check_energy(a, tt, n, what)
    return a


# ---- energy sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ENERGY_SIZES)
@pytest.mark.parametrize("prec", PRECISIONS, ids=IDS)
def test_energy_sums_beyond_one_trip(prec, n):
    m, p, v = R.state(n)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec)) as e:
        e.upload(p, v, m)
        x, u = e.download()
        assert np.array_equal(x, p) and np.array_equal(u, v) and np.array_equal(e.masses(), m)     # fp32-representable
        reduce_and_check(e, n, prec.name)


@pytest.mark.parametrize("prec", PRECISIONS, ids=IDS)
def test_a_smaller_system_on_a_used_context(prec):
    """300 bodies after 196,909: 255 of the 256 partial records and every phi past 300 are the larger system's unless the
    reduction writes and reads only its own."""
    n, small = 196909, 300
    m, p, v = R.state(n)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec)) as e:
        e.upload(p, v, m)
        big = reduce_and_check(e, n, prec.name)
        e.upload(p[:small], v[:small], m[:small])
        # (the first 300 of a shuffled state: no mirrored pairs to speak of, so no condition on this input)
        a = reduce_and_check(e, small, prec.name + " after 196,909", cancelling=False)
        assert a.mass < big.mass / 100


@pytest.mark.parametrize("prec", [P.F32, P.MIXED], ids=["F32", "MIXED"])
def test_energy_sums_in_device_order(monkeypatch, prec):
    """BH_REORDER_EVERY=1 and one step: the state is physically in tree order, phi is indexed by slot.  dt = 1e-12 leaves
    the cancellation standing (asserted on what comes back)."""
    monkeypatch.setenv("BH_REORDER_EVERY", "1")
    n = N2
    m, p, v = R.state(n)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec, dt=1e-12)) as e:
        e.upload(p, v, m)
        e.step(1)
        reduce_and_check(e, n, prec.name + " re-ordered")


# ---- LET -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F32, P.MIXED], ids=["F32", "MIXED"])
def test_rank_sums_beyond_one_trip(prec):
    """Two emulated ranks: rank 0 holds a mirrored state of 65,799 bodies, rank 1 one of 300 (another seed)."""
    sizes = [65799, 300]
    m0, p0, v0 = R.state(sizes[0])
    m1, p1, v1 = R.mirrored_state(sizes[1], R.SEED + 1)
    m, p, v = np.concatenate([m0, m1]), np.concatenate([p0, p1]), np.concatenate([v0, v1])
    assert len(np.unique(p, axis=0)) == len(p)
    parts = [np.arange(sizes[0]), sizes[0] + np.arange(sizes[1])]
    er = EnergyRanks(m, p, v, 2, None, partition=lambda pp, w: parts, precision=prec)
    try:
        er.forest()
        rows = er.energy_rows()
        er.check()
        assert rows == er.energy_rows()                      # the same bits twice
        for r, (e, row) in enumerate(zip(er.engs, rows)):
            phi = e.let_potential()
            x, u = e.download()
            mm = e.masses()
            assert len(mm) == sizes[r] == row[8] and np.isfinite(phi).all()
            tt = R.terms(mm, x, u, phi)
            conditioned(tt, full=(r == 0))                   # (300 bodies: sum |m x| is too small for the position bound)
            R.check_sums(row, tt, sizes[r], f"{prec.name} rank {r}")
    finally:
        er.close()


# ---- time-step argmax --------------------------------------------------------------------------------------------------------
def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def light_bodies(n, seed=4):
    """n light bodies, uniform in [-0.1, 0.1]^2: masses around 1e-6, velocities of 1e-4."""
    r = np.random.default_rng(seed)
    return r.uniform(0.5, 1.5, n) * 1e-6, r.uniform(-0.1, 0.1, (n, 2)), r.uniform(-1e-4, 1e-4, (n, 2))


def workgroup(i):
    return (i % R.STRIDE) // 256


def ts_engine(n, prec, **kw):
    if prec in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    else:
        kw.setdefault("max_depth", 16)
    return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec, G=1.0, **kw))


def forces_only(e):
    e._check(e._lib.bh_compute_forces(e._h))


@pytest.mark.parametrize("j", [0, 65535, 65536, 65536 + 255, N2 - 1])
@pytest.mark.parametrize("prec", PRECISIONS, ids=IDS)
def test_timestep_argmax_beyond_one_trip(monkeypatch, prec, j):
    """Body j sits alone at (0.2, 0.2) with a body of mass 1 at 1e-4 from it: |a_j| ~ 1e8, a hundred times anybody else's."""
    monkeypatch.setenv("BH_REORDER_EVERY", "1")
    n = N2
    m, p, v = light_bodies(n)
    heavy = (j + 32768) % n
    assert workgroup(heavy) != workgroup(j)
    p[j] = (0.2, 0.2)
    p[heavy] = (0.2001, 0.2)
    m[heavy] = 1.0
    if prec == P.F32:
        m, p, v = _f32(m), _f32(p), _f32(v)
    with ts_engine(n, prec, dt=1e-12) as e:
        e.upload(p, v, m)
        if prec in (P.F32, P.MIXED):
            e.step(1)                                         # device slots are no caller indices from here on
        forces_only(e)
        a = e.accelerations()
        a2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        assert np.isfinite(a2).all()
        top = np.sort(a2)[-2:]
        assert int(np.argmax(a2)) == j and top[1] - top[0] > 1e-12 * top[1]
        a_max = np.sqrt(a2[j])
        t = e.timestep(ETA, LENGTH)
        print(f"{prec.name} j {j}: dt {t.dt!r}, a_max {t.a_max!r}, worst {t.worst}; second largest a2 / largest {top[0] / top[1]:.3g}")
        assert t.worst == j and t.n_bodies == n
        assert abs(t.a_max - a_max) <= 4 * np.spacing(a_max)
        dt = ETA * np.sqrt(LENGTH / a_max)
        assert abs(t.dt - dt) <= 4 * np.spacing(dt)
        assert e.timestep(ETA, LENGTH) == t                  # the same bits twice


TIES = {
    "trip0-wg200_trip1-wg0": (51205, 65541),
    "one-thread-trips-1-and-2": (5 + 65536, 5 + 131072),
    "one-workgroup-two-waves": (7, 200),
}


@pytest.mark.parametrize("layout", list(TIES))
def test_timestep_ties_across_trips_and_workgroups(layout):
    """Two pairs of exactly coincident bodies (equal masses 2^-20, so the cell they share has its centre of mass exactly
    on them): four accelerations are not finite, four records carry +inf, and the smallest caller index has to win
    whichever trip, workgroup or wave holds it.  F64 (F64_EXACT runs the same timestep_partial_kernel<double2>)."""
    n = N2
    lo, other = TIES[layout]
    partners = (100000, 120000)                              # each above both, in workgroups of their own
    four = sorted((lo, other) + partners)
    assert four[0] == lo and len({workgroup(i) for i in partners} | {workgroup(lo), workgroup(other)}) >= 3
    m, p, v = light_bodies(n, seed=6)
    p[partners[0]] = p[lo]
    p[partners[1]] = p[other]
    m[four] = 2.0 ** -20
    with ts_engine(n, P.F64) as e:
        e.upload(p, v, m)
        forces_only(e)
        a = e.accelerations()
        bad = np.flatnonzero(~np.isfinite(a).all(axis=1))
        assert bad.tolist() == four, bad
        t = e.timestep(ETA, LENGTH)
        print(f"{layout}: worst {t.worst}, a_max {t.a_max}, dt {t.dt}")
        assert t.worst == lo and t.a_max == math.inf and t.dt == 0.0 and t.n_bodies == n
        assert e.timestep(ETA, LENGTH) == t
