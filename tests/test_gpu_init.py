"""init_bodies_kernel (csrc/bh_init.hpp) against its numpy twin (tests/init_ref.py), body by body, in all four precisions.

Bitwise (np.array_equal on the raw arrays): the raw 53-bit uniforms of the five streams (a 0..1 range hands them back), every
linear range (bh_engine.hip is built with -ffp-contract=off: u * (upper - lower) + lower is two IEEE roundings), Plummer
masses and velocities, prefix and capacity independence, and initialize == upload of the same values.
Toleranced, against the extended-precision twin: the log-uniform rule and the Plummer positions, which go through the
device's libm.  The two constants LOG_UNITS and PLUMMER_K are 4 x the worst value measured on the device (DESIGN.md section
29); an fp32 state is bracketed: float32(twin - tol) <= device <= float32(twin + tol)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_STATS  # noqa: E402
import init_ref as R  # noqa: E402

LD = np.longdouble
P = G.Precision
PLUMMER_CASES = R.PLUMMER_CASES
PRECISIONS = [P.F64_EXACT, P.F64, P.MIXED, P.F32]
CAP = 4352                                    # 17 workgroups of kBlock = 256
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099]     # empty launch, one lane, wave edges, workgroup edges, a tail
SEEDS = [0, 7, 7 + (1 << 32), (1 << 63) + 7, (1 << 64) - 1]
U = 2.0 ** -53

# 4 x the worst value measured on the device against the extended-precision twin (the three fp64-state
# precisions; log-uniform: LOG_RANGES at n = 4,099, seeds 0, 7, 2^63 + 7; Plummer: PLUMMER_CASES with seeds 1, 2, 3).  Four is
# for other seeds, not for slack.
LOG_UNITS = 4 * 1.30         # relative error of a log-uniform value in units of 2^-53 (1 + ln 10 max |log10 bound|)
PLUMMER_K = 4 * 4.52         # |dx|, |dy| in units of 2^-53 rad (8 + p / (p - 1)).  4.52 is ONE body (seed 1, hp = 0.006, body
                             # 342) that sits 1 - cz^2 = 1.2e-6 from the pole, where the rounding of cz * cz is amplified by
                             # 1 / (4 sqrt(1 - cz^2)); the worst of every other body is 1.02

OUTSIDE_PROJECTED = 206      # of the 218 exhausted bodies of the hp = 0.006 case, those whose projection is beyond hp too
LOG_RANGES = [(0.1, 0.5), (1e-16, 1e-14), (1.0, 1.0)]


def engine(precision, capacity=CAP, **kw):
    return G.BarnesHutEngine(G.BhConfig(capacity=capacity, precision=precision, **kw))


def state(e):
    p, v = e.download()
    return e.masses(), p, v


def device_box(e, n, seed, *ranges):
    e.initialize(n, seed, "box", *ranges)
    return state(e)


def device_plummer(e, n, seed, a, hp, m):
    e.initialize(n, seed, "plummer", higher_m=m, lower_p=a, higher_p=hp)
    return state(e)


def log_unit(lower, upper):
    return U * (1.0 + math.log(10.0) * max(abs(math.log10(lower)), abs(math.log10(upper))))


def log_error_units(dev, twin, lower, upper):
    """Worst relative error of fp64 device values against the extended twin, in log_unit."""
    return float(np.max(np.abs(dev.astype(LD) - twin) / np.abs(twin))) / log_unit(lower, upper) if len(dev) else 0.0


def plummer_unit(rad, p):
    return LD(U) * rad * (LD(8) + p / (p - LD(1)))


def plummer_error_units(dev_pos, twin_pos, rad, p):
    return float(np.max(np.abs(dev_pos.astype(LD) - twin_pos) / plummer_unit(rad, p)[:, None])) if len(dev_pos) else 0.0


def assert_within(dev, twin, tol, precision, what):
    """fp64 state: |dev - twin| <= tol.  F32 state: the rounding is exact given that bound."""
    twin, tol = np.asarray(twin, dtype=LD), np.asarray(tol, dtype=LD)
    if precision == P.F32:
        lo, hi = (twin - tol).astype(np.float32).astype(np.float64), (twin + tol).astype(np.float32).astype(np.float64)
        bad = (dev < lo) | (dev > hi)
    else:
        bad = np.abs(dev.astype(LD) - twin) > tol
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- raw uniforms
@pytest.mark.parametrize("precision", PRECISIONS)
def test_raw_uniforms_bitwise(precision):
    """lower = 0, upper = 1 is the linear rule and returns u itself: the five streams' 53-bit uniforms, every launch edge,
    seeds that use the high word."""
    seen = {}
    with engine(precision) as e:
        for seed in SEEDS:
            want = R.uniforms(SIZES[-1], seed)
            for n in SIZES:
                m, p, v = device_box(e, n, seed, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
                got = np.column_stack([m, p, v]) if n else np.zeros((0, 5))
                assert m.shape == (n,) and p.shape == (n, 2) and v.shape == (n, 2)
                assert np.array_equal(got, R.to_state(want[:n], precision)), (seed, n)
            seen[seed] = got
    for a in SEEDS:
        for b in SEEDS:
            if a < b:
                for j in range(5):
                    assert not np.array_equal(seen[a][:, j], seen[b][:, j]), (a, b, j)
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(seen[7][:, a], seen[7][:, b]), (a, b)


# ---- linear ranges
LINEAR = [(-0.1, 0.1, -1e-4, 1e-4),            # the reference's position and velocity ranges
          (-3.0, 1e-3, -3.0, 1e-3),            # straddling zero asymmetrically
          (0.25, 0.25, -2.0, -2.0),            # lower == upper (the first pair positive: the log rule of one point)
          (0.5, -0.5, 1e-4, -1e-4),            # lower > upper
          (0.0, 2.5, 0.0, 1e-4)]               # lower = 0: linear by the rule, not log


@pytest.mark.parametrize("precision", PRECISIONS)
def test_linear_ranges_bitwise(precision):
    n = 1000
    with engine(precision) as e:
        for seed in (7, (1 << 63) + 7):
            for lp, hp, lv, hv in LINEAR:
                # masses through the linear rule as well: a bound <= 0
                m, p, v = device_box(e, n, seed, -0.5, 0.5, lp, hp, lv, hv)
                tm, tp, tv = R.box_exact(n, seed, -0.5, 0.5, lp, hp, lv, hv)
                assert tm.dtype == np.float64 and tv.dtype == np.float64
                assert np.array_equal(m, R.to_state(tm, precision)), (seed, lp, hp)
                assert np.array_equal(v, R.to_state(tv, precision)), (seed, lv, hv)
                if R.is_log(lp, hp):
                    assert lp == hp
                    assert_within(p, tp, np.abs(tp) * LD(LOG_UNITS * log_unit(lp, hp)), precision, (seed, lp, hp))
                else:
                    assert tp.dtype == np.float64 and np.array_equal(p, R.to_state(tp, precision)), (seed, lp, hp)


# ---- log-uniform masses
@pytest.mark.parametrize("precision", PRECISIONS)
def test_log_uniform_masses(precision):
    n = 4099
    worst = 0.0
    with engine(precision) as e:
        for lower, upper in LOG_RANGES:
            for seed in (0, 7, (1 << 63) + 7):
                m, p, v = device_box(e, n, seed, lower, upper, -0.1, 0.1, -1e-4, 1e-4)
                tm, tp, tv = R.box_exact(n, seed, lower, upper, -0.1, 0.1, -1e-4, 1e-4)
                assert tm.dtype == LD
                if precision != P.F32:
                    worst = max(worst, log_error_units(m, tm, lower, upper))
                assert_within(m, tm, tm * LD(LOG_UNITS * log_unit(lower, upper)), precision, (lower, upper, seed))
                assert np.array_equal(p, R.to_state(tp, precision)) and np.array_equal(v, R.to_state(tv, precision))
                if lower == upper:
                    assert np.all(np.abs(m - 1.0) <= LOG_UNITS * log_unit(1.0, 1.0))
    print("log-uniform: worst error %.3f units (%s)" % (worst, precision.name))


# ---- Plummer
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", PLUMMER_CASES, ids=lambda c: "hp%g" % c[3])
def test_plummer_against_the_twin(precision, case):
    seed, n, a, hp = case
    mass = 1e-8 / n
    tm, tp, tv, tries, rad, p, gap = R.plummer_exact(n, seed, a, hp, mass)
    assert float(gap.min()) > 1e-6                       # test_init_cpu.py: no rejection can fall the other way
    with engine(precision, max_depth=21, reference_compat=False) as e:
        m, pos, vel = device_plummer(e, n, seed, a, hp, mass)
    assert np.array_equal(m, R.to_state(tm, precision))
    assert np.array_equal(vel, np.zeros((n, 2))) and not np.signbit(vel).any()
    if precision != P.F32:
        print("plummer hp = %g: worst error %.3f units (%s)" % (hp, plummer_error_units(pos, tp, rad, p), precision.name))
    assert_within(pos, tp, (PLUMMER_K * plummer_unit(rad, p))[:, None], precision, case)
    # from the device arrays alone: a body beyond hp is one whose 64 draws were all rejected.  The arrays hold the PROJECTED
    # position, so the bodies seen beyond hp are those of the exhausted set whose projection lies beyond it too.
    ex = R.exhausted(tries, rad, hp)
    rt = np.hypot(tp[:, 0], tp[:, 1])
    assert float(np.abs(rt / LD(hp) - 1).min()) > 1e-6   # and no projected radius sits on the edge
    outside = np.hypot(pos[:, 0], pos[:, 1]) > hp
    assert np.array_equal(outside, np.asarray(rt > hp)) and not (outside & ~ex).any()
    assert outside.sum() == {0.2: 0, 0.02: 0, 0.006: OUTSIDE_PROJECTED}[hp]


# ---- prefix and capacity independence
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["box", "plummer"])
def test_a_body_is_a_function_of_seed_and_index(precision, kind):
    """initialize(257) == the first 257 bodies of initialize(1000) and of initialize(4099), on any engine capacity."""
    args = dict(box={}, plummer=dict(higher_m=1e-9, lower_p=0.02, higher_p=0.02))[kind]
    seed = (1 << 63) + 7

    def run(e, n):
        e.initialize(n, seed, kind, **args)
        return state(e)

    with engine(precision) as e:
        a4099, a1000, a257 = run(e, 4099), run(e, 1000), run(e, 257)
    with engine(precision, capacity=257) as e:
        small = run(e, 257)
    for other in (a1000, a4099, small):
        for x, y in zip(a257, other):
            assert x.shape[0] == 257 and np.array_equal(x, y[:257])
    assert len(np.unique(a257[1][:, 0])) > 250


# ---- initialize is an upload
@pytest.mark.parametrize("precision", [P.F64_EXACT, P.F32])
def test_initialize_is_an_upload(precision):
    """Engine A has run 40 steps of another system of 4,099 bodies (an fp32 state physically re-ordered; tree, forces and the
    direct-sort record stale) before initialize; engine B is fresh and uploads what A hands back.  Everything either then
    computes is bitwise equal."""
    n = 1000
    flags = FLAG_WALK_STATS if precision != P.F64_EXACT else 0
    r = np.random.default_rng(5)
    m0, p0, v0 = 10.0 ** r.uniform(-2, 0, 4099), r.uniform(-0.3, 0.2, (4099, 2)), r.uniform(-1e-4, 1e-4, (4099, 2))
    with engine(precision, max_depth=21, flags=flags) as A, engine(precision, max_depth=21, flags=flags) as B:
        A.upload(p0, v0, m0)
        A.step(40)
        A.sync()
        A.initialize(n, seed=7)
        m, p, v = state(A)
        tm, tp, tv = R.box(n, 7)
        assert np.array_equal(p, R.to_state(tp, precision)) and np.array_equal(v, R.to_state(tv, precision))
        B.upload(p, v, m)
        for x, y in zip(state(A), state(B)):
            assert np.array_equal(x, y)
        fa, fb = A.compute_forces(), B.compute_forces()
        assert np.array_equal(fa, fb) and np.isfinite(fa).all() and fa.any()
        if precision == P.F64_EXACT:
            assert A.stats().interactions == B.stats().interactions
        else:
            ca, cb = A.interaction_counts(), B.interaction_counts()
            assert np.array_equal(ca, cb) and ca.min() > 0
            assert np.array_equal(A.ids(), B.ids()) and np.array_equal(np.sort(A.ids()), np.arange(n))
        (na, da), (nb, db) = A.export_tree(), B.export_tree()
        assert len(na) > n and na.tobytes() == nb.tobytes() and np.array_equal(da, db)
        A.step(3)
        B.step(3)
        for x, y in zip(state(A), state(B)):
            assert np.array_equal(x, y)
        assert A.stats().steps_done == B.stats().steps_done == 3


# ---- errors
def test_argument_errors():
    with engine(P.F32, capacity=256) as e:
        with pytest.raises(G.BhError) as ei:
            e.initialize(257, 1)
        assert ei.value.code == -1 and "Requested number of bodies exceeds N_BODIES." in str(ei.value)
        with pytest.raises(G.BhError) as ei:
            e._check(e._lib.bh_initialize(e._h, 16, 1, 2, 0.1, 0.5, -0.1, 0.1, -1e-4, 1e-4))
        assert ei.value.code == -1 and "kind" in str(ei.value)
        e.initialize(0, 1)
        m, p, v = state(e)
        assert m.shape == (0,) and p.shape == (0, 2) and v.shape == (0, 2)
        e.initialize(0, 1, "plummer", higher_m=1.0, lower_p=0.02, higher_p=0.2)
        assert e.masses().shape == (0,)
        nan, inf = float("nan"), float("inf")
        bad = [dict(lower_p=0.0), dict(lower_p=-0.02), dict(lower_p=nan), dict(lower_p=inf),
               dict(higher_p=0.0), dict(higher_p=-0.2), dict(higher_p=nan), dict(higher_p=-inf),
               dict(higher_m=nan), dict(higher_m=inf), dict(higher_m=-inf)]
        for kw in bad:
            args = dict(higher_m=1e-9, lower_p=0.02, higher_p=0.2)
            args.update(kw)
            with pytest.raises(G.BhError) as ei:
                e.initialize(16, 1, "plummer", **args)
            assert ei.value.code == -1 and "plummer" in str(ei.value) and next(iter(kw)) in str(ei.value), kw
        # a refused call changes nothing: the empty set of before is still there
        assert e.masses().shape == (0,)
        # kind 0 stays as permissive as the reference; lower_m is ignored by kind 1; +inf is no truncation
        e.initialize(16, 1, "box", -1.0, 0.0, 5.0, -5.0, 0.0, 0.0)
        e.initialize(256, 1, "plummer", lower_m=nan, higher_m=0.0, lower_p=0.02, higher_p=inf)
        m, p, v = state(e)
        tm, tp, tv, tries, rad, pp, gap = R.plummer_exact(256, 1, 0.02, inf, 0.0)
        assert (tries == 1).all() and np.isfinite(p).all() and not m.any()
        assert_within(p, tp, (PLUMMER_K * plummer_unit(rad, pp))[:, None], P.F32, "untruncated")
        assert np.hypot(p[:, 0], p[:, 1]).max() > 0.2
