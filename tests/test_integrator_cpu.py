"""The exact twin of the walk epilogues (tests/integrator_ref.py) checked on its own: the fused multiply-adds against
hand-built witnesses of double rounding and against an independent error-free formulation, the unfused kind against the
oracle's integrator, and the teeth of the fixture that tests/test_gpu_integrator.py runs on the device -- on it a
fused and an unfused fp32 epilogue, and an fp64 epilogue with dt and with float32(dt), must be told apart."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import bh_oracle as O
import integrator_ref as R


def one32(a, b, c):
    return float(R.fma32(a, b, c))


def one64(a, b, c):
    return float(R.fma64(a, b, c))


# ---- witnesses -------------------------------------------------------------------------------------------------------
def test_fma32_double_rounding_witness():
    # (1 + 2^-11)(1 - 2^-11 + 2^-22) = 1 + 2^-33, so a * b + 1 = 1 + 2^-24 + 2^-57: just ABOVE the midpoint of 1 and
    # 1 + 2^-23.  Rounded to fp64 first it IS the midpoint (2^-57 is below half of fp64's last place at 1), and the tie then
    # goes to even: 1.  One rounding gives 1 + 2^-23.
    a, b, c = np.float32(2.0 ** -24 * (1 + 2.0 ** -11)), np.float32(1 - 2.0 ** -11 + 2.0 ** -22), np.float32(1.0)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert exact == 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 57)
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(c))) == 1.0
    assert one32(a, b, c) == 1.0 + 2.0 ** -23
    # (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46: a * b + (1 + 2^-23) lies 2^-70 BELOW the midpoint of 1 + 2^-23 and 1 + 2^-22, and
    # the tie that fp64 makes of it goes up to the even neighbour
    a, b, c = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert exact == 1 + Fraction(3, 2 ** 24) - Fraction(1, 2 ** 70)
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(c))) == 1.0 + 2.0 ** -22
    assert one32(a, b, c) == 1.0 + 2.0 ** -23
    assert one32(-a, b, -c) == -(1.0 + 2.0 ** -23)


def test_fma64_double_rounding_witness():
    # the fp64 analogue: (1 + 2^-26)(1 - 2^-26 + 2^-52) = 1 + 2^-78, exact = 1 + 2^-53 + 2^-131, above the midpoint of 1 and
    # 1 + 2^-52; the rounded product is 2^-53 and the sum a tie
    a, b, c = 2.0 ** -53 * (1 + 2.0 ** -26), 1 - 2.0 ** -26 + 2.0 ** -52, 1.0
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    assert exact == 1 + Fraction(1, 2 ** 53) + Fraction(1, 2 ** 131)
    assert one64(a, b, c) == 1.0 + 2.0 ** -52
    assert a * b + c == 1.0                                  # two roundings in fp64: the product, then a tie to even
    if np.finfo(np.longdouble).nmant >= 63:                  # extended or quad precision: 79 bits do not fit either
        assert float(np.longdouble(a) * np.longdouble(b) + np.longdouble(c)) == (1.0 if np.finfo(np.longdouble).nmant < 78 else 1.0 + 2.0 ** -52)
    # and a product whose low half survives a cancellation: (1 + 2^-52)^2 - 1 = 2^-51 + 2^-104 exactly
    x = 1.0 + 2.0 ** -52
    assert one64(x, x, -1.0) == 2.0 ** -51 + 2.0 ** -104
    assert x * x - 1.0 == 2.0 ** -51
    if np.finfo(np.longdouble).nmant == 63:                  # the platform's long double shows the difference
        assert float(np.longdouble(x) * np.longdouble(x) - np.longdouble(1.0)) == 2.0 ** -51


def test_exact_cancellations():
    assert one32(np.float32(3.0), np.float32(5.0), np.float32(-15.0)) == 0.0
    assert one64(0.1, 10.0, -1.0) == float(Fraction(0.1) * 10 - 1)          # 2^-54: the rounding error of 0.1, recovered
    assert one64(0.1, 10.0, -1.0) == 2.0 ** -54
    x = np.float32(1.0 + 2.0 ** -23)
    assert one32(x, x, -x) == float(Fraction(float(x)) ** 2 - Fraction(float(x)))   # exactly representable
    assert one64(1e300, 0.0, 0.0) == 0.0 and one64(0.0, 5.0, 7.5) == 7.5


def test_subnormal_and_overflowing_results():
    tiny32 = 2.0 ** -149
    assert one32(np.float32(2.0 ** -100), np.float32(2.0 ** -49), 0.0) == tiny32
    assert one32(np.float32(2.0 ** -100), np.float32(2.0 ** -50), 0.0) == 0.0            # half of the smallest: tie to even
    assert one32(np.float32(2.0 ** -100), np.float32(1.5 * 2.0 ** -50), 0.0) == tiny32   # three quarters: up
    assert one32(np.float32(2.0 ** -100), np.float32(1.5 * 2.0 ** -49), 0.0) == 2 * tiny32   # 1.5 quanta: tie to even (2)
    assert one32(np.float32(3.0), np.float32(2.0 ** -149), np.float32(2.0 ** -149)) == 4 * tiny32
    # subnormal kept through an a = 0 kick (the n = 1 case of the device test)
    sub = float(np.float32(1e-42))
    assert sub != 0.0 and sub < 2.0 ** -126
    assert one32(0.0, np.float32(0.01), np.float32(1e-42)) == sub
    # a result in the subnormal range loses precision where a normal one would not
    assert one32(np.float32(1.0 + 2.0 ** -23), np.float32(2.0 ** -127), 0.0) == 2.0 ** -127
    tiny64 = 5e-324
    assert one64(2.0 ** -1000, 2.0 ** -74, 0.0) == tiny64 and one64(2.0 ** -1000, 2.0 ** -75, 0.0) == 0.0
    assert one64(2.0 ** -1000, 2.0 ** -75, tiny64) == 2 * tiny64                          # 1.5 quanta: tie to even
    big32 = float(np.finfo(np.float32).max)
    assert one32(np.float32(big32), np.float32(2.0), 0.0) == math.inf
    assert one32(np.float32(big32), np.float32(1.0), np.float32(2.0 ** 102)) == big32     # below half a quantum: stays
    assert one32(np.float32(big32), np.float32(1.0), np.float32(2.0 ** 103)) == math.inf  # the tie rounds up and out
    assert one32(np.float32(-big32), np.float32(2.0), np.float32(big32)) == -big32        # finite although a*b is not
    big64 = float(np.finfo(np.float64).max)
    assert one64(big64, 2.0, 0.0) == math.inf and one64(big64, 2.0, -big64) == big64
    assert one64(-big64, 1.0, -2.0 ** 970) == -math.inf and one64(big64, 1.0, 2.0 ** 969) == big64


# ---- an independent formulation ----------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """Dekker / Veltkamp: a * b = p + e exactly, in fp64 without an fma."""
    p = a * b
    split = 134217729.0                                     # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(hi, lo):
    """fl_odd(hi + lo): the fp64 sum with its last bit made sticky (Boldo-Melquiond)."""
    s, e = _two_sum(hi, lo)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    up = (e > 0) == (s > 0)                                 # the exact sum lies further from zero than s
    return (bits + np.where(fix, np.where(up, 1, -1), 0)).view(np.float64)


def test_fma32_against_an_exact_fp64_product():
    """For fp32 inputs a * b is exact in fp64 (48 bits), so a*b + c is one TwoSum away from exact; rounding that sum to odd
    in fp64 and then to fp32 is a single rounding (53 >= 2 * 24 + 2)."""
    rng = np.random.default_rng(3)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 2.0 ** rng.integers(-30, 2, n))).astype(np.float32)
    c[::7] = (rng.standard_normal(len(c[::7])) * 2.0 ** rng.integers(-40, 40, len(c[::7]))).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)
    want = _round_to_odd_sum(prod, c.astype(np.float64)).astype(np.float32)
    got = R.fma32(a, b, c)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_fma64_against_two_product_two_sum():
    """Boldo-Melquiond: with a*b = ph + pl (TwoProduct) and ph + c = sh + sl (TwoSum), fma = fl(sh + fl_odd(sl + pl)).
    Inputs are scaled away from underflow and overflow, where the error-free transformations hold."""
    rng = np.random.default_rng(4)
    n = 4000
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)
    b = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)
    c = -(a * b) * (1 + rng.standard_normal(n) * 2.0 ** rng.integers(-60, 2, n))
    c[::7] = rng.standard_normal(len(c[::7])) * 2.0 ** rng.integers(-60, 60, len(c[::7]))
    ph, pl = _two_prod(a, b)
    sh, sl = _two_sum(ph, c)
    want = sh + _round_to_odd_sum(sl, pl)
    got = R.fma64(a, b, c)
    assert np.array_equal(got, want)
    assert (got != a * b + c).mean() > 0.05                 # the unfused expression is something else on this input
    for i in range(0, n, 40):                               # and both are the rational result, rounded by Python's own division
        assert got[i] == float(Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i]))


# ---- the kinds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1.0, 0.01, 2.5e-3])
def test_exact_kind_is_the_oracles_integrator(dt):
    rng = np.random.default_rng(5)
    n = 3000
    f = rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-12, 3, (n, 2))
    m = rng.uniform(0.1, 0.5, n)
    v = rng.uniform(-1e-4, 1e-4, (n, 2))
    p = rng.uniform(-0.1, 0.1, (n, 2))
    acc, vo, po = O.integrate(f, m, v, p, dt=dt)
    a = R.accel_exact(f, m)
    vn, pn = R.kick_drift(a, v, p, dt, "exact")
    assert np.array_equal(a, acc) and np.array_equal(vn, vo) and np.array_equal(pn, po)
    vf, pf = R.kick_drift(a, v, p, dt, "f64")
    if dt != 1.0:
        assert not np.array_equal(vf, vo)                   # (the fused kind is a different function)


def test_kinds_take_the_stated_types():
    a = np.array([[0.1, 0.2]])
    with pytest.raises(ValueError):
        R.kick_drift(a, a, a, 0.01, "mixed")                # 0.1 is no fp32 value
    with pytest.raises(ValueError):
        R.kick_drift(a, a, a, 0.01, "leapfrog")
    a32 = R.to_f32(a)
    vn, pn = R.kick_drift(a32, a32, a32, 0.01, "f32")
    assert np.array_equal(vn, R.to_f32(vn)) and np.array_equal(pn, R.to_f32(pn))
    vm, _ = R.kick_drift(a32, a, a, 0.01, "mixed")
    assert vm[0, 0] == float(Fraction(float(a32[0, 0])) * Fraction(0.01) + Fraction(0.1))


# ---- teeth: the device test's fixture tells the wrong epilogues from the right one ---------------------------------------
def _oracle_accel(m, p):
    t = O.build_tree(p, m, 0)
    return O.compute_forces(t, p, m, G=R.FIX_G, compat_self_skip=False) / m[:, None]


@pytest.fixture(scope="module")
def fixture1000():
    m, p, v = R.make_fixture(1000)
    return m, p, v


def test_fixture_is_what_the_issue_describes(fixture1000):
    m, p, v = fixture1000
    n = len(m)
    assert float(np.float32(R.FIX_DT)) != R.FIX_DT and Fraction(R.FIX_DT) != Fraction(1, 100)
    speed = np.abs(v).max(1)
    assert (speed == 0).sum() >= n // 3 - 1 and ((speed > 0) & (speed < 1e-29)).sum() >= n // 3 - 1
    assert (speed > 1e-6).sum() >= 0.3 * n
    assert (np.abs(p) <= 0.1).all() and np.isfinite(p).all()
    assert len(np.unique(p, axis=0)) == n and len(np.unique(R.to_f32(p), axis=0)) == n      # no coincident bodies
    adt = np.linalg.norm(_oracle_accel(m, p), axis=1) * R.FIX_DT
    fast = speed > 1e-6
    ratio = adt[fast] / np.linalg.norm(v[fast], axis=1)
    assert 0.1 < np.median(ratio) < 100.0                   # comparable for the fast third ...
    assert (adt[~fast] > 1e20 * np.linalg.norm(v[~fast], axis=1)).all()   # ... and dominant for the rest


def test_fused_fp32_twin_differs_from_the_unfused_one(fixture1000):
    m, p, v = (R.to_f32(x) for x in fixture1000)
    a = R.to_f32(_oracle_accel(m, p))
    vf, pf = R.kick_drift(a, v, p, R.FIX_DT, "f32")
    vu, pu = R.kick_drift_unfused32(a, v, p, R.FIX_DT)
    frac_v, frac_p = (vf != vu).mean(), (pf != pu).mean()
    print(f"fused != unfused: {frac_v:.3f} of the velocity, {frac_p:.3f} of the position components")
    assert max(frac_v, frac_p) >= 0.05
    # and an epilogue that drifts with the OLD velocity, or kicks with another dt, is somebody else entirely
    p_old = R.fma32(v, np.float32(R.FIX_DT), p).astype(np.float64)
    assert (p_old != pf).mean() >= 0.9


def test_fp64_twin_with_dt_differs_from_the_one_with_rounded_dt(fixture1000):
    m, p, v = fixture1000
    p = p * (1.0 + 3e-9 * np.random.default_rng(2).standard_normal(p.shape))
    a64 = _oracle_accel(m, p)
    for kind, a in (("mixed", R.to_f32(a64)), ("f64", a64)):
        vd, pd = R.kick_drift(a, v, p, R.FIX_DT, kind)
        vr, pr = R.kick_drift(a, v, p, float(np.float32(R.FIX_DT)), kind)
        frac = (pd != pr).mean()
        print(f"{kind}: dt != f32(dt) on {frac:.4f} of the position components")
        assert frac >= 0.99
