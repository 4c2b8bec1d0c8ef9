"""An exact twin of the walk epilogues' kick-drift (a = G * sum, v += a dt, p += v dt), in plain Python integers -- a
helper of tests/test_integrator_cpu.py and tests/test_gpu_integrator.py, not a test file.

fma32 / fma64 are correctly rounded fused multiply-adds: the product and the sum are formed exactly on integer
significands and rounded ONCE, to nearest even, into the target format (gradual underflow and overflow included).
Signed zeros are not modelled (every comparison is ==).  kick_drift states, per precision mode, which operations of
the epilogue are fused, which dt and which acceleration enter (DESIGN.md section 2, row "integration")."""
import math

import numpy as np

_F32 = (24, -126, 127)        # significand bits, exponent of the smallest normal, exponent of the largest binade
_F64 = (53, -1022, 1023)


def _split(x):
    """finite float -> (M, E) with x == M * 2**E exactly."""
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def _round_scaled(n, e, fmt):
    """n * 2**e (n any integer), rounded to nearest even into fmt; returned as a Python float (exact for both formats)."""
    prec, emin, emax = fmt
    if n == 0:
        return 0.0
    sign, n = (-1.0, -n) if n < 0 else (1.0, n)
    top = n.bit_length() - 1 + e                 # floor(log2(value))
    q = max(top, emin) - prec + 1                # exponent of the result's last place (subnormals share emin's)
    sh = q - e
    if sh <= 0:
        k = n << -sh
    else:
        k, r = n >> sh, n & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if r > half or (r == half and (k & 1)):
            k += 1
    if k.bit_length() + q > emax + 1:            # (a carry out of the largest binade included)
        return sign * math.inf
    return sign * math.ldexp(float(k), q)


def _fma_scalar(a, b, c, fmt):
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))     # inf / nan: no rounding left to model
    ma, ea = _split(a)
    mb, eb = _split(b)
    mc, ec = _split(c)
    mp, ep = ma * mb, ea + eb
    if mp == 0:
        return _round_scaled(mc, ec, fmt)
    if mc == 0:
        return _round_scaled(mp, ep, fmt)
    e = min(ep, ec)
    return _round_scaled((mp << (ep - e)) + (mc << (ec - e)), e, fmt)


def _fma(a, b, c, fmt, dtype):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(c, dtype=dtype))
    out = np.empty(a.shape, dtype=np.float64)
    fo = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        fo[i] = _fma_scalar(x, y, z, fmt)
    with np.errstate(over="ignore"):
        return out.astype(dtype)                 # exact: every value is already one of dtype's


def fma32(a, b, c):
    """round_fp32(a * b + c), one rounding; arguments are taken as float32, the result is float32."""
    return _fma(a, b, c, _F32, np.float32)


def fma64(a, b, c):
    """round_fp64(a * b + c), one rounding."""
    return _fma(a, b, c, _F64, np.float64)


def accel_exact(forces, mass):
    """updateAccelerations of the reference: a = F / m, one correctly rounded division per component."""
    return np.asarray(forces, dtype=np.float64) / np.asarray(mass, dtype=np.float64)[:, None]


KINDS = ("f32", "mixed", "f64", "exact")


def kick_drift(a, v, p, dt, kind):
    """(v', p') as float64 arrays, of one epilogue with the accelerations a (shape (n, 2)) it used.

    "f32":   v' = fma32(a, f32(dt), v), p' = fma32(v', f32(dt), p); a, v, p are fp32 values.
    "mixed": v' = fma64(f64(a32), dt, v), p' = fma64(v', dt, p): the fp32 acceleration widened, the fp64 dt.
    "f64":   the same from an fp64 a (= G * sum).
    "exact": unfused, the reference's order: a = F / m (accel_exact), v += a * dt, p += v * dt."""
    dt = float(dt)
    if kind == "f32":
        a, v, p = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (a, v, p))
        d = np.float32(dt)
        vn = fma32(a, d, v)
        return vn.astype(np.float64), fma32(vn, d, p).astype(np.float64)
    a, v, p = (np.asarray(x, dtype=np.float64) for x in (a, v, p))
    if kind == "mixed":
        a32 = a.astype(np.float32).astype(np.float64)
        if not np.array_equal(a32, a, equal_nan=True):
            raise ValueError("mixed: the acceleration must be an fp32 value")
        vn = fma64(a32, dt, v)
        return vn, fma64(vn, dt, p)
    if kind == "f64":
        vn = fma64(a, dt, v)
        return vn, fma64(vn, dt, p)
    if kind == "exact":
        vn = v + a * dt
        return vn, p + vn * dt
    raise ValueError(f"kind must be one of {KINDS}")


def kick_drift_unfused32(a, v, p, dt):
    """What "f32" must NOT be: the product rounded before the sum (v + f32(a * dt)).  For the teeth checks only."""
    a, v, p = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (a, v, p))
    d = np.float32(dt)
    vn = v + a * d
    return vn.astype(np.float64), (p + vn * d).astype(np.float64)


# ---- the fixture of the integrator tests ---------------------------------------------------------------------------
FIX_G, FIX_DT = 1.0, 0.01          # dt = 0.01 is representable neither in fp32 nor in fp64


def make_fixture(n, seed=0, masses="scaled"):
    """(m, p, v) in fp64: a third of the bodies in a tight Gaussian clump, the rest uniform in [-0.1, 0.1]^2; velocities
    of 1e-4, of 1e-30 and exact zeros by thirds; masses such that, with G = 1 and dt = 0.01, a dt is comparable with |v|
    for the fast third (total mass 1e-4 at distances ~0.1: a ~ 1e-2) and dominates for the rest.
    masses="pow2": 2**k, k in [-12, -6) -- (G m) * sum / m is then exactly G * sum."""
    rng = np.random.default_rng(1000 + seed)
    nc = n // 3
    p = np.concatenate([rng.normal(0.0, 5e-3, (nc, 2)) + np.array([0.03, -0.02]), rng.uniform(-0.1, 0.1, (n - nc, 2))])
    p = p[rng.permutation(n)]
    v = rng.uniform(-1e-4, 1e-4, (n, 2))
    third = rng.permutation(n) % 3
    v[third == 1] *= 1e-26                       # ~1e-30
    v[third == 2] = 0.0
    if masses == "pow2":
        m = 2.0 ** rng.integers(-12, -6, n)
    else:
        m = rng.uniform(0.5, 1.5, n) * (1e-4 / n)
    return m, p, v


def to_f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
