"""An exact twin of the split operators bh_kick and bh_drift (csrc/bh_split.hpp), on the correctly rounded fma32 / fma64 of
tests/integrator_ref.py -- a helper of tests/test_split_cpu.py and tests/test_gpu_split.py, not a test file.

kick(a, v, h, kind) and drift(v, p, h, kind) are the two halves of integrator_ref.kick_drift: drift(kick(...)) with the
same h IS that function, bit for bit, for every kind (tests/test_split_cpu.py).  Per kind:

    "f32":   v' = fma32(a, f32(h), v),        p' = fma32(v, f32(h), p); a, v, p are fp32 values.
    "mixed": v' = fma64(f64(a32), h, v),      p' = fma64(v, h, p): the fp32 acceleration widened, the fp64 h unrounded.
    "f64":   v' = fma64(a, h, v),             p' = fma64(v, h, p), a = forces / masses (one IEEE division).
    "exact": v' = v + a * h,                  p' = p + v * h, unfused, a = forces / masses.

Everything is returned as float64 arrays (exact for the fp32 kinds)."""
import numpy as np

import integrator_ref as R

KINDS = R.KINDS


def kick(a, v, h, kind):
    h = float(h)
    if kind == "f32":
        a, v = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (a, v))
        return R.fma32(a, np.float32(h), v).astype(np.float64)
    a, v = (np.asarray(x, dtype=np.float64) for x in (a, v))
    if kind == "mixed":
        a32 = a.astype(np.float32).astype(np.float64)
        if not np.array_equal(a32, a, equal_nan=True):
            raise ValueError("mixed: the acceleration must be an fp32 value")
        return R.fma64(a32, h, v)
    if kind == "f64":
        return R.fma64(a, h, v)
    if kind == "exact":
        return v + a * h
    raise ValueError(f"kind must be one of {KINDS}")


def drift(v, p, h, kind):
    h = float(h)
    if kind == "f32":
        v, p = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (v, p))
        return R.fma32(v, np.float32(h), p).astype(np.float64)
    v, p = (np.asarray(x, dtype=np.float64) for x in (v, p))
    if kind in ("mixed", "f64"):
        return R.fma64(v, h, p)
    if kind == "exact":
        return p + v * h
    raise ValueError(f"kind must be one of {KINDS}")


# ---- what the kinds must NOT be: for the teeth checks only ---------------------------------------------------------------
def kick_mixed_rounded_h(a, v, h):
    """A mixed kick fed (float)h."""
    return kick(a, v, float(np.float32(h)), "mixed")


def kick_unfused32(a, v, h):
    """An fp32 kick with the product rounded before the sum."""
    a, v = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (a, v))
    return (v + a * np.float32(h)).astype(np.float64)


# ---- the two-body problems of the convergence and adaptive tests ------------------------------------------------------------
def pair(e=0.5):
    """(m, p, v): G = 1, two unit masses at separation 1, at the apocentre of an orbit of eccentricity e about the origin
    (relative speed sqrt(2 (1 - e)); e = 0.5: speeds of sqrt(0.5) * sqrt(0.5) = 0.5 each)."""
    s = 0.5 * np.sqrt(2.0 * (1.0 - e))
    return np.array([1.0, 1.0]), np.array([[-0.5, 0.0], [0.5, 0.0]]), np.array([[0.0, -s], [0.0, s]])


def pair_accel(m, p, eps=0.0):
    """Direct two-body accelerations, G = 1, Plummer-softened."""
    d = p[1] - p[0]
    s2 = d @ d + eps * eps
    w = d / (s2 * np.sqrt(s2))
    return np.array([m[1] * w, -m[0] * w])


def pair_energy(m, p, v):
    d = p[1] - p[0]
    return 0.5 * float((m[:, None] * v * v).sum()) - m[0] * m[1] / float(np.sqrt(d @ d))


def pair_energy_error(e, dt, t_end, scheme):
    """max |E - E0| / |E0| over the steps of a fixed-step fp64 run of the pair: scheme "euler" (the fused kick-drift) or
    "kdk"."""
    m, p, v = pair(e)
    e0 = pair_energy(m, p, v)
    worst = 0.0
    for _ in range(int(round(t_end / dt))):
        if scheme == "euler":
            v = v + pair_accel(m, p) * dt
            p = p + v * dt
        else:
            v = v + pair_accel(m, p) * (0.5 * dt)
            p = p + v * dt
            v = v + pair_accel(m, p) * (0.5 * dt)
        worst = max(worst, abs(pair_energy(m, p, v) - e0) / abs(e0))
    return worst


def pair_adaptive(e, eta, length, t_end, dt_max=None, t=0.0):
    """BarnesHutEngine.step_adaptive's loop on the direct two-body force, in fp64: (t, steps, p, v, dts, clips), clips the
    values every dt was compared against ((dt_max,) t_end - t) -- for the caller's margin check."""
    m, p, v = pair(e)
    steps, dts, clips = 0, [], []
    a = pair_accel(m, p)
    while t < t_end:
        a_max = np.sqrt((a * a).sum(axis=1).max())
        crit = eta * np.sqrt(length / a_max)
        dt = crit if dt_max is None else min(crit, dt_max)
        dts.append(crit)
        clips.append(([] if dt_max is None else [dt_max]) + [t_end - t])
        last = not (dt < t_end - t)
        if last:
            dt = t_end - t
        v = v + a * (0.5 * dt)
        p = p + v * dt
        a = pair_accel(m, p)
        v = v + a * (0.5 * dt)
        t = t_end if last else t + dt
        steps += 1
    return t, steps, p, v, np.array(dts), clips
