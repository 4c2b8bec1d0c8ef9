"""The numpy twin of csrc/bh_disc.hpp (include/bhgpu.h, "a disc"): vectorised fp64 in the stated operation order on the Philox
draws of tests/init_ref.py.  The device calls no mathematical library beyond the correctly rounded sqrt, so every GPU test
compares with np.array_equal.

    mass, pos, vel, tries = disc(n, seed, mass, a, r_max)            (bh_initialize_disc)
    planes, exponents = curve(pos, mass, acc, centre, edges)         (bh_rotation_curve; acc = accelerations())
    vel = velocities(pos, centre, centre_vel, radii, vt, sr, st, seed)   (bh_set_disc_velocities; rows in caller order)

numpy only: no GPU, no oracle."""
import math

import numpy as np

import init_ref as I
from radial_ref import MIN_R2, _fixed, exponents_of, slots_of, squared_edges

RADIUS_STREAM = 96
DIR_STREAM0 = 128
DIR_TRIES = 64
G1_STREAM0, G2_STREAM0 = 192, 195


def truncation_factor(a, r_max):
    """F = 1 - a / sqrt(r_max^2 + a^2), as the host forms it (1 without a cut)."""
    a, r_max = float(a), float(r_max)
    return 1.0 if math.isinf(r_max) else 1.0 - a / math.sqrt(r_max * r_max + a * a)


def disc_radii(n, seed, a, r_max):
    i = np.arange(n, dtype=np.uint64)
    w = I.draw(seed, i, RADIUS_STREAM)
    u = I.u01(w[0], w[1]) * truncation_factor(a, r_max)
    t = u * (2.0 - u)
    return (float(a) * np.sqrt(t)) / (1.0 - u)


def disc_directions(n, seed):
    """(c, z, tries): the von Neumann direction of every body and the draws it took (1 .. 64)."""
    i = np.arange(n, dtype=np.uint64)
    p, q, s = np.zeros(n), np.zeros(n), np.zeros(n)
    tries = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    for t in range(DIR_TRIES):
        if not len(live):
            break
        w = I.draw(seed, i[live], DIR_STREAM0 + t)
        pp, qq = 2.0 * I.u01(w[0], w[1]) - 1.0, 2.0 * I.u01(w[2], w[3]) - 1.0
        ss = pp * pp + qq * qq
        p[live], q[live], s[live], tries[live] = pp, qq, ss, t + 1
        live = live[~((ss >= MIN_R2) & (ss <= 1.0))]
    ok = s >= MIN_R2
    rs = np.sqrt(np.where(ok, s, 1.0))
    return np.where(ok, p / rs, 1.0), np.where(ok, q / rs, 0.0), tries


def disc(n, seed, mass, a, r_max):
    """(mass (n,), pos (n, 2), vel (n, 2), tries) in fp64, before the rounding to the state type (init_ref.to_state)."""
    R = disc_radii(n, seed, a, r_max)
    c, z, tries = disc_directions(n, seed)
    m = float(mass) / float(n) if n else 0.0
    return np.full(n, m), np.stack([R * c, R * z], axis=1), np.zeros((n, 2)), tries


def deviates(index, seed):
    """(g1, g2) of the caller indices: ((int64) sum of twelve words - 6 (2^32 - 1)) * 2^-32, exact."""
    index = np.asarray(index, dtype=np.uint64)
    out = []
    for s0 in (G1_STREAM0, G2_STREAM0):
        total = np.zeros(len(index), dtype=np.uint64)
        for k in range(3):
            for word in I.draw(seed, index, s0 + k):
                total = total + word
        out.append((total.astype(np.int64) - np.int64(6 * 0xFFFFFFFF)).astype(np.float64) * (1.0 / 4294967296.0))
    return out


# ---- the rotation curve ------------------------------------------------------------------------------------------------------
def curve_moments(pos, mass, acc, centre):
    """(r2 (n,), q (4, n)) in the stated order; acc is what accelerations() returns."""
    cx, cy = (np.float64(c) for c in centre)
    dx, dy = pos[:, 0] - cx, pos[:, 1] - cy
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    ax, ay = acc[:, 0], acc[:, 1]
    return r2, np.stack([mass, mass * r, mass * (dx * ax + dy * ay), mass * (dx * ay - dy * ax)])


def curve(pos, mass, acc, centre, edges):
    """(planes int64 (5, nb + 2), exponents int32 (4,)); ValueError for a non-finite input or contribution."""
    e2 = squared_edges(edges)
    if len(e2) - 1 > 1022:
        raise ValueError("nb <= 1022")
    with np.errstate(over="ignore", invalid="ignore"):
        r2, q = curve_moments(pos, mass, acc, centre)
    if not (np.isfinite(pos).all() and np.isfinite(mass).all() and np.isfinite(acc).all() and np.isfinite(r2).all() and np.isfinite(q).all()):
        raise ValueError("a body has a non-finite position, mass, acceleration, squared radius or contribution")
    ex = exponents_of(np.abs(q).max(axis=1) if len(mass) else np.zeros(4), len(mass))
    slot = slots_of(r2, e2)
    planes = np.zeros((5, len(e2) + 1), dtype=np.int64)
    for p in range(4):
        np.add.at(planes[p], slot, _fixed(q[p], ex[p]))
    np.add.at(planes[4], slot, 1)
    return planes, ex


# ---- velocities --------------------------------------------------------------------------------------------------------------
def table_at(y, radii, j, r):
    y, radii = np.asarray(y, dtype=np.float64), np.asarray(radii, dtype=np.float64)
    k = len(radii)
    lo, hi = np.clip(j - 1, 0, k - 1), np.clip(j, 0, k - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (r - radii[lo]) / (radii[hi] - radii[lo])
        mid = y[lo] + t * (y[hi] - y[lo])
    return np.where(j == 0, y[0], np.where(j == k, y[k - 1], mid))


def velocities(pos, centre, centre_vel, radii, vt, sr, st, seed, index=None):
    """vel (n, 2) in fp64, before the rounding to the state type; index: the caller indices of the rows (default 0 .. n - 1)."""
    n = len(pos)
    radii = np.asarray(radii, dtype=np.float64)
    cx, cy = (np.float64(c) for c in centre)
    ucx, ucy = (np.float64(c) for c in centre_vel)
    dx, dy = pos[:, 0] - cx, pos[:, 1] - cy
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    j = np.searchsorted(radii * radii, r2, side="right")
    g1, g2 = deviates(np.arange(n) if index is None else index, seed)
    vr = table_at(sr, radii, j, r) * g1
    vtt = table_at(vt, radii, j, r) + table_at(st, radii, j, r) * g2
    with np.errstate(divide="ignore", invalid="ignore"):
        vx, vy = ucx + (vr * dx - vtt * dy) / r, ucy + (vr * dy + vtt * dx) / r
    none = r2 < MIN_R2
    return np.stack([np.where(none, ucx, vx), np.where(none, ucy, vy)], axis=1)


# ---- the analytic Kuzmin-Toomre disc (G M = gm, scale a) ------------------------------------------------------------------------
def kuzmin_sigma(R, mass, a):
    return mass * a / (2.0 * np.pi * (R * R + a * a) ** 1.5)


def kuzmin_vc2(R, gm, a):
    return gm * R * R / (R * R + a * a) ** 1.5


def kuzmin_fraction_inside(R, a, r_max):
    """The fraction of the truncated disc's mass inside R <= r_max."""
    return (1.0 - a / math.sqrt(R * R + a * a)) / truncation_factor(a, r_max)
