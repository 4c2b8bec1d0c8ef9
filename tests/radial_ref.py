"""The numpy twin of csrc/bh_radial.hpp (include/bhgpu.h, "radial profiles and Lagrangian radii"): vectorised fp64 in the stated
operation order, np.frexp / np.ldexp / np.rint, accumulation with np.add.at on int64.  Every GPU test compares with
np.array_equal.

    planes, exponents = profile(pos, vel, mass, centre, centre_vel, edges)
    r2, count, mass_units, e0 = lagrangian(pos, mass, centre, fractions)          (by plain sorting)
    r2, count, mass_units, e0 = lagrangian_rounds(pos, mass, centre, fractions)   (the eight rounds, emulated)

and the pieces a distributed call is made of: maxima(), exponents_of(), deposit(), select_hist().  slow_profile() is the same
definition body by body in Python's integers and fractions.  fixture() is the body set of tests/test_gpu_radial.py."""
import math
from fractions import Fraction

import numpy as np

from gpu_nbody_simulation_amd.engine import LagrangianSelect
from moments_ref import _rint_fraction, log2_ceil, state_of  # noqa: F401

MIN_R2 = 2.0 ** -1022


def moments(pos, vel, mass, centre, centre_vel=(0.0, 0.0), with_vel=True):
    """(r2 (n,), q (5, n)) in the stated order; with_vel=False (the radii): q1 .. q4 are 0 and vel is not read."""
    cx, cy = (np.float64(c) for c in centre)
    dx, dy = pos[:, 0] - cx, pos[:, 1] - cy
    r2 = dx * dx + dy * dy
    vr, vt = np.zeros(len(mass)), np.zeros(len(mass))
    if with_vel:
        ux, uy = vel[:, 0] - np.float64(centre_vel[0]), vel[:, 1] - np.float64(centre_vel[1])
        a, b = dx * ux + dy * uy, dx * uy - dy * ux
        ok = r2 >= MIN_R2
        with np.errstate(all="ignore"):
            r = np.sqrt(r2)
            vr, vt = np.where(ok, a / np.where(ok, r, 1.0), 0.0), np.where(ok, b / np.where(ok, r, 1.0), 0.0)
    return r2, np.stack([mass, mass * vr, mass * vt, mass * (vr * vr), mass * (vt * vt)])


def maxima(pos, vel, mass, centre, centre_vel=(0.0, 0.0), with_vel=True):
    """max |q_p| per plane (0 without bodies); ValueError for a non-finite body, as the engine's BH_ERR_ARG."""
    with np.errstate(over="ignore", invalid="ignore"):
        r2, q = moments(pos, vel, mass, centre, centre_vel, with_vel)
    fin = np.isfinite(pos).all() and np.isfinite(mass).all() and np.isfinite(r2).all() and np.isfinite(q).all()
    if not (fin and (not with_vel or np.isfinite(vel).all())):
        raise ValueError("a body has a non-finite position, velocity, mass, squared radius or moment")
    return np.abs(q).max(axis=1) if q.shape[1] else np.zeros(5)


def exponents_of(maxabs, n_total):
    L = log2_ceil(n_total)
    _, E = np.frexp(np.asarray(maxabs, dtype=np.float64))
    return np.where(np.asarray(maxabs) == 0.0, 0, 62 - E - L).astype(np.int32)


def _fixed(v, e):
    return np.rint(np.ldexp(v, int(e))).astype(np.int64)


def squared_edges(edges):
    """e2 of valid edges; ValueError otherwise, as the engine's BH_ERR_ARG."""
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        e2 = edges * edges
    if len(edges) < 2 or len(edges) > 4097 or not (np.isfinite(edges).all() and np.isfinite(e2).all()) or edges[0] < 0.0 \
            or not (np.diff(edges) > 0.0).all() or not (np.diff(e2) > 0.0).all():
        raise ValueError("edges: finite, >= 0, strictly ascending, and so their squares; 1 .. 4096 bins")
    return e2


def slots_of(r2, e2):
    """The number of squared edges <= r2: 0 inside edges[0], nb + 1 at or beyond edges[nb]."""
    return np.searchsorted(e2, r2, side="right")


def deposit(pos, vel, mass, centre, centre_vel, edges, exponents):
    """planes int64 (6, nb + 2) of these bodies with the given exponents."""
    e2 = squared_edges(edges)
    r2, q = moments(pos, vel, mass, centre, centre_vel)
    slot = slots_of(r2, e2)
    planes = np.zeros((6, len(e2) + 1), dtype=np.int64)
    for p in range(5):
        np.add.at(planes[p], slot, _fixed(q[p], exponents[p]))
    np.add.at(planes[5], slot, 1)
    return planes


def profile(pos, vel, mass, centre, centre_vel, edges, n_total=None):
    """(planes, exponents): bh_radial_profile of a state already in the device's precision (state_of)."""
    e = exponents_of(maxima(pos, vel, mass, centre, centre_vel), len(mass) if n_total is None else n_total)
    return deposit(pos, vel, mass, centre, centre_vel, edges, e), e


def slow_profile(pos, vel, mass, centre, centre_vel, edges, n_total=None):
    """The same definition, one body at a time: Python floats for the fp64 operations, integers for the sums, exact fractions
    for the rounding.  (planes as lists of ints, exponents)"""
    n = len(mass)
    cx, cy, ucx, ucy = float(centre[0]), float(centre[1]), float(centre_vel[0]), float(centre_vel[1])
    e2 = [float(e) * float(e) for e in edges]
    rows = []
    for i in range(n):
        dx, dy = float(pos[i][0]) - cx, float(pos[i][1]) - cy
        r2 = dx * dx + dy * dy
        ux, uy = float(vel[i][0]) - ucx, float(vel[i][1]) - ucy
        a, b = dx * ux + dy * uy, dx * uy - dy * ux
        vr = vt = 0.0
        if r2 >= MIN_R2:
            r = math.sqrt(r2)
            vr, vt = a / r, b / r
        m = float(mass[i])
        rows.append((r2, (m, m * vr, m * vt, m * (vr * vr), m * (vt * vt))))
    L = log2_ceil(n if n_total is None else n_total)
    e = []
    for p in range(5):
        mx = max((abs(q[p]) for _, q in rows), default=0.0)
        e.append(0 if mx == 0.0 else 62 - math.frexp(mx)[1] - L)
    planes = [[0] * (len(e2) + 1) for _ in range(6)]
    for r2, q in rows:
        slot = sum(1 for t in e2 if t <= r2)
        for p in range(5):
            planes[p][slot] += _rint_fraction(Fraction(q[p]) * Fraction(2) ** e[p])
        planes[5][slot] += 1
    return planes, e


# ---- Lagrangian radii --------------------------------------------------------------------------------------------------------
def weights(pos, mass, centre, n_total=None, e0=None):
    """(r2, w int64, e0): ValueError for a non-finite body or a negative mass."""
    mx = maxima(pos, None, mass, centre, with_vel=False)
    if (mass < 0.0).any():
        raise ValueError("a body has a negative mass")
    if e0 is None:
        e0 = int(exponents_of(mx, len(mass) if n_total is None else n_total)[0])
    r2, _ = moments(pos, None, mass, centre, with_vel=False)
    return r2, _fixed(mass, e0), e0


def target_of(f, W):
    return min(W, max(1, int(math.ceil(float(f) * float(W)))))


def check_fractions(fractions):
    f = [float(x) for x in np.asarray(fractions, dtype=np.float64).reshape(-1)]
    if not 1 <= len(f) <= 32 or not all(math.isfinite(x) and 0.0 < x <= 1.0 for x in f):
        raise ValueError("1 .. 32 fractions, each finite, > 0 and <= 1")
    return f


def lagrangian(pos, mass, centre, fractions, n_total=None):
    """The definition by plain sorting: (r2 float64, count int64, mass_units int64, e0)."""
    fr = check_fractions(fractions)
    r2, w, e0 = weights(pos, mass, centre, n_total)
    W = sum(int(x) for x in w)
    nf = len(fr)
    if W == 0:
        return np.full(nf, np.nan), np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64), e0
    order = np.argsort(r2, kind="stable")
    rs, cum = r2[order], np.cumsum(w[order])                   # (W <= 2^62: the cumulative sums stay in int64)
    out_r2, out_n, out_m = [], [], []
    for f in fr:
        T = target_of(f, W)
        # the candidates t are the r2 of bodies; the sum over r2_i <= t is the cumulative sum at the LAST body tied with t
        last = np.searchsorted(rs, rs, side="right") - 1
        k = int(np.argmax(cum[last] >= T))
        out_r2.append(rs[k]); out_n.append(int(last[k]) + 1); out_m.append(int(cum[last[k]]))
    return np.array(out_r2), np.array(out_n, dtype=np.int64), np.array(out_m, dtype=np.int64), e0


def select_hist(r2, w, round, prefixes):
    """One round's histograms (np, 256, 2) int64 of these bodies: the twin of bh_radial_select."""
    key = np.ascontiguousarray(r2, dtype=np.float64).view(np.uint64)
    hist = np.zeros((len(prefixes), 256, 2), dtype=np.int64)
    high = np.zeros(len(key), dtype=np.uint64) if round == 0 else key >> np.uint64(64 - 8 * round)
    digit = ((key >> np.uint64(56 - 8 * round)) & np.uint64(255)).astype(np.int64)
    for k, p in enumerate(prefixes):
        sel = high == np.uint64(p)
        np.add.at(hist[k, :, 0], digit[sel], w[sel])
        np.add.at(hist[k, :, 1], digit[sel], 1)
    return hist


def lagrangian_rounds(parts, centre, fractions, n_total=None):
    """The eight rounds over `parts` = [(pos, mass), ...] ("ranks": their maxima are combined with max, their body counts and
    histograms added), the decisions by engine.LagrangianSelect.  (r2, count, mass_units, e0, rounds run)"""
    check_fractions(fractions)
    n = sum(len(m) for _, m in parts) if n_total is None else n_total
    mx = max((float(maxima(p, None, m, centre, with_vel=False)[0]) for p, m in parts), default=0.0)
    e0 = int(exponents_of([mx], n)[0])
    ws = [weights(p, m, centre, e0=e0)[:2] for p, m in parts]
    sel = LagrangianSelect(fractions)
    rounds = 0
    while not sel.done:
        pre = sel.prefixes()
        sel.advance(sum(select_hist(r2, w, sel.round, pre) for r2, w in ws))
        rounds += 1
    return (*sel.result(), e0, rounds)


def convert(planes, exponents, edges):
    """The derived quantities as BarnesHutEngine.radial_profile forms them."""
    edges = np.asarray(edges, dtype=np.float64)
    val = [np.ldexp(planes[p].astype(np.float64), -int(exponents[p])) for p in range(5)]
    mass, pr, pt, kr, kt = (v[1:-1] for v in val)
    e2 = edges * edges
    with np.errstate(divide="ignore", invalid="ignore"):
        vr, vt = pr / mass, pt / mass
        var_r, var_t = np.maximum(kr / mass - vr * vr, 0.0), np.maximum(kt / mass - vt * vt, 0.0)
        beta = 1.0 - var_t / var_r
    out = dict(vr=vr, vt=vt, sigma_r=np.sqrt(var_r), sigma_t=np.sqrt(var_t), anisotropy=beta)
    for a in out.values():
        a[mass == 0.0] = np.nan
    enclosed = np.ldexp(np.array([float(sum(int(v) for v in planes[0][:k + 1])) for k in range(len(edges))]), -int(exponents[0]))
    out.update(mass=mass, sigma=mass / (np.pi * (e2[1:] - e2[:-1])), count=planes[5][1:-1], enclosed=enclosed,
               r_mid=0.5 * (edges[:-1] + edges[1:]), mass_inside=float(val[0][0]), mass_outside=float(val[0][-1]))
    return out


# ---- the fixture of the GPU tests ------------------------------------------------------------------------------------------
CENTRE = (0.0, -0.5)                     # cx = 0: a body can stand 2^-520 from the centre; binary fractions: dx is exact
CENTRE_VEL = (0.125, -0.0625)


def fixture_edges(nb):
    """nb + 1 edges from 0.125 to 2.125: linear, so that with nb a power of two an edge is a binary fraction."""
    return 0.125 + 2.0 * (np.arange(nb + 1) / nb)


def hand_placed(edges, centre=CENTRE):
    """Bodies where the rules can go wrong: exactly on edges (on the axes, where r2 is the edge's square exactly), one at the
    centre, one with a subnormal r2, mirror images with equal r2, inside edges[0] and beyond edges[nb], a massless one."""
    cx, cy = centre
    e = np.asarray(edges, dtype=np.float64)
    nb = len(e) - 1
    pts = [(cx + e[0], cy), (cx, cy - e[nb]), (cx - e[nb // 2], cy), (cx, cy + e[min(1, nb)]),              # on edges
           (cx, cy),                                                                                     # at the centre
           (cx + 2.0 ** -520, cy),                                                                       # r2 = 2^-1040, subnormal
           (cx + 0.75, cy + 0.5), (cx - 0.75, cy + 0.5), (cx + 0.75, cy - 0.5), (cx - 0.5, cy - 0.75),   # mirror images: equal r2
           (cx + 0.0625, cy), (cx, cy - 0.03125),                                                        # inside edges[0]
           (cx + 3.0, cy + 4.0), (cx - 100.0, cy),                                                       # beyond edges[nb]
           (cx + 0.3, cy + 0.1)]                                                                         # massless (below)
    pos = np.array(pts, dtype=np.float64)
    k = len(pos)
    mass = 10.0 ** np.linspace(-3.0, 3.0, k)
    mass[6:10] = [8.0, 8.0, 8.0, 8.0]
    mass[k - 1] = 0.0
    vel = np.zeros((k, 2))
    vel[0::3] = [[0.75, -1.5]]
    vel[1::3] = [[-2.0e-3, 3.0e2]]
    return pos, vel, mass


def fixture(n, nb=32, seed=11, at_rest=False, hand=True, decades=6.0):
    """n bodies: the hand-placed ones first (as many as fit), the rest from a seeded clumped distribution about CENTRE with
    masses log-uniform over 10^-decades ... 10^decades and signed velocities."""
    rng = np.random.default_rng(seed)
    hp, hv, hm = hand_placed(fixture_edges(nb))
    k = min(n, len(hm)) if (n > 1 and hand) else 0
    r = n - k
    rad = np.abs(rng.normal(size=r)) * np.where(rng.random(r) < 0.7, 0.6, 2.5)
    phi = rng.uniform(0.0, 2.0 * np.pi, size=r)
    pos = np.array(CENTRE) + np.stack([rad * np.cos(phi), rad * np.sin(phi)], axis=1)
    mass = 10.0 ** rng.uniform(-decades, decades, size=r)
    vel = rng.normal(size=(r, 2)) * 2.0
    vel[rng.random(r) < 0.1] = 0.0
    pos, vel, mass = np.concatenate([hp[:k], pos]), np.concatenate([hv[:k], vel]), np.concatenate([hm[:k], mass])
    if at_rest:
        vel = np.zeros_like(vel)
    return pos, vel, mass
