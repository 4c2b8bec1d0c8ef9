"""The numpy twin of csrc/bh_modes.hpp (include/bhgpu.h, "azimuthal Fourier modes"): vectorised fp64 in the stated operation
order, np.frexp / np.ldexp / np.rint, accumulation with np.add.at on int64.  Every GPU test compares with np.array_equal.

    planes, exponents = modes(pos, vel, mass, centre, centre_vel, edges, M, rates)

and the pieces a distributed call is made of: maxima(), exponents_of(), deposit().  slow_modes() is the same definition body by
body in Python's floats, integers and fractions (moments_ref's exact rint); trig_sums() is an INDEPENDENT formulation,
m exp(i k atan2(dy, dx)) summed in long double.  convert() is the conversion of BarnesHutEngine.azimuthal_modes.  The slots are
radial_ref's; fixture() is radial_ref's body set (bodies on edges, at the centre, with a subnormal r2 ...), square() and
rotator() are the known answers."""
import math
from fractions import Fraction

import numpy as np

from moments_ref import _rint_fraction, log2_ceil, state_of  # noqa: F401
from radial_ref import CENTRE, CENTRE_VEL, MIN_R2, exponents_of, fixture, fixture_edges, slots_of, squared_edges  # noqa: F401

MAX_M, MAX_BINS, LDS_BYTES = 16, 4096, 65536


def n_planes(M, rates):
    return (2 if rates else 1) * (1 + 2 * M) + 1


def plan(P, nb):
    """(tile, bytes) of the deposit's dynamic LDS: tile 0 is the private histogram with its edges, else floor(65,536 / (8 P))
    slots (csrc/bh_query_host.hpp: modes_plan)."""
    whole = 8 * P * (nb + 2) + 8 * (nb + 1)
    if whole <= LDS_BYTES:
        return 0, whole
    tile = LDS_BYTES // (8 * P)
    return tile, 8 * P * tile


def largest_private_nb(P):
    """The largest nb whose whole histogram and edges fit: 8 P (nb + 2) + 8 (nb + 1) <= 65,536."""
    return (LDS_BYTES // 8 - 2 * P - 1) // (P + 1)


def contributions(pos, vel, mass, centre, centre_vel=(0.0, 0.0), M=4, rates=False):
    """(r2 (n,), qA (1 + 2M, n), qD (1 + 2M, n) or None) in the stated order; without rates vel is not read."""
    cx, cy = (np.float64(c) for c in centre)
    dx, dy = pos[:, 0] - cx, pos[:, 1] - cy
    with np.errstate(all="ignore"):
        r2 = dx * dx + dy * dy
        ok = r2 >= MIN_R2
        r = np.sqrt(np.where(ok, r2, 1.0))
        c1, s1 = np.where(ok, dx / r, 0.0), np.where(ok, dy / r, 0.0)
        mw = None
        if rates:
            ux, uy = vel[:, 0] - np.float64(centre_vel[0]), vel[:, 1] - np.float64(centre_vel[1])
            b = dx * uy - dy * ux
            w = np.where(ok, b / np.where(ok, r2, 1.0), 0.0)
            mw = mass * w
        c, s = np.ones(len(mass)), np.zeros(len(mass))
        rows_a, rows_d = [mass * c], [mw * c] if rates else []
        for _ in range(M):
            c, s = c * c1 - s * s1, s * c1 + c * s1
            rows_a += [mass * c, mass * s]
            if rates:
                rows_d += [mw * c, mw * s]
    return r2, np.stack(rows_a), np.stack(rows_d) if rates else None


def maxima(pos, vel, mass, centre, centre_vel=(0.0, 0.0), M=4, rates=False):
    """[maxA, maxD] (0 without bodies, maxD = 0 without rates); ValueError for a non-finite body, as the engine's BH_ERR_ARG."""
    r2, qa, qd = contributions(pos, vel, mass, centre, centre_vel, M, rates)
    fin = np.isfinite(pos).all() and np.isfinite(mass).all() and np.isfinite(r2).all() and np.isfinite(qa).all()
    if rates:
        fin = fin and np.isfinite(vel).all() and np.isfinite(qd).all()
    if not fin:
        raise ValueError("a body has a non-finite position, velocity, mass, squared radius or contribution")
    n = len(mass)
    return np.array([np.abs(qa).max() if n else 0.0, np.abs(qd).max() if (n and rates) else 0.0])


def _fixed(v, e):
    return np.rint(np.ldexp(v, int(e))).astype(np.int64)


def deposit(pos, vel, mass, centre, centre_vel, edges, M, rates, exponents):
    """planes int64 (P, nb + 2) of these bodies with the two given exponents."""
    e2 = squared_edges(edges)
    r2, qa, qd = contributions(pos, vel, mass, centre, centre_vel, M, rates)
    slot = slots_of(r2, e2)
    n_a = 1 + 2 * M
    planes = np.zeros((n_planes(M, rates), len(e2) + 1), dtype=np.int64)
    for p in range(n_a):
        np.add.at(planes[p], slot, _fixed(qa[p], exponents[0]))
        if rates:
            np.add.at(planes[n_a + p], slot, _fixed(qd[p], exponents[1]))
    np.add.at(planes[-1], slot, 1)
    return planes


def modes(pos, vel, mass, centre, centre_vel, edges, M, rates, n_total=None):
    """(planes, exponents): bh_azimuthal_modes of a state already in the device's precision (state_of)."""
    e = exponents_of(maxima(pos, vel, mass, centre, centre_vel, M, rates), len(mass) if n_total is None else n_total)
    return deposit(pos, vel, mass, centre, centre_vel, edges, M, rates, e), e


def slow_modes(pos, vel, mass, centre, centre_vel, edges, M, rates, n_total=None):
    """The same definition, one body at a time: Python floats for the fp64 operations, integers for the sums, exact fractions
    for the rounding.  (planes as lists of ints, exponents)"""
    n = len(mass)
    cx, cy, ucx, ucy = float(centre[0]), float(centre[1]), float(centre_vel[0]), float(centre_vel[1])
    e2 = [float(e) * float(e) for e in edges]
    n_a = 1 + 2 * M
    rows = []
    for i in range(n):
        dx, dy = float(pos[i][0]) - cx, float(pos[i][1]) - cy
        r2 = dx * dx + dy * dy
        m = float(mass[i])
        c1 = s1 = w = 0.0
        if r2 >= MIN_R2:
            r = math.sqrt(r2)
            c1, s1 = dx / r, dy / r
        if rates:
            ux, uy = float(vel[i][0]) - ucx, float(vel[i][1]) - ucy
            b = dx * uy - dy * ux
            if r2 >= MIN_R2:
                w = b / r2
        mw = m * w
        c, s = 1.0, 0.0
        qa, qd = [m * c], [mw * c]
        for _ in range(M):
            c, s = c * c1 - s * s1, s * c1 + c * s1
            qa += [m * c, m * s]
            qd += [mw * c, mw * s]
        rows.append((r2, qa, qd))
    L = log2_ceil(n if n_total is None else n_total)
    e = []
    for which in (1, 2):
        mx = max((abs(v) for row in rows for v in row[which]), default=0.0) if (which == 1 or rates) else 0.0
        e.append(0 if mx == 0.0 else 62 - math.frexp(mx)[1] - L)
    planes = [[0] * (len(e2) + 1) for _ in range(n_planes(M, rates))]
    for r2, qa, qd in rows:
        slot = sum(1 for t in e2 if t <= r2)
        for p in range(n_a):
            planes[p][slot] += _rint_fraction(Fraction(qa[p]) * Fraction(2) ** e[0])
            if rates:
                planes[n_a + p][slot] += _rint_fraction(Fraction(qd[p]) * Fraction(2) ** e[1])
        planes[-1][slot] += 1
    return planes, e


def trig_sums(pos, mass, centre, edges, M):
    """An independent formulation: A_k per slot as sum m exp(i k atan2(dy, dx)) in long double -> (re, im) (M + 1, nb + 2)."""
    ld = np.longdouble
    dx, dy = pos[:, 0] - np.float64(centre[0]), pos[:, 1] - np.float64(centre[1])
    r2 = dx * dx + dy * dy
    slot = slots_of(r2, squared_edges(edges))
    phi = np.arctan2(dy.astype(ld), dx.astype(ld))
    has = (r2 >= MIN_R2).astype(ld)
    re, im = np.zeros((M + 1, len(edges) + 1), dtype=ld), np.zeros((M + 1, len(edges) + 1), dtype=ld)
    for k in range(M + 1):
        f = has if k else np.ones(len(mass), dtype=ld)
        np.add.at(re[k], slot, mass.astype(ld) * np.cos(k * phi) * f)
        np.add.at(im[k], slot, mass.astype(ld) * np.sin(k * phi) * f)
    return re, im


def values(planes, exponents, M, rates):
    """(A (M + 1, nb + 2) complex, D likewise or None): the sums times 2^-exponent."""
    n_a = 1 + 2 * M

    def rows(first, e):
        val = np.ldexp(np.asarray(planes[first:first + n_a], dtype=np.int64).astype(np.float64), -int(e))
        out = np.zeros((M + 1, val.shape[1]), dtype=np.complex128)
        out[0] = val[0]
        out[1:] = val[1::2] + 1j * val[2::2]
        return out

    return rows(0, exponents[0]), rows(n_a, exponents[1]) if rates else None


def convert(planes, exponents, M, rates):
    """The derived quantities as BarnesHutEngine.azimuthal_modes forms them."""
    a, d = values(planes, exponents, M, rates)
    a = a[:, 1:-1]
    mass = a[0].real.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.where(mass == 0.0, np.nan, np.hypot(a.real, a.imag) / mass)
        phase = np.zeros(a.shape)
        for k in range(1, M + 1):
            phase[k] = np.arctan2(a[k].imag, a[k].real) / k
        out = dict(mass=mass, coeff=a, amplitude=amp, phase=phase, count=np.asarray(planes[-1], dtype=np.int64)[1:-1])
        if rates:
            d = d[:, 1:-1]
            speed = (d.real * a.real + d.imag * a.imag) / (a.real * a.real + a.imag * a.imag)
            speed[(a.real == 0.0) & (a.imag == 0.0)] = np.nan
            speed[0] = np.nan
            out.update(rate_coeff=d, pattern_speed=speed)
    return out


# ---- known answers -------------------------------------------------------------------------------------------------------------
SQUARE_CENTRE = (0.5, 0.25)
OMEGA = 0.37


def square(m=1.0):
    """Four equal masses at c +- (3, 0) and c +- (0, 3): every quantity is exact, A_0 = A_4 = A_8 = ... = 4 m, every other 0."""
    c = np.array(SQUARE_CENTRE)
    pos = c + np.array([[3.0, 0.0], [-3.0, 0.0], [0.0, 3.0], [0.0, -3.0]])
    return pos, np.zeros((4, 2)), np.full(4, float(m))


def rotator(n, seed=5, centre=(0.75, -0.5), centre_vel=(0.125, -0.0625), omega=OMEGA):
    """An anisotropic Gaussian with axes 1 : 0.4 about `centre` in rigid rotation: v = u_c + omega z x (x - c)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 2)) * np.array([1.0, 0.4])
    pos = np.array(centre) + d
    d = pos - np.array(centre)
    vel = np.array(centre_vel) + omega * np.stack([-d[:, 1], d[:, 0]], axis=1)
    return pos, vel, rng.uniform(0.5, 1.5, n)


def quarter_turn(pos, vel, centre):
    """Every body turned by exactly 90 degrees about the centre, by swapping and negating coordinates: (dx, dy) -> (-dy, dx).
    Exact when the offsets are (binary fractions about a binary-fraction centre); returns (pos, vel)."""
    c = np.array(centre)
    d = pos - c
    return c + np.stack([-d[:, 1], d[:, 0]], axis=1), np.stack([-vel[:, 1], vel[:, 0]], axis=1)
