"""The numpy twin of csrc/bh_moments.hpp (include/bhgpu.h, "moment maps"): vectorised fp64 in the stated operation order,
np.frexp / np.ldexp / np.rint, accumulation with np.add.at on int64.  Every GPU test compares with np.array_equal.

    planes, exponents, n_deposited = moment_map(pos, vel, mass, box, nx, ny, scheme)

and the pieces a distributed map is made of: maxima(), exponents_of(), deposit().  convert() is the conversion of
BarnesHutEngine.moment_map.  slow_map() is the same definition body by body in Python's integers and fractions, for the
CPU test of this file.  fixture() is the body set of tests/test_gpu_moments.py."""
import math
from fractions import Fraction

import numpy as np

NGP, CIC = 0, 1
SCHEMES = {"ngp": NGP, "cic": CIC}


def state_of(pos, vel, mass, precision_is_f32=False):
    """The state as the device holds it: fp64, after a round trip through fp32 for an fp32 state."""
    out = []
    for a, shape in ((pos, (-1, 2)), (vel, (-1, 2)), (mass, (-1,))):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
        out.append(a.astype(np.float32).astype(np.float64) if precision_is_f32 else a)
    return out


def moments(vel, mass):
    """(4, n): m, m vx, m vy, m (vx vx + vy vy), each product and sum rounded once, in that order."""
    vx, vy = vel[:, 0], vel[:, 1]
    return np.stack([mass, mass * vx, mass * vy, mass * (vx * vx + vy * vy)])


def maxima(pos, vel, mass):
    """max |q_p| per plane (0 without bodies); ValueError for a non-finite body, as the engine's BH_ERR_ARG."""
    with np.errstate(over="ignore", invalid="ignore"):
        q = moments(vel, mass)
    if not (np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(mass).all() and np.isfinite(q).all()):
        raise ValueError("a body has a non-finite position, velocity, mass or moment")
    return np.abs(q).max(axis=1) if q.shape[1] else np.zeros(4)


def log2_ceil(n):
    return 0 if n <= 1 else (int(n) - 1).bit_length()


def exponents_of(maxabs, n_total):
    """62 - E_p - L with max < 2^E_p (frexp) and L = ceil(log2(max(n, 1))); 0 for a plane whose maximum is 0."""
    L = log2_ceil(n_total)
    _, E = np.frexp(np.asarray(maxabs, dtype=np.float64))
    return np.where(np.asarray(maxabs) == 0.0, 0, 62 - E - L).astype(np.int32)


def _fixed(v, e):
    return np.rint(np.ldexp(v, int(e))).astype(np.int64)


def deposit(pos, vel, mass, box, nx, ny, scheme, exponents):
    """(planes int64 (4, ny, nx), n_deposited) of these bodies with the given exponents."""
    xmin, xmax, ymin, ymax = (np.float64(b) for b in box)
    sx, sy = np.float64(nx) / (xmax - xmin), np.float64(ny) / (ymax - ymin)
    x, y = pos[:, 0], pos[:, 1]
    q = moments(vel, mass)
    planes = np.zeros((4, ny * nx), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        if scheme == NGP:
            tx, ty = (x - xmin) * sx, (y - ymin) * sy
            inside = (tx >= 0.0) & (tx < nx) & (x < xmax) & (ty >= 0.0) & (ty < ny) & (y < ymax)
            cell = np.floor(ty[inside]).astype(np.int64) * nx + np.floor(tx[inside]).astype(np.int64)
            for p in range(4):
                np.add.at(planes[p], cell, _fixed(q[p][inside], exponents[p]))
            return planes.reshape(4, ny, nx), int(inside.sum())
        tx, ty = (x - xmin) * sx - 0.5, (y - ymin) * sy - 0.5
        flx, fly = np.floor(tx), np.floor(ty)
        fx, fy = tx - flx, ty - fly
        okx = [(flx >= 0.0) & (flx < nx), (flx >= -1.0) & (flx < nx - 1)]
        oky = [(fly >= 0.0) & (fly < ny), (fly >= -1.0) & (fly < ny - 1)]
        wx, wy = [1.0 - fx, fx], [1.0 - fy, fy]
        for cy in range(2):
            for cx in range(2):
                ok = okx[cx] & oky[cy]
                w = wx[cx][ok] * wy[cy][ok]
                cell = (fly[ok].astype(np.int64) + cy) * nx + (flx[ok].astype(np.int64) + cx)
                for p in range(4):
                    np.add.at(planes[p], cell, _fixed(q[p][ok] * w, exponents[p]))
        return planes.reshape(4, ny, nx), int(((okx[0] | okx[1]) & (oky[0] | oky[1])).sum())


def moment_map(pos, vel, mass, box, nx, ny, scheme, n_total=None):
    """(planes, exponents, n_deposited): bh_moment_map of a state already in the device's precision (state_of)."""
    e = exponents_of(maxima(pos, vel, mass), len(mass) if n_total is None else n_total)
    planes, n_dep = deposit(pos, vel, mass, box, nx, ny, scheme, e)
    return planes, e, n_dep


def convert(planes, exponents, box, nx, ny):
    """mass, px, py, k2, sigma, vx, vy, dispersion as BarnesHutEngine.moment_map forms them."""
    val = [np.ldexp(planes[p].astype(np.float64), -int(exponents[p])) for p in range(4)]
    mass, px, py, k2 = val
    area = ((box[1] - box[0]) / nx) * ((box[3] - box[2]) / ny)
    with np.errstate(divide="ignore", invalid="ignore"):
        vx, vy = px / mass, py / mass
        disp = np.sqrt(np.maximum(k2 / mass - vx * vx - vy * vy, 0.0))
    empty = mass == 0.0
    for a in (vx, vy, disp):
        a[empty] = np.nan
    return dict(mass=mass, px=px, py=py, k2=k2, sigma=mass / area, vx=vx, vy=vy, dispersion=disp)


# ---- the same definition, slowly: one body at a time, Python integers, exact fractions for the rounding ---------------------
def _rint_fraction(f):
    """Round a Fraction to the nearest integer, ties to even (what rint does)."""
    fl = math.floor(f)
    r = f - fl
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2 == 1):
        return fl + 1
    return fl


def slow_map(pos, vel, mass, box, nx, ny, scheme, n_total=None):
    n = len(mass)
    xmin, xmax, ymin, ymax = (float(b) for b in box)
    sx, sy = nx / (xmax - xmin), ny / (ymax - ymin)
    qs = []
    for i in range(n):
        m, vx, vy = float(mass[i]), float(vel[i][0]), float(vel[i][1])
        qs.append((m, m * vx, m * vy, m * (vx * vx + vy * vy)))
    L = log2_ceil(n if n_total is None else n_total)
    e = []
    for p in range(4):
        mx = max((abs(q[p]) for q in qs), default=0.0)
        e.append(0 if mx == 0.0 else 62 - math.frexp(mx)[1] - L)
    planes = [[[0] * nx for _ in range(ny)] for _ in range(4)]
    n_dep = 0
    for i in range(n):
        x, y = float(pos[i][0]), float(pos[i][1])
        corners = []
        if scheme == NGP:
            tx, ty = (x - xmin) * sx, (y - ymin) * sy
            if 0.0 <= tx < nx and x < xmax and 0.0 <= ty < ny and y < ymax:
                corners.append((math.floor(tx), math.floor(ty), None))
        else:
            tx, ty = (x - xmin) * sx - 0.5, (y - ymin) * sy - 0.5
            if math.isfinite(tx) and math.isfinite(ty) and abs(tx) < 2.0 ** 40 and abs(ty) < 2.0 ** 40:
                ix, iy = math.floor(tx), math.floor(ty)
                fx, fy = tx - ix, ty - iy
                for cy, wy in ((0, 1.0 - fy), (1, fy)):
                    for cx, wx in ((0, 1.0 - fx), (1, fx)):
                        if 0 <= ix + cx < nx and 0 <= iy + cy < ny:
                            corners.append((ix + cx, iy + cy, wx * wy))
        n_dep += bool(corners)
        for cx, cy, w in corners:
            for p in range(4):
                v = qs[i][p] if w is None else qs[i][p] * w
                planes[p][cy][cx] += _rint_fraction(Fraction(v) * Fraction(2) ** e[p])
    return planes, e, n_dep


# ---- the fixture of the GPU tests ------------------------------------------------------------------------------------------
BOX = (-1.0, 3.0, -2.0, 1.0)             # 4 x 3: a cell edge is a binary fraction on the 64 x 64 grid, not on 3 x 5 or 257 x 130


def hand_placed(box, nx, ny, far=1e300):
    """Bodies where the rules can go wrong: on interior cell edges, on xmin and xmax, half a cell outside every side and corner,
    far outside (far = 1e300; an fp32 state takes 1e38, the largest decade it can hold), two coincident; masses over
    1e-12 ... 1e6, velocities of both signs and zero."""
    xmin, xmax, ymin, ymax = box
    hx, hy = (xmax - xmin) / nx, (ymax - ymin) / ny
    cx, cy = 0.5 * (xmin + xmax), 0.5 * (ymin + ymax)
    pts = [(xmin + hx * (nx // 2), cy), (cx, ymin + hy * (ny // 2)), (xmin + hx * (nx // 2), ymin + hy * (ny // 2)),   # edges
           (xmin, cy), (xmax, cy), (cx, ymin), (cx, ymax), (xmin, ymin), (xmax, ymax),
           (xmin - 0.5 * hx, cy), (xmax + 0.5 * hx, cy), (cx, ymin - 0.5 * hy), (cx, ymax + 0.5 * hy),               # sides
           (xmin - 0.5 * hx, ymin - 0.5 * hy), (xmax + 0.5 * hx, ymin - 0.5 * hy), (xmin - 0.5 * hx, ymax + 0.5 * hy),
           (xmax + 0.5 * hx, ymax + 0.5 * hy),                                                                       # corners
           (xmin - 0.25 * hx, ymin - 0.25 * hy), (xmax + 0.25 * hx, ymax + 0.25 * hy), (xmax - 0.25 * hx, cy),
           (far, cy), (cx, -far), (-far, far), (1e30, 1e30),                                                 # far outside
           (cx + 0.3 * hx, cy + 0.3 * hy), (cx + 0.3 * hx, cy + 0.3 * hy)]                                           # coincident
    pos = np.array(pts, dtype=np.float64)
    k = len(pos)
    mass = 10.0 ** np.linspace(-12.0, 6.0, k)
    vel = np.zeros((k, 2))
    vel[0::3] = [[0.75, -1.5]]
    vel[1::3] = [[-2.0e-3, 3.0e2]]           # (every third body stays at rest)
    return pos, vel, mass


def fixture(n, box=BOX, nx=64, ny=64, seed=7, at_rest=False, far=1e300, hand=True):
    """n bodies: the hand-placed ones first (as many as fit), the rest from a seeded clumped distribution -- three Gaussian
    clumps, one of them across the box's edge -- with masses log-uniform over 1e-12 ... 1e6 and signed velocities."""
    rng = np.random.default_rng(seed)
    hp, hv, hm = hand_placed(box, nx, ny, far)
    k = min(n, len(hm)) if (n > 1 and hand) else 0      # n = 1: one clump body; hand=False: clump bodies only
    r = n - k
    xmin, xmax, ymin, ymax = box
    centres = np.array([[0.5 * (xmin + xmax), 0.5 * (ymin + ymax)], [xmin + 0.8 * (xmax - xmin), ymin + 0.3 * (ymax - ymin)],
                        [xmax, ymax]])
    which = rng.integers(0, 3, size=r)
    pos = centres[which] + rng.normal(size=(r, 2)) * np.array([0.3, 0.05, 0.2])[which, None]
    mass = 10.0 ** rng.uniform(-12.0, 6.0, size=r)
    vel = rng.normal(size=(r, 2)) * 2.0
    vel[rng.random(r) < 0.1] = 0.0
    pos, vel, mass = np.concatenate([hp[:k], pos]), np.concatenate([hv[:k], vel]), np.concatenate([hm[:k], mass])
    if at_rest:
        vel = np.zeros_like(vel)
    return pos, vel, mass
