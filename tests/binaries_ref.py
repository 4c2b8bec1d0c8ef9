"""Brute-force twin of bh_binaries / bh_binaries_catalogue (no test in here): numpy float64 over all pairs in chunks, with exactly
the operation order of include/bhgpu.h -- numpy fuses nothing, and its sqrt and division are the correctly rounded ones.

  dx = x_j - x_i; dy = y_j - y_i; d2 = dx * dx + dy * dy
  ux = vx_j - vx_i; uy = vy_j - vy_i; v2 = ux * ux + uy * uy
  M = m_i + m_j;  eps_ij = 0.5 * v2 - (G * M) / sqrt(d2)
  candidates of i: 0 < d2 <= R * R and eps_ij < 0;  partner: first in (eps_ij, j);  binary: mutual partners lo < hi."""
import math

import numpy as np

_BLOCK = 256                      # rows per block of the pair matrices
RECORD = 11


def _state(pos, vel, mass):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    return pos, np.asarray(vel, dtype=np.float64).reshape(-1, 2), np.asarray(mass, dtype=np.float64).reshape(-1)


def eps_block(pos, vel, mass, G, rows):
    """(d2, eps)[r, j] of body rows[r] and body j"""
    dx = pos[None, :, 0] - pos[rows, None, 0]
    dy = pos[None, :, 1] - pos[rows, None, 1]
    d2 = dx * dx + dy * dy
    ux = vel[None, :, 0] - vel[rows, None, 0]
    uy = vel[None, :, 1] - vel[rows, None, 1]
    v2 = ux * ux + uy * uy
    M = mass[rows, None] + mass[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        eps = 0.5 * v2 - (G * M) / np.sqrt(d2)
    return d2, eps


def partners(pos, vel, mass, G, R):
    """(partner (n,) int64, eps (n,)): -1 and +inf without a candidate"""
    pos, vel, mass = _state(pos, vel, mass)
    n = len(pos)
    R2 = float(R) * float(R)
    G = float(G)
    partner = np.full(n, -1, dtype=np.int64)
    eps_out = np.full(n, np.inf)
    for r0 in range(0, n, _BLOCK):
        rows = np.arange(r0, min(n, r0 + _BLOCK))
        d2, eps = eps_block(pos, vel, mass, G, rows)
        cand = (d2 > 0.0) & (d2 <= R2) & (eps < 0.0)
        low = np.where(cand, eps, np.inf).min(axis=1)
        first = cand & (eps == low[:, None])
        j = first.argmax(axis=1)                                  # (the first True: the smallest index among the ties)
        have = cand.any(axis=1)
        partner[rows[have]] = j[have]
        eps_out[rows[have]] = low[have]
    return partner, eps_out


def mutual(partner):
    """(lo, hi) of the mutual pairs, ascending in lo"""
    partner = np.asarray(partner, dtype=np.int64)
    i = np.arange(len(partner), dtype=np.int64)
    ok = partner > i
    ok[ok] = partner[partner[ok]] == i[ok]
    return i[ok], partner[ok]


def elements(pos, vel, mass, G, lo, hi):
    """(p, 11): r, eps, a, e, period, binding, M, com x, com y, velocity x, velocity y of the pairs (lo, hi)"""
    pos, vel, mass = _state(pos, vel, mass)
    G = float(G)
    xi, xj, vi, vj, mi, mj = pos[lo], pos[hi], vel[lo], vel[hi], mass[lo], mass[hi]
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    d2 = dx * dx + dy * dy
    ux, uy = vj[:, 0] - vi[:, 0], vj[:, 1] - vi[:, 1]
    v2 = ux * ux + uy * uy
    M = mi + mj
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = G * M
        r = np.sqrt(d2)
        eps = 0.5 * v2 - mu / r
        a = mu / (-2.0 * eps)
        h = dx * uy - dy * ux
        e2 = 1.0 + ((2.0 * eps) * (h * h)) / (mu * mu)
        e = np.sqrt(np.where(e2 > 0.0, e2, 0.0))
        period = 6.283185307179586 * np.sqrt(((a * a) * a) / mu)
        binding = -(((mi * mj) / M) * eps)
        com_x, com_y = (mi * xi[:, 0] + mj * xj[:, 0]) / M, (mi * xi[:, 1] + mj * xj[:, 1]) / M
        vel_x, vel_y = (mi * vi[:, 0] + mj * vj[:, 0]) / M, (mi * vi[:, 1] + mj * vj[:, 1]) / M
    return np.stack([r, eps, a, e, period, binding, M, com_x, com_y, vel_x, vel_y], axis=1).reshape(-1, RECORD)


def catalogue(pos, vel, mass, G, R):
    """(partner, eps, lo, hi, records (p, 11))"""
    partner, eps = partners(pos, vel, mass, G, R)
    lo, hi = mutual(partner)
    return partner, eps, lo, hi, elements(pos, vel, mass, G, lo, hi)


# ---- the same in plain Python: float arithmetic, math.sqrt, every pair, `sorted` on (eps, j) tuples ---------------------------
def partners_py(pos, vel, mass, G, R):
    pos, vel, mass = _state(pos, vel, mass)
    P, V, Mm = pos.tolist(), vel.tolist(), mass.tolist()
    n = len(P)
    R2 = float(R) * float(R)
    G = float(G)
    partner, out = [], []
    for i in range(n):
        cand = []
        for j in range(n):
            if j == i:
                continue
            dx = P[j][0] - P[i][0]
            dy = P[j][1] - P[i][1]
            d2 = dx * dx + dy * dy
            if not (0.0 < d2 <= R2):
                continue
            ux = V[j][0] - V[i][0]
            uy = V[j][1] - V[i][1]
            v2 = ux * ux + uy * uy
            M = Mm[i] + Mm[j]
            eps = 0.5 * v2 - (G * M) / math.sqrt(d2)
            if eps < 0.0:
                cand.append((eps, j))
        best = sorted(cand)[0] if cand else (math.inf, -1)
        partner.append(best[1])
        out.append(best[0])
    return np.array(partner, dtype=np.int64).reshape(-1), np.array(out, dtype=np.float64).reshape(-1)


def mutual_py(partner):
    p = [int(x) for x in partner]
    pairs = [(i, p[i]) for i in range(len(p)) if p[i] > i and p[p[i]] == i]
    return (np.array([a for a, _ in pairs], dtype=np.int64).reshape(-1), np.array([b for _, b in pairs], dtype=np.int64).reshape(-1))


# ---- states ---------------------------------------------------------------------------------------------------------------------
def kepler_pair(m1, m2, a, e, phase, G=1.0):
    """(mass (2,), pos (2, 2), vel (2, 2)): two bodies on the Kepler orbit of semi-major axis a and eccentricity e < 1 at true
    anomaly `phase`, pericentre on the +x axis, counter-clockwise, centre of mass at rest at the origin"""
    M = m1 + m2
    mu = G * M
    p = a * (1.0 - e * e)
    r = p / (1.0 + e * math.cos(phase))
    rel = np.array([r * math.cos(phase), r * math.sin(phase)])
    w = math.sqrt(mu / p)
    urel = np.array([-w * math.sin(phase), w * (e + math.cos(phase))])
    pos = np.stack([-(m2 / M) * rel, (m1 / M) * rel])
    vel = np.stack([-(m2 / M) * urel, (m1 / M) * urel])
    return np.array([m1, m2], dtype=np.float64), pos, vel


def kepler_period(m1, m2, a, G=1.0):
    return 2.0 * math.pi * math.sqrt(a ** 3 / (G * (m1 + m2)))


def cluster(n, n_binaries, seed):
    """(mass, pos, vel, planted): a Plummer-like disc in units G = 1, total mass about 1, scale radius 1 -- n - n_binaries
    centres of mass, of which the first n_binaries are replaced by a tight Kepler pair each (a log-uniform in [1e-5, 3e-4],
    e uniform in [0, 0.7], random phase and orientation) --, in a shuffled caller order.  planted: (n_binaries, 4) rows
    {caller index, caller index, a, e}.  2 * n_binaries <= n."""
    assert 0 <= 2 * n_binaries <= n
    rng = np.random.default_rng(seed)
    nc = n - n_binaries
    u = rng.uniform(0.02, 0.98, size=nc)
    rad = 1.0 / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
    ang = rng.uniform(0.0, 2.0 * math.pi, size=nc)
    cpos = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    cvel = rng.normal(size=(nc, 2)) * (math.sqrt(1.0 / 6.0) / (1.0 + rad * rad) ** 0.25)[:, None]
    m = rng.uniform(0.5, 1.5, size=n) / max(n, 1)
    mass, pos, vel = np.zeros(n), np.zeros((n, 2)), np.zeros((n, 2))
    a = 10.0 ** rng.uniform(-5.0, math.log10(3e-4), size=n_binaries)
    e = rng.uniform(0.0, 0.7, size=n_binaries)
    phase = rng.uniform(0.0, 2.0 * math.pi, size=n_binaries)
    turn = rng.uniform(0.0, 2.0 * math.pi, size=n_binaries)
    for k in range(n_binaries):
        mk, pk, vk = kepler_pair(m[2 * k], m[2 * k + 1], a[k], e[k], phase[k])
        c, s = math.cos(turn[k]), math.sin(turn[k])
        rot = np.array([[c, -s], [s, c]])
        mass[2 * k:2 * k + 2] = mk
        pos[2 * k:2 * k + 2] = pk @ rot.T + cpos[k]
        vel[2 * k:2 * k + 2] = vk @ rot.T + cvel[k]
    mass[2 * n_binaries:] = m[2 * n_binaries:]
    pos[2 * n_binaries:] = cpos[n_binaries:]
    vel[2 * n_binaries:] = cvel[n_binaries:]
    order = rng.permutation(n)                                    # caller index c holds body order[c]
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    planted = np.stack([inv[0:2 * n_binaries:2].astype(np.float64), inv[1:2 * n_binaries:2].astype(np.float64), a, e], axis=1)
    return mass[order], pos[order], vel[order], planted.reshape(-1, 4)
