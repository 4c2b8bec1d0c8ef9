"""The numpy twin of bh_groups / bh_groups_catalogue (include/bhgpu.h; no test in here): friends by brute force over every pair,
components by a plain union-find.

  d2 = dx * dx + dy * dy with dx = x_j - x_i, dy = y_j - y_i, every operation an fp64 numpy ufunc of its own (nothing fused);
  i and j are friends when d2 <= b * b (the product formed once);
  a group is a connected component, its label the smallest caller index in it;
  the catalogue: the groups with at least min_members bodies, the sums of m, m x, m y, m vx, m vy over their members in the fixed
  point of the header -- np.rint(np.ldexp(q, 62 - E_p - L)).astype(np.int64) summed as integers -- in the order (count
  descending, label ascending).

groups_py says the same in plain Python floats and a breadth-first search; tests/test_groups_cpu.py holds the twin to it."""
import collections
import functools
import math

import numpy as np

_BLOCK = 256                      # rows per d2 block


def friend_pairs(pos, b):
    """(i, j) int64 arrays of all friend pairs with i < j"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    b2 = float(b) * float(b)
    n = len(pos)
    ii, jj = [], []
    for r0 in range(0, n, _BLOCK):
        q = pos[r0:r0 + _BLOCK]
        dx = pos[None, :, 0] - q[:, None, 0]
        dy = pos[None, :, 1] - q[:, None, 1]
        i, j = np.nonzero(dx * dx + dy * dy <= b2)
        i = i + r0
        keep = i < j
        ii.append(i[keep])
        jj.append(j[keep])
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


def components(n, ii, jj):
    """label (n,) int64 = the smallest index of the component, from a plain union-find over the pairs"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, c in zip(ii.tolist(), jj.tolist()):
        ra, rc = find(a), find(c)
        if ra != rc:
            if ra < rc:
                parent[rc] = ra
            else:
                parent[ra] = rc
    # (hooking the larger root under the smaller: a root is the smallest index of its tree)
    return np.array([find(i) for i in range(n)], dtype=np.int64).reshape(n)


def groups(pos, b):
    """(label (n,) int64, n_groups, number of friend pairs)"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    ii, jj = friend_pairs(pos, b)
    label = components(len(pos), ii, jj)
    return label, int(len(np.unique(label))), int(len(ii))


def exponents(q, n):
    """the five exponents 62 - E_p - L of the moments q (n, 5); 0 where the maximum is 0"""
    L = 0 if n <= 1 else (int(n) - 1).bit_length()
    e = np.zeros(5, dtype=np.int32)
    for p in range(5):
        m = float(np.abs(q[:, p]).max()) if len(q) else 0.0
        if m != 0.0:
            e[p] = 62 - int(np.frexp(m)[1]) - L
    return e


def moments(pos, vel, mass):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    return np.stack([m, m * pos[:, 0], m * pos[:, 1], m * vel[:, 0], m * vel[:, 1]], axis=1)


def catalogue(pos, vel, mass, label, min_members):
    """(ids (g,), counts (g,), sums (g, 5) int64, exponents (5,) int32) in the order (count descending, id ascending)"""
    label = np.asarray(label, dtype=np.int64)
    q = moments(pos, vel, mass)
    n = len(label)
    e = exponents(q, n)
    contrib = np.stack([np.rint(np.ldexp(q[:, p], int(e[p]))).astype(np.int64) for p in range(5)], axis=1).reshape(n, 5)
    ids, inverse, counts = np.unique(label, return_inverse=True, return_counts=True)
    sums = np.zeros((len(ids), 5), dtype=np.int64)
    np.add.at(sums, inverse, contrib)
    keep = counts >= min_members
    ids, counts, sums = ids[keep], counts[keep].astype(np.int64), sums[keep]
    order = np.lexsort((ids, -counts))
    return ids[order].astype(np.int64), counts[order], sums[order], e


def kth_neighbour_distance(pos, k):
    """(n,): the distance of every body to its k-th nearest other body (brute force, the operations of d2)"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    n = len(pos)
    out = np.empty(n)
    for r0 in range(0, n, _BLOCK):
        q = pos[r0:r0 + _BLOCK]
        dx = pos[None, :, 0] - q[:, None, 0]
        dy = pos[None, :, 1] - q[:, None, 1]
        d2 = dx * dx + dy * dy
        d2[np.arange(len(q)), np.arange(r0, r0 + len(q))] = np.inf
        out[r0:r0 + len(q)] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return out


# ---- the same in plain Python: breadth-first search from every unvisited body ---------------------------------------------------
def groups_py(pos, b):
    pts = [(float(x), float(y)) for x, y in np.asarray(pos, dtype=np.float64).reshape(-1, 2)]
    n = len(pts)
    b2 = float(b) * float(b)
    label = [-1] * n
    n_groups = 0
    for start in range(n):                    # ascending: the start is the smallest index of its component
        if label[start] >= 0:
            continue
        n_groups += 1
        label[start] = start
        queue = collections.deque([start])
        while queue:
            i = queue.popleft()
            for j in range(n):
                if label[j] < 0:
                    dx = pts[j][0] - pts[i][0]
                    dy = pts[j][1] - pts[i][1]
                    if dx * dx + dy * dy <= b2:
                        label[j] = start
                        queue.append(j)
    return np.array(label, dtype=np.int64).reshape(n), n_groups


# ---- fixtures shared by the CPU and GPU tests -----------------------------------------------------------------------------------
def spiral(n, b, seed=17, gap=None):
    """(pos (n or n - 1, 2), order): an Archimedean spiral whose neighbouring bodies lie 0.9 b apart along the arm and whose
    arms are 4 b apart, in a caller order shuffled with `seed`; order[c] is the place along the arm of caller index c.
    gap: the body at that place along the arm is left out (the bodies around it are then 1.8 b apart).

    r = a * theta with a = 4 b / (2 pi); the places are set by arc length: theta_k solves s(theta) = 0.9 b * (k + k0) with
    s(theta) = a / 2 * (theta * sqrt(1 + theta^2) + asinh(theta)), by Newton's method; k0 keeps the first body away from the
    tightly wound centre.  A chord is at most its arc (0.9 b) and, the curvature being small out there, at least 0.89 b."""
    a = 4.0 * b / (2.0 * math.pi)
    ds = 0.9 * b

    def arc(t):
        return 0.5 * a * (t * math.sqrt(1.0 + t * t) + math.asinh(t))

    k0 = int(math.ceil(arc(4.0 * math.pi) / ds))              # start two turns out
    pts = []
    t = 4.0 * math.pi
    for k in range(n):
        target = ds * (k + k0)
        for _ in range(50):
            step = (arc(t) - target) / (a * math.sqrt(1.0 + t * t))
            t -= step
            if abs(step) < 1e-15 * t:
                break
        pts.append((a * t * math.cos(t), a * t * math.sin(t)))
    along = np.array(pts)
    place = np.arange(n)
    if gap is not None:
        along = np.delete(along, gap, axis=0)
        place = np.delete(place, gap)
    order = np.random.default_rng(seed).permutation(len(along))
    return along[order], place[order]


@functools.lru_cache(maxsize=None)
def uniform_square(n, seed):
    pos = np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 2))
    pos.setflags(write=False)
    return pos
