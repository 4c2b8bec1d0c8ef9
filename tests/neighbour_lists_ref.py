"""The numpy twin of bh_neighbour_lists (include/bhgpu.h; no test in here): brute force over every (query, body) pair.

  d2 = dx * dx + dy * dy as tests/neighbours_ref.py forms it (d2_block: every operation an fp64 numpy ufunc of its own);
  row r: the bodies with d2 <= radius_r * radius_r, the query's own index dropped for a body query and nobody else, in the order
  (d2, caller index j) -- np.lexsort on (j, d2);
  offsets: the exclusive prefix of the row lengths.

lists_py says the same in plain Python floats and `sorted` on (d2, j) tuples; tests/test_neighbour_lists_cpu.py holds the numpy
version to it."""
import numpy as np

import neighbours_ref as R

_BLOCK = R._BLOCK


def _radii(radius, q):
    """(q,) squared radii: a scalar for every query, or one per query; each product formed once in fp64"""
    rad = np.asarray(radius, dtype=np.float64)
    assert rad.ndim == 0 or rad.shape == (q,), rad.shape
    return np.broadcast_to(rad * rad, (q,))


def lists(pos, radius, points=None, rows=None):
    """(offsets (q + 1,) int64, idx int64, d2 float64) of the body queries (points None) or of `points`; rows: only these
    queries (with per-query radii: radius[rows])."""
    q_all = len(np.asarray(pos).reshape(-1, 2)) if points is None else len(np.asarray(points).reshape(-1, 2))
    r2 = _radii(radius, q_all)
    pos, q, self_of = R._queries(pos, points, rows)
    if rows is not None:
        r2 = r2[np.asarray(rows, dtype=np.int64)]
    idx, out, lens = [], [], np.zeros(len(q), dtype=np.int64)
    if len(pos):
        for r0 in range(0, len(q), _BLOCK):
            d2 = R.d2_block(pos, q[r0:r0 + _BLOCK])
            for r in range(len(d2)):
                cand = np.nonzero(d2[r] <= r2[r0 + r])[0]
                cand = cand[cand != self_of[r0 + r]]
                order = cand[np.lexsort((cand, d2[r, cand]))]
                idx.append(order)
                out.append(d2[r, order])
                lens[r0 + r] = len(order)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (offsets, np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, dtype=np.int64),
            np.concatenate(out).astype(np.float64) if out else np.zeros(0))


def pairs(offsets, idx, d2):
    """(lo, hi, d2) of body queries with one radius: every unordered pair once, lo < hi, ascending in (lo, hi)"""
    got = []
    for i in range(len(offsets) - 1):
        for e in range(int(offsets[i]), int(offsets[i + 1])):
            if i < idx[e]:
                got.append((i, int(idx[e]), float(d2[e])))
    got.sort()
    return (np.array([g[0] for g in got], dtype=np.int64), np.array([g[1] for g in got], dtype=np.int64),
            np.array([g[2] for g in got], dtype=np.float64))


# ---- the same in plain Python -------------------------------------------------------------------------------------------------
def lists_py(pos, radius, points=None):
    pos = [(float(x), float(y)) for x, y in np.asarray(pos, dtype=np.float64).reshape(-1, 2)]
    qs = pos if points is None else [(float(x), float(y)) for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    rad = np.asarray(radius, dtype=np.float64)
    offsets, idx, out = [0], [], []
    for i, q in enumerate(qs):
        r = float(rad) if rad.ndim == 0 else float(rad[i])
        r2 = r * r
        c = sorted((R._d2_py(p, q), j) for j, p in enumerate(pos) if (points is not None or j != i) and R._d2_py(p, q) <= r2)
        idx += [j for _, j in c]
        out += [d for d, _ in c]
        offsets.append(len(idx))
    return np.array(offsets, dtype=np.int64), np.array(idx, dtype=np.int64), np.array(out, dtype=np.float64)


def components(n, lo, hi):
    """label (n,) int64 of the graph's components, each named by its smallest member: a small union-find"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(lo.tolist(), hi.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def r8_of(pos):
    """the square root of the median 8th-neighbour d2"""
    return float(np.sqrt(np.median(R.neighbours(pos, 8)[1][:, 7])))
