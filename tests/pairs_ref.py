"""The numpy twin of bh_pair_counts (include/bhgpu.h) (no test in here): brute force over every pair.

  d2 = dx * dx + dy * dy with dx = x_j - q.x, dy = y_j - q.y, every operation an fp64 numpy ufunc of its own (nothing fused);
  e2 = edges * edges; the bin of a d2 is np.searchsorted(e2, d2, side="left"): 0 for d2 <= e2[0] ("below"), k + 1 for
  e2[k] < d2 <= e2[k + 1], nb + 1 for d2 > e2[nb] ("beyond");
  auto mode (points None): every unordered pair i < j of the bodies once; cross mode: every (point, body) combination.

pair_counts_py says the same in plain Python floats and loops; tests/test_pairs_cpu.py holds the numpy version to it."""
import numpy as np

MAX_BINS = 1024
_BLOCK_D2 = 1 << 21               # d2 per block: 16 MiB of doubles


def squared_edges(edges):
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    assert 1 <= len(e) - 1 <= MAX_BINS and np.isfinite(e).all() and (e >= 0).all() and (np.diff(e) > 0).all()
    e2 = e * e
    assert np.isfinite(e2).all() and (np.diff(e2) > 0).all()
    return e2


def pair_counts(pos, edges, points=None):
    """int64[nb + 2]: below, the nb bins, beyond"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    e2 = squared_edges(edges)
    out = np.zeros(len(e2) + 1, dtype=np.int64)
    q = pos if points is None else np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(pos) == 0:
        return out
    block = max(1, _BLOCK_D2 // len(pos))
    for r0 in range(0, len(q), block):
        rows = q[r0:r0 + block]
        dx = pos[None, :, 0] - rows[:, None, 0]
        dy = pos[None, :, 1] - rows[:, None, 1]
        d2 = dx * dx + dy * dy
        if points is None:                                        # the pairs (r, j) with j < r
            keep = np.arange(len(pos))[None, :] < (r0 + np.arange(len(rows)))[:, None]
            d2 = d2[keep]
        out += np.bincount(np.searchsorted(e2, d2.reshape(-1), side="left"), minlength=len(out))
    return out


def pair_counts_py(pos, edges, points=None):
    """The same in plain Python."""
    pos = [(float(x), float(y)) for x, y in np.asarray(pos, dtype=np.float64).reshape(-1, 2)]
    e2 = [float(e) * float(e) for e in np.asarray(edges, dtype=np.float64).reshape(-1)]
    out = [0] * (len(e2) + 1)

    def add(p, qq):
        dx, dy = p[0] - qq[0], p[1] - qq[1]
        d2 = dx * dx + dy * dy
        k = 0
        while k < len(e2) and e2[k] < d2:
            k += 1
        out[k] += 1

    if points is None:
        for i in range(len(pos)):
            for j in range(i):
                add(pos[j], pos[i])
    else:
        for qq in [(float(x), float(y)) for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]:
            for p in pos:
                add(p, qq)
    return np.array(out, dtype=np.int64)
