"""The numpy twin of bh_spanning_tree / bh_spanning_tree_subsets (include/bhgpu.h) and of BarnesHutEngine.mass_segregation (no test
in here): brute force over every pair.

  d2 = dx * dx + dy * dy with dx = x_j - x_i, dy = y_j - y_i, every operation an fp64 numpy ufunc of its own (nothing fused): the
  d2_block of tests/neighbours_ref.py;
  the edges of the complete graph in the strict total order (d2, lo, hi), lo < hi the caller indices of the ends;
  the tree: Prim's algorithm, which picks the smallest edge, in that order, that leaves the tree -- under a strict order the
  minimum spanning tree is unique, so whatever the start it is THE tree; the edges are returned ascending in the order.

kruskal_py says the same in plain Python floats: every pair, `sorted` on tuples, a union-find; tests/test_mst_cpu.py holds the twin
to it."""
import math

import numpy as np

import neighbours_ref as NR


def tree(pos):
    """(lo (n - 1,) int64, hi (n - 1,) int64, d2 (n - 1,)) ascending in (d2, lo, hi); empty for n <= 1"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    n = len(pos)
    m = max(n - 1, 0)
    lo, hi, d2 = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m)
    if n <= 1:
        return lo, hi, d2
    ids = np.arange(n, dtype=np.int64)
    out = np.ones(n, dtype=bool)                 # not yet in the tree
    key_d = np.full(n, np.inf)                   # the smallest edge of every outside body into the tree: (key_d, key_lo, key_hi)
    key_lo = np.full(n, n, dtype=np.int64)
    key_hi = np.full(n, n, dtype=np.int64)
    cur = 0
    out[0] = False
    for e in range(m):
        d = NR.d2_block(pos, pos[cur:cur + 1])[0]
        a, b = np.minimum(ids, cur), np.maximum(ids, cur)
        better = out & ((d < key_d) | ((d == key_d) & ((a < key_lo) | ((a == key_lo) & (b < key_hi)))))
        key_d[better], key_lo[better], key_hi[better] = d[better], a[better], b[better]
        cand = np.nonzero(out)[0]
        cand = cand[key_d[cand] == key_d[cand].min()]
        pick = cand[np.lexsort((key_hi[cand], key_lo[cand]))[0]] if len(cand) > 1 else cand[0]
        lo[e], hi[e], d2[e] = key_lo[pick], key_hi[pick], key_d[pick]
        out[pick] = False
        cur = int(pick)
    order = np.lexsort((hi, lo, d2))
    return lo[order], hi[order], d2[order]


def labels_at(n, lo, hi, d2, b):
    """(label (n,) int64 = the smallest index of the component of the edges with d2 <= b * b, the number of components)"""
    b2 = float(b) * float(b)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    used = 0
    for a, c, d in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(d2).tolist()):
        if d <= b2:
            ra, rc = find(a), find(c)
            assert ra != rc                       # (a tree: no edge closes a cycle)
            parent[max(ra, rc)] = min(ra, rc)
            used += 1
    return np.array([find(i) for i in range(n)], dtype=np.int64).reshape(n), n - used


def subset_trees(pos, members):
    """(lo, hi, d2), each (n_sets, k - 1): the tree of every row's bodies alone, in caller indices, each row ascending"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    members = np.asarray(members, dtype=np.int64)
    sets, k = members.shape
    lo, hi, d2 = (np.zeros((sets, k - 1), dtype=np.int64), np.zeros((sets, k - 1), dtype=np.int64), np.zeros((sets, k - 1)))
    for r in range(sets):
        row = members[r]
        # the order of the row's own tree is by caller index, not by place in the row: build it on the row sorted by index
        srt = np.sort(row)
        assert (srt[1:] != srt[:-1]).all()
        a, b, d = tree(pos[srt])
        lo[r], hi[r], d2[r] = srt[a], srt[b], d
    return lo, hi, d2


def segregation_sets(weights, n_massive, n_random, seed):
    """(1 + n_random, n_massive) int64: the bodies of largest weight (ties to the smaller index), then the random sets"""
    w = np.asarray(weights, dtype=np.float64)
    n = len(w)
    massive = sorted(range(n), key=lambda i: (-w[i], i))[:n_massive]
    rows = [np.array(massive, dtype=np.int64)]
    rows += [np.random.default_rng([seed, r]).choice(n, n_massive, replace=False).astype(np.int64) for r in range(n_random)]
    return np.stack(rows)


def mass_segregation(pos, weights, n_massive, n_random=500, seed=0):
    """(ratio, sigma, l_massive, l_random (n_random,), members)"""
    members = segregation_sets(weights, n_massive, n_random, seed)
    d2 = subset_trees(pos, members)[2]
    l = [math.fsum(math.sqrt(x) for x in row.tolist()) for row in d2]
    l_massive, l_random = l[0], l[1:]
    mean = math.fsum(l_random) / n_random
    std = math.sqrt(math.fsum((x - mean) * (x - mean) for x in l_random) / n_random)
    return mean / l_massive, std / l_massive, l_massive, np.array(l_random), members


# ---- the same in plain Python: every pair, sorted, Kruskal ------------------------------------------------------------------------
def kruskal_py(pos):
    pts = [(float(x), float(y)) for x, y in np.asarray(pos, dtype=np.float64).reshape(-1, 2)]
    n = len(pts)
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            dx = pts[j][0] - pts[i][0]
            dy = pts[j][1] - pts[i][1]
            edges.append((dx * dx + dy * dy, i, j))
    edges.sort()
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    out = []
    for d, i, j in edges:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[ri] = rj
            out.append((d, i, j))
    m = len(out)
    return (np.array([e[1] for e in out], dtype=np.int64).reshape(m), np.array([e[2] for e in out], dtype=np.int64).reshape(m),
            np.array([e[0] for e in out], dtype=np.float64).reshape(m))
