"""Reference field at arbitrary points for the tests of bh_field_at: the numpy walk of tests/potential_ref.py over the
oracle's node array (reference order, oracle.bh_oracle.build_tree), extended from the potential to everything the
checks need.  Helper of tests/test_field_cpu.py, tests/test_gpu_field.py and (the deep chain) tests/test_gpu_energy.py -- not a
test file.

A point is nobody, so no leaf is skipped.  Per node (project.cu:617-658 with m_i = 1):

    skip a node of mass <= 1e-15; d2 = dx*dx + dy*dy, d = sqrt(d2) + 1e-15; size = max(xmax - xmin, ymax - ymin);
    a leaf (all children -1) or size / d < theta is taken: f = (G*M)/d2, a += f*(dx/d, dy/d), phi -= (G*M)/d;
    otherwise its children are opened.

All points walk together, level by level: a frontier of (point, node) pairs.  Besides the sums, per point: the number
of taken nodes, sum |a_j|, sum G*M/d_j (the scales of the forward error bound below) and the smallest
|size/d - theta| / theta met on a subdivided cell (how far the point is from a decision that rounding could turn)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import bh_oracle as O


@dataclass
class FieldRef:
    accel: np.ndarray        # (k, 2)
    phi: np.ndarray          # (k,)
    counts: np.ndarray       # terms taken
    abs_sum: np.ndarray      # sum of |a_j| over the taken nodes
    pot_sum: np.ndarray      # sum of G M_j / d_j over the taken nodes
    margin: np.ndarray       # min over the subdivided cells met of |size/d - theta| / theta (inf: none met)


def field_walk(nodes, points, theta=0.5, G=6.67e-11) -> FieldRef:
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    k = pts.shape[0]
    child = nodes["child"].astype(np.int64)
    leaf_all = (child == -1).all(axis=1)
    size_all = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    ax, ay, phi, asum, psum = (np.zeros(k) for _ in range(5))
    cnt = np.zeros(k, dtype=np.int64)
    margin = np.full(k, np.inf)
    b = np.arange(k)
    nd = np.zeros(k, dtype=np.int64)
    if len(nodes) == 0:
        b = b[:0]
    while b.size:
        m = nodes["mass"][nd]
        keep = m > 1e-15
        b, nd, m = b[keep], nd[keep], m[keep]
        dx = nodes["comx"][nd] - pts[b, 0]
        dy = nodes["comy"][nd] - pts[b, 1]
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2) + 1e-15
        leaf = leaf_all[nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = size_all[nd] / d
            take = leaf | (ratio < theta)
            np.minimum.at(margin, b[~leaf], np.abs(ratio[~leaf] - theta) / theta)
            bt, gm = b[take], G * m[take]
            f = gm / d2[take]
            tx, ty = f * (dx[take] / d[take]), f * (dy[take] / d[take])
            tp = gm / d[take]
        ax += np.bincount(bt, weights=tx, minlength=k)
        ay += np.bincount(bt, weights=ty, minlength=k)
        phi -= np.bincount(bt, weights=tp, minlength=k)
        asum += np.bincount(bt, weights=np.hypot(tx, ty), minlength=k)
        psum += np.bincount(bt, weights=tp, minlength=k)
        cnt += np.bincount(bt, minlength=k)
        op = ~take
        ch = child[nd[op]].reshape(-1)
        bo = np.repeat(b[op], 4)
        ok = ch >= 0
        b, nd = bo[ok], ch[ok]
    return FieldRef(np.stack([ax, ay], axis=1), phi, cnt, asum, psum, margin)


def oracle_at_points(nodes, pos, mass, points, theta=0.5, G=6.67e-11, compat=True, **diag_kw) -> O.WalkDiag:
    """The pinned oracle's walk of `points` through a tree of the bodies only: the points are appended after the n bodies
    with unit masses and rows [n, n + k) are walked -- an index >= n matches no occupant, so neither self skip fires, and
    mass 1 makes the force the acceleration.  Returns the WalkDiag rows of the points (forces = accelerations)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n, k = len(pos), len(pts)
    pe = np.concatenate([pos, pts])
    me = np.concatenate([np.asarray(mass, dtype=np.float64), np.ones(k)])
    d = O.compute_forces_diag(nodes, pe, me, theta=theta, G=G, compat_self_skip=compat, lo=n, hi=n + k, **diag_kw)
    return O.WalkDiag(d.forces[n:], d.counts[n:], d.abs_sum[n:], d.coord[n:], d.flip[n:], d.cap[n:])


def accel_bound(counts, abs_sum):
    """|a - a_ref| <= (count + 16) * 2^-52 * sum |a_j|: two sequential fp64 sums of `count` terms (each within
    (count - 1) * 2^-53 * sum |a_j| of the exact sum of its own terms) plus a fixed budget of roundings per term on
    both sides (32 * 2^-53).  The same form with sum G M / d_j bounds the potential."""
    return (np.asarray(counts, dtype=np.float64) + 16.0) * 2.0 ** -52 * np.asarray(abs_sum)


# ---- inputs shared by the CPU and the GPU tests --------------------------------------------------------------------
def clumped(n, seed):
    """Three Gaussian clumps of different widths and a thin uniform background; masses in [0.1, 0.5)."""
    rng = np.random.default_rng(seed)
    parts = [rng.normal((-0.05, 0.02), 0.004, (n // 3, 2)), rng.normal((0.06, -0.03), 0.0005, (n // 3, 2)),
             rng.normal((0.0, 0.07), 0.02, (n // 6, 2))]
    parts.append(rng.uniform(-0.1, 0.1, (n - sum(len(q) for q in parts), 2)))
    return np.concatenate(parts), rng.uniform(0.1, 0.5, n)


def points_around(pos, k, seed):
    """k points in, on the edge of and outside the bounding box of `pos`: a third uniform over the box, a third uniform
    over the box enlarged threefold, the four corners and edge midpoints, and bodies jittered by 1 % of the box."""
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    mid, ext = 0.5 * (lo + hi), hi - lo
    edge = np.array([[lo[0], lo[1]], [lo[0], hi[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], mid[1]], [hi[0], mid[1]],
                     [mid[0], lo[1]], [mid[0], hi[1]]])
    a = k // 3
    inside = rng.uniform(lo, hi, (a, 2))
    wide = rng.uniform(mid - 1.5 * ext, mid + 1.5 * ext, (a, 2))
    near = pos[rng.integers(0, len(pos), k - 2 * a - len(edge))] + rng.normal(0.0, 0.01, (k - 2 * a - len(edge), 1)) * ext
    return np.concatenate([inside, wide, edge, near])


def plummer_disc(n, seed, scale=0.02, rmax=1.0):
    """n equal-mass bodies on a disc, radii from the Plummer law of the given scale truncated at rmax; positions and
    masses rounded to fp32."""
    rng = np.random.default_rng(seed)
    r = np.empty(0)
    while len(r) < n:
        u = rng.uniform(0.0, 1.0, 2 * n)
        q = scale / np.sqrt(np.maximum(u ** (-2.0 / 3.0) - 1.0, 1e-300))
        r = np.concatenate([r, q[q < rmax]])
    r = r[:n]
    ph = rng.uniform(0.0, 2.0 * np.pi, n)
    p = np.stack([r * np.cos(ph), r * np.sin(ph)], axis=1).astype(np.float32).astype(np.float64)
    m = np.full(n, np.float32(1.0 / n), dtype=np.float64)
    return p, m


def class_points(pos, k, seed):
    """k fp32-rounded points: half uniform over the bounding box enlarged by 20 % on each side, half bodies jittered by
    N(0, 0.004)."""
    rng = np.random.default_rng(1000 + seed)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = hi - lo
    a = k // 2
    u = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (a, 2))
    j = pos[rng.integers(0, len(pos), k - a)] + rng.normal(0.0, 0.004, (k - a, 2))
    return np.concatenate([u, j]).astype(np.float32).astype(np.float64)


# ---- the deep chain: an input whose walks need the second tier of the kernels' lane stack -----------------------------
DEEP_THETA, DEEP_DEPTH = 0.2, 32
DEEP_POINT = np.array([[-1e-10, -1e-10]])


def deep_chain(levels=28):
    """172 bodies of mass 0.3.  Anchors at (-1, -1) and (1, 1) pad the root box to [-1.2, 1.2]^2, centre at the origin.  For
    l = 1 .. levels the cell [-s, 0]^2, s = 1.2 * 2^-l, has two bodies in each of its three children other than the
    upper-right one, at (0.3, 0.3) and (0.7, 0.6) of the child's extent, and the last upper-right child holds two more: a
    walker next to the origin opens the upper-right child of every level last and leaves its three siblings pending."""
    at = np.array([[0.3, 0.3], [0.7, 0.6]])
    pos = [np.array([[-1.0, -1.0], [1.0, 1.0]])]
    for l in range(1, levels + 1):
        h = 1.2 * 2.0 ** -l / 2.0                                  # extent of the children of [-s, 0]^2
        for cx, cy in ((-2.0 * h, -2.0 * h), (-h, -2.0 * h), (-2.0 * h, -h)):
            pos.append(np.array([cx, cy]) + at * h)
    pos.append(np.array([-h, -h]) + at * h)
    pos = np.concatenate(pos)
    return pos, np.full(len(pos), 0.3)


def pending_quads(nodes, point, theta, self_index=-1):
    """(most sibling quads pending at once, terms taken) of one walker's depth-first walk as the side-walk kernels run it
    (csrc/bh_treewalk.hpp): the root alone, then quads popped last first, their siblings in index order, every opened
    cell's quad pushed.  A wavefront's stack is at least its deepest lane's: same sibling order, a superset pushed."""
    child = nodes["child"].astype(np.int64)
    size = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    stack, deepest, terms = [], 0, 0

    def visit(nd):
        nonlocal deepest, terms
        if not nodes["mass"][nd] > 1e-15:
            return
        dx, dy = nodes["comx"][nd] - point[0], nodes["comy"][nd] - point[1]
        d = np.sqrt(dx * dx + dy * dy) + 1e-15
        if (child[nd] == -1).all():
            terms += int(nodes["particle"][nd]) != self_index
        elif size[nd] / d < theta:
            terms += 1
        else:
            stack.append(child[nd])
            deepest = max(deepest, len(stack))

    visit(0)
    while stack:
        for nd in stack.pop():
            if nd >= 0:
                visit(nd)
    return deepest, terms
