"""Plummer-softened forms of the numpy reference walks -- a helper of tests/test_soft_cpu.py and tests/test_gpu_soft.py, not
a test file.

Softening length eps >= 0 (bh_set_softening, include/bhgpu.h).  With d2 = dx*dx + dy*dy the geometric squared distance
and s2 = d2 + eps*eps, every walk below makes the DECISIONS of its unsoftened sibling on the geometric d = sqrt(d2) + 1e-15
(the mass cut-off, leaf or size / d < theta, the self skip by occupant index) and takes only the magnitude of an accepted
term at s2: ds = sqrt(s2) + 1e-15, f = (G M) / s2, a += f * (dx / ds), phi -= (G M) / ds.  Same traversal, same order of
the operations: at eps = 0, s2 = d2 + 0.0 is d2 bit for bit and every function returns the bits of its sibling
(tests/field_ref.py, tests/potential_ref.py, tests/forest_potential_ref.py, tests/direct_ref.py).

soft_field_walk also serves the bodies themselves: self_of[k] names the body standing at points[k], whose own leaf is
skipped as the force walks skip it (occ == i, or occ + 2 == -i with compat); the force on body i is then m_i * accel."""
from __future__ import annotations

import numpy as np

from oracle import bh_oracle as O
from box_ref import box_ref
from field_ref import FieldRef


def node_depths(nodes):
    """Depth of every node of a reference-order node array (root 0) from the child links."""
    child = nodes["child"].astype(np.int64)
    depth = np.zeros(len(nodes), dtype=np.int64)
    level = np.array([0], dtype=np.int64) if len(nodes) else np.zeros(0, dtype=np.int64)
    while level.size:
        ch = child[level].reshape(-1)
        par = np.repeat(level, 4)
        ok = ch >= 0
        depth[ch[ok]] = depth[par[ok]] + 1
        level = ch[ok]
    return depth


def soft_field_walk(nodes, points, theta=0.5, G=6.67e-11, eps=0.0, self_of=None, compat=True, cap_depth=0) -> FieldRef:
    """field_ref.field_walk with softened terms; abs_sum / pot_sum are the sums of the softened |a_j| and G M / ds_j.
    cap_depth > 0 (an uncapped tree): a subdivided cell at depth >= cap_depth - 1 is never accepted -- the fp32 walks' bucket
    leaves of a tree built with max_depth = cap_depth and reference_compat off, summed body by body."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    k = pts.shape[0]
    eps2 = float(eps) * float(eps)
    child = nodes["child"].astype(np.int64)
    leaf_all = (child == -1).all(axis=1)
    size_all = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    occ_all = nodes["particle"].astype(np.int64)
    who = None if self_of is None else np.asarray(self_of, dtype=np.int64)
    ax, ay, phi, asum, psum = (np.zeros(k) for _ in range(5))
    cnt = np.zeros(k, dtype=np.int64)
    margin = np.full(k, np.inf)
    forced = (node_depths(nodes) >= cap_depth - 1) if cap_depth > 0 else np.zeros(len(nodes), dtype=bool)
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
        s2 = d2 + eps2
        ds = np.sqrt(s2) + 1e-15
        leaf = leaf_all[nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = size_all[nd] / d
            acc = leaf | ((ratio < theta) & ~forced[nd])
            np.minimum.at(margin, b[~leaf], np.abs(ratio[~leaf] - theta) / theta)
            take = acc
            if who is not None:
                occ, i = occ_all[nd], who[b]
                take = acc & ~(leaf & ((occ == i) | (compat & (occ + 2 == -i))))
            bt, gm = b[take], G * m[take]
            f = gm / s2[take]
            tx, ty = f * (dx[take] / ds[take]), f * (dy[take] / ds[take])
            tp = gm / ds[take]
        ax += np.bincount(bt, weights=tx, minlength=k)
        ay += np.bincount(bt, weights=ty, minlength=k)
        phi -= np.bincount(bt, weights=tp, minlength=k)
        asum += np.bincount(bt, weights=np.hypot(tx, ty), minlength=k)
        psum += np.bincount(bt, weights=tp, minlength=k)
        cnt += np.bincount(bt, minlength=k)
        op = ~acc
        ch = child[nd[op]].reshape(-1)
        bo = np.repeat(b[op], 4)
        ok = ch >= 0
        b, nd = bo[ok], ch[ok]
    return FieldRef(np.stack([ax, ay], axis=1), phi, cnt, asum, psum, margin)


def soft_potential_walk(nodes, pos, theta=0.5, G=6.67e-11, compat=True, bodies=None, eps=0.0):
    """potential_ref.potential_walk with the term M / (sqrt(d2 + eps^2) + 1e-15): (phi, counts)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    eps2 = float(eps) * float(eps)
    bodies = np.arange(n) if bodies is None else np.asarray(bodies, dtype=np.int64)
    k = len(bodies)
    child = nodes["child"].astype(np.int64)
    leaf_all = (child == -1).all(axis=1)
    size_all = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    occ_all = nodes["particle"].astype(np.int64)
    phi = np.zeros(k)
    cnt = np.zeros(k, dtype=np.int64)
    b = np.arange(k)
    nd = np.zeros(k, dtype=np.int64)
    while b.size:
        m = nodes["mass"][nd]
        keep = m > 1e-15
        b, nd, m = b[keep], nd[keep], m[keep]
        i = bodies[b]
        dx = nodes["comx"][nd] - pos[i, 0]
        dy = nodes["comy"][nd] - pos[i, 1]
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2) + 1e-15
        ds = np.sqrt(d2 + eps2) + 1e-15
        leaf = leaf_all[nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = leaf | (size_all[nd] / d < theta)
        occ = occ_all[nd]
        self_ = leaf & ((occ == i) | (compat & (occ + 2 == -i)))
        take = acc & ~self_
        phi += np.bincount(b[take], weights=m[take] / ds[take], minlength=k)
        cnt += np.bincount(b[take], minlength=k)
        op = ~acc
        ch = child[nd[op]]
        bo = np.repeat(b[op], 4)
        ch = ch.reshape(-1)
        ok = ch >= 0
        b, nd = bo[ok], ch[ok]
    return -G * phi, cnt


def soft_forest_potential(m, p, parts, theta=0.5, G=6.67e-11, bodies=None, eps=0.0):
    """forest_potential_ref.forest_potential over soft_potential_walk: the own tree first, then the peers' in rank order."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n = len(m)
    parts = [np.asarray(ix, dtype=np.int64) for ix in parts]
    assert np.array_equal(np.sort(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64), np.arange(n)), "not a partition"
    box = box_ref(p)
    trees = [O.build_tree_box(p[ix], m[ix], box, 0) if len(ix) else None for ix in parts]
    wanted = np.ones(n, dtype=bool) if bodies is None else np.isin(np.arange(n), bodies)
    phi = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    for q, ix in enumerate(parts):
        local = np.flatnonzero(wanted[ix])
        if len(local):
            f, c = soft_potential_walk(trees[q], p[ix], theta=theta, G=G, compat=False, bodies=local, eps=eps)
            phi[ix[local]] += f
            cnt[ix[local]] += c
    owner = np.empty(n, dtype=np.int64)
    for q, ix in enumerate(parts):
        owner[ix] = q
    for r, ix in enumerate(parts):
        tg = np.flatnonzero(wanted & (owner != r))
        if not len(ix) or not len(tg):
            continue
        f, c = soft_potential_walk(trees[r], np.concatenate([p[ix], p[tg]]), theta=theta, G=G, compat=False,
                                   bodies=np.arange(len(ix), len(ix) + len(tg)), eps=eps)
        phi[tg] += f
        cnt[tg] += c
    if bodies is None:
        return phi, cnt
    bodies = np.asarray(bodies, dtype=np.int64)
    return phi[bodies], cnt[bodies]


def soft_direct_ref(pos, mass, targets, G: float = 6.67e-11, eps: float = 0.0) -> np.ndarray:
    """direct_ref.direct_ref with s2 = d2 + eps*eps, d = sqrt(s2), k = ((G*m_i)*m_j) / (s2*d): same order, j == i dropped
    by index."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    mass = np.asarray(mass, dtype=np.float64).reshape(-1)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    eps2 = float(eps) * float(eps)
    out = np.empty((len(targets), 2))
    for r, i in enumerate(targets):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dx = pos[:, 0] - pos[i, 0]
            d2 = 0.0 + dx * dx
            dy = pos[:, 1] - pos[i, 1]
            d2 = d2 + dy * dy
            s2 = d2 + eps2
            d = np.sqrt(s2)
            k = ((G * mass[i]) * mass) / (s2 * d)
            tx, ty = np.delete(k * dx, i), np.delete(k * dy, i)
            out[r, 0] = np.cumsum(np.concatenate(([0.0], tx)))[-1]
            out[r, 1] = np.cumsum(np.concatenate(([0.0], ty)))[-1]
    return out


def coord_scale(nodes, points, theta=0.5, G=6.67e-11, self_of=None, compat=True):
    """sum over the taken nodes of |a_j| (|comx| + |comy| + |px| + |py|) / d_j with the UNSOFTENED |a_j| = G M / d2 and the
    geometric d: the scale of what an fp32 rounding of the coordinates moves (oracle.WalkDiag.coord for unit masses).  A
    softened term and its derivative are no larger than the unsoftened ones, so the scale bounds the softened walk too."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    k = pts.shape[0]
    child = nodes["child"].astype(np.int64)
    leaf_all = (child == -1).all(axis=1)
    size_all = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    occ_all = nodes["particle"].astype(np.int64)
    who = None if self_of is None else np.asarray(self_of, dtype=np.int64)
    out = np.zeros(k)
    b = np.arange(k)
    nd = np.zeros(k, dtype=np.int64)
    while b.size:
        m = nodes["mass"][nd]
        keep = m > 1e-15
        b, nd, m = b[keep], nd[keep], m[keep]
        cx, cy = nodes["comx"][nd], nodes["comy"][nd]
        dx, dy = cx - pts[b, 0], cy - pts[b, 1]
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2) + 1e-15
        leaf = leaf_all[nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = leaf | (size_all[nd] / d < theta)
            take = acc
            if who is not None:
                occ, i = occ_all[nd], who[b]
                take = acc & ~(leaf & ((occ == i) | (compat & (occ + 2 == -i))))
            w = (G * m / d2) * (np.abs(cx) + np.abs(cy) + np.abs(pts[b, 0]) + np.abs(pts[b, 1])) / d
        out += np.bincount(b[take], weights=w[take], minlength=k)
        op = ~acc
        ch = child[nd[op]].reshape(-1)
        bo = np.repeat(b[op], 4)
        ok = ch >= 0
        b, nd = bo[ok], ch[ok]
    return out


def soft_forest_field(m, p, parts, theta=0.5, G=6.67e-11, eps=0.0) -> FieldRef:
    """The softened forest walk of the distributed step for every body, caller order: rank r holds the tree of ITS bodies under
    the root box of ALL bodies (uncapped); a body takes its terms from its own rank's tree with the self skip and from every
    other whole tree without one.  accel is per unit mass; counts, abs_sum, pot_sum are summed over the trees."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n = len(m)
    parts = [np.asarray(ix, dtype=np.int64) for ix in parts]
    box = box_ref(p)
    out = FieldRef(np.zeros((n, 2)), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n), np.full(n, np.inf))
    owner = np.empty(n, dtype=np.int64)
    for q, ix in enumerate(parts):
        owner[ix] = q
    for r, ix in enumerate(parts):
        if not len(ix):
            continue
        tree = O.build_tree_box(p[ix], m[ix], box, 0)
        others = np.flatnonzero(owner != r)
        for tg, who in ((ix, np.arange(len(ix))), (others, None)):
            if not len(tg):
                continue
            f = soft_field_walk(tree, p[tg], theta=theta, G=G, eps=eps, self_of=who, compat=False)
            out.accel[tg] += f.accel
            out.phi[tg] += f.phi
            out.counts[tg] += f.counts
            out.abs_sum[tg] += f.abs_sum
            out.pot_sum[tg] += f.pot_sum
            out.margin[tg] = np.minimum(out.margin[tg], f.margin)
    return out
