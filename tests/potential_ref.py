"""Reference potential for the diagnostics tests: a numpy walk over the oracle's node array (reference order,
oracle.bh_oracle.build_tree) with the reference's criterion and term set, project.cu:617-658:

    skip a node of mass <= 1e-15; d2 = dx*dx + dy*dy, d = sqrt(d2) + 1e-15; size = max(xmax - xmin, ymax - ymin);
    a leaf (all children -1) or size / d < theta is taken unless it is the body's own leaf (occ == i, or
    occ + 2 == -i with compat); otherwise its children are opened.

phi_i = -G * sum over the taken nodes of M / d, and the number of taken nodes per body.  All bodies (or the `bodies`
subset) walk together, level by level: a frontier of (body, node) pairs."""
from __future__ import annotations

import numpy as np


def potential_walk(nodes, pos, theta=0.5, G=6.67e-11, compat=True, bodies=None):
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    bodies = np.arange(n) if bodies is None else np.asarray(bodies, dtype=np.int64)
    k = len(bodies)
    child = nodes["child"].astype(np.int64)
    leaf_all = (child == -1).all(axis=1)
    size_all = np.maximum(nodes["xmax"] - nodes["xmin"], nodes["ymax"] - nodes["ymin"])
    occ_all = nodes["particle"].astype(np.int64)
    phi = np.zeros(k)
    cnt = np.zeros(k, dtype=np.int64)
    b = np.arange(k)                      # index into `bodies`
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
        leaf = leaf_all[nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = leaf | (size_all[nd] / d < theta)
        occ = occ_all[nd]
        self_ = leaf & ((occ == i) | (compat & (occ + 2 == -i)))
        take = acc & ~self_
        phi += np.bincount(b[take], weights=m[take] / d[take], minlength=k)
        cnt += np.bincount(b[take], minlength=k)
        op = ~acc
        ch = child[nd[op]]
        bo = np.repeat(b[op], 4)
        ch = ch.reshape(-1)
        ok = ch >= 0
        b, nd = bo[ok], ch[ok]
    return -G * phi, cnt
