"""The whole-tree reference of the distributed step's forest walk, in fp64 on the CPU -- a helper of
tests/test_forest_ref_cpu.py and the tests/test_gpu_let_*.py modules, not a test file.

The distributed step (csrc/bh_let.hpp) gives every rank r the tree T_r of ITS bodies under the root box of ALL bodies, and
the force on body i of rank q is the sum of i's walks over T_0 .. T_{W-1}: its own tree with the self skip, and of every
other tree the part the bodies of q can open (the locally-essential tree).  A correct LET changes nothing: walking it
takes the terms that walking the whole of T_r takes.  So the reference has NO pruning anywhere -- forest_diag walks every
body through every WHOLE tree with the oracle's diagnostic walk (oracle/bh_oracle.c: bho_compute_forces_diag) and adds
forces, counts, abs_sum, coord, flip and cap over the trees.  tests/parity_classes.classify takes the result in place of
its single-tree walk.

  * the root box is ComputeRootBounds of all positions (tests/box_ref.py), T_r = O.build_tree_box of rank r's bodies in
    partition order, uncapped;
  * own tree: bodies [0, n_q) of T_q with cap_depth (a cell at the device's depth cap is a bucket, summed body by body);
  * another rank's tree T_r: the walked array is T_r's bodies followed by the targets, lo = n_r, so that no occupant
    index equals a target's index and the walk skips nothing;
  * remote_capped: the remote trees are the CAPPED trees build_tree_box(..., max_depth=cap_depth) -- the sender packs its
    depth-cap buckets as aggregates (let_pack_kernel: child = -1, thr = 0), which every remote body accepts whatever its
    distance, as the walk accepts the capped tree's depth-cap leaf.  Those aggregates carry a centre of mass that the
    device rounds to fp32, so their terms are priced like cells' (pos_rounded for the remote walks: an upper bound).

let_prune is the numpy statement of the LET rule, let_boxes the boxes a rank describes itself by."""
from __future__ import annotations

import numpy as np

from oracle import bh_oracle as O
from box_ref import box_ref

LET_BOXES = 8                 # kLetBoxes, csrc/bh_let.hpp


def rank_trees(m, p, parts, max_depth=0, box=None):
    """(global box, [T_r]): every rank's tree of its own bodies, in partition order, under the box of all bodies."""
    box = box_ref(p) if box is None else box
    return box, [O.build_tree_box(p[ix], m[ix], box, max_depth) for ix in parts]


def forest_diag(m, p, parts, theta, cap_depth=21, pos_rounded=False, remote_capped=False, G=6.67e-11, trees=None,
                threads=0) -> O.WalkDiag:
    """Per-body diagnostics of the forest walk of all len(m) bodies, caller order.  parts: list of index arrays, a
    partition of range(len(m)) (empty ranks allowed).  trees: (box, [T_r]) of rank_trees, if already built."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n = len(m)
    parts = [np.asarray(ix, dtype=np.int64) for ix in parts]
    assert np.array_equal(np.sort(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64), np.arange(n)), "not a partition"
    box, own_trees = trees if trees is not None else rank_trees(m, p, parts, 0)
    f = np.zeros((n, 2))
    cnt = np.zeros(n, dtype=np.uint32)
    asum, coord, flip, cap = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)

    def add(ix, d, sl):
        f[ix] += d.forces[sl]
        cnt[ix] += d.counts[sl]
        asum[ix] += d.abs_sum[sl]
        coord[ix] += d.coord[sl]
        flip[ix] += d.flip[sl]
        cap[ix] += d.cap[sl]

    # the device walks a body's own tree first, then the peers' in rank order: the same order here
    for q, ix in enumerate(parts):
        if len(ix):
            d = O.compute_forces_diag(own_trees[q], p[ix], m[ix], theta=theta, G=G, compat_self_skip=False,
                                      pos_rounded=pos_rounded, cap_depth=cap_depth, threads=threads)
            add(ix, d, slice(0, len(ix)))
    everyone = np.arange(n)
    owner = np.empty(n, dtype=np.int64)
    for q, ix in enumerate(parts):
        owner[ix] = q
    for r, ix in enumerate(parts):
        if not len(ix) or len(ix) == n:
            continue
        tree = O.build_tree_box(p[ix], m[ix], box, cap_depth) if remote_capped else own_trees[r]
        tg = everyone[owner != r]
        pp, mm = np.concatenate([p[ix], p[tg]]), np.concatenate([m[ix], m[tg]])
        d = O.compute_forces_diag(tree, pp, mm, theta=theta, G=G, compat_self_skip=False, lo=len(ix),
                                  pos_rounded=pos_rounded or remote_capped, cap_depth=0 if remote_capped else cap_depth,
                                  threads=threads)
        add(tg, d, slice(len(ix), len(pp)))
    return O.WalkDiag(f, cnt, asum, coord, flip, cap)


def let_boxes(p, ix, boxes=LET_BOXES):
    """[boxes, 4] rows {xmin, xmax, ymin, ymax}: the raw bounds of `boxes` consecutive runs of the bodies ix (any grouping
    is a correct description; an empty run is (+inf, -inf) and matches nothing)."""
    out = np.empty((boxes, 4))
    out[:, 0::2], out[:, 1::2] = np.inf, -np.inf
    for k in range(boxes):
        q = p[ix[len(ix) * k // boxes: len(ix) * (k + 1) // boxes]]
        if len(q):
            out[k] = [q[:, 0].min(), q[:, 0].max(), q[:, 1].min(), q[:, 1].max()]
    return out


def box_dist2(cx, cy, boxes):
    """Exact fp64 distance^2 from the points (cx, cy) [k] to the nearest of `boxes` [b, 4]; inf for empty boxes."""
    cx, cy = np.asarray(cx, dtype=np.float64)[:, None], np.asarray(cy, dtype=np.float64)[:, None]
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        dx = np.maximum(np.maximum(b[None, :, 0] - cx, cx - b[None, :, 1]), 0.0)
        dy = np.maximum(np.maximum(b[None, :, 2] - cy, cy - b[None, :, 3]), 0.0)
        d2 = dx * dx + dy * dy
    d2 = np.where(np.isnan(d2), np.inf, d2)
    return d2.min(axis=1) if d2.shape[1] else np.full(len(cx), np.inf)


def let_prune(tree, boxes, theta):
    """The LET rule on an oracle tree: a node's children go to the peer iff the exact fp64 distance^2 from the node's
    centre of mass to some box of the peer is <= (size / theta)^2.  Returns (the tree with every other child link cut,
    the number of nodes reachable from the root afterwards).  A node whose links are cut is a leaf to the walk: accepted."""
    t = tree.copy()
    size = np.maximum(t["xmax"] - t["xmin"], t["ymax"] - t["ymin"])
    keep = box_dist2(t["comx"], t["comy"], boxes) <= (size / theta) ** 2
    has = t["child"][:, 0] != -1
    t["child"][has & ~keep] = -1.0
    return t, len(O.export_preorder(t)[0])
