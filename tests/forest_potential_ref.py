"""The fp64 potential of the distributed step's forest walk on the CPU -- a helper of tests/test_let_energy_cpu.py and
tests/test_gpu_let_energy.py, not a test file.

The distributed step gives every rank r the tree T_r of ITS bodies under the root box of ALL bodies (tests/forest_ref.py),
and body i of rank q takes its terms from T_q with the self skip and from every other WHOLE tree (a correct
locally-essential tree changes no term).  The potential over those terms is the sum of tests/potential_ref.potential_walk
over the trees, in the device's order: the own tree first, then the peers' in rank order.

  * T_r = O.build_tree_box(p[ix_r], m[ix_r], box_ref(p), 0): partition order, uncapped;
  * own tree: potential_walk(T_q, p[ix_q], compat=False, bodies = all of its own): the leaf whose occupant is the body
    itself is skipped;
  * another rank's tree T_r: the walked positions are T_r's bodies followed by the targets, bodies = the appended ones,
    so that no occupant index equals a target's index and the walk skips nothing (the device of forest_ref.forest_diag)."""
from __future__ import annotations

import numpy as np

from oracle import bh_oracle as O
from box_ref import box_ref
from potential_ref import potential_walk


def forest_potential(m, p, parts, theta=0.5, G=6.67e-11, bodies=None):
    """(phi, counts) of all len(m) bodies in caller order, or of the caller indices `bodies` in their order.  parts: list
    of index arrays, a partition of range(len(m)); empty ranks allowed."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    n = len(m)
    parts = [np.asarray(ix, dtype=np.int64) for ix in parts]
    assert np.array_equal(np.sort(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64), np.arange(n)), "not a partition"
    box = box_ref(p)
    trees = [O.build_tree_box(p[ix], m[ix], box, 0) if len(ix) else None for ix in parts]
    wanted = np.ones(n, dtype=bool) if bodies is None else np.isin(np.arange(n), bodies)
    phi = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    for q, ix in enumerate(parts):                              # the own tree first ...
        local = np.flatnonzero(wanted[ix])
        if len(local):
            f, c = potential_walk(trees[q], p[ix], theta=theta, G=G, compat=False, bodies=local)
            phi[ix[local]] += f
            cnt[ix[local]] += c
    owner = np.empty(n, dtype=np.int64)
    for q, ix in enumerate(parts):
        owner[ix] = q
    for r, ix in enumerate(parts):                              # ... then the peers' in rank order
        tg = np.flatnonzero(wanted & (owner != r))
        if not len(ix) or not len(tg):
            continue
        f, c = potential_walk(trees[r], np.concatenate([p[ix], p[tg]]), theta=theta, G=G, compat=False,
                              bodies=np.arange(len(ix), len(ix) + len(tg)))
        phi[tg] += f
        cnt[tg] += c
    if bodies is None:
        return phi, cnt
    bodies = np.asarray(bodies, dtype=np.int64)
    return phi[bodies], cnt[bodies]


def direct_potential(m, p, G=6.67e-11):
    """phi_i = -G sum_{j != i} m_j / (d_ij + 1e-15): the exact pair potential with the walks' distance, fp64 numpy."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    phi = np.zeros(len(m))
    for i in range(len(m)):
        d = np.sqrt(((p - p[i]) ** 2).sum(axis=1)) + 1e-15
        t = m / d
        t[i] = 0.0
        phi[i] = -G * t.sum()
    return phi
