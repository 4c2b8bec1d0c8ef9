"""The packed LET blocks themselves (let_mark_alloc_kernel, let_pack_kernel: csrc/bh_let.hpp), read back from the device.

For every (sender r, peer q) pair the send block is compared with the sender's own quads and with the rule it states:

  WELL-FORMED  following the links from slot 0, every link lies inside the block, below the count let_counts() reports; no
               slot is reached twice; the record reached through slot s of a record that is the sender's quad k IS the
               sender's quad child[s] of k -- xy, m and thr bit for bit; a sender-side bucket arrives as child = -1, thr = 0.
  COMPLETE     a reached node with a child quad whose EXACT fp64 distance^2 -- from the device's own fp32 centre of mass to
               the nearest of the peer's unrounded boxes in all_bounds -- is <= the device's own thr has that child quad
               linked.  The conservative direction: no tolerance.  (The device tests outward-rounded fp32 boxes against
               thr * 1.0001f: rounding can only add links.)
  TIGHT        a linked child quad is within reach up to rounding: with dx, dy the exact per-axis distances to a box,
               u = 2^-23 * (the largest coordinate magnitude of the axis) >= one fp32 ulp there,
                   max(dx - 2u_x, 0)^2 + max(dy - 2u_y, 0)^2 <= 1.0002 * thr        for some box of the peer.
               Derivation: the device's fp32 box edge is at most one ulp outside the fp64 one, and its fp32 subtraction
               rounds by 2^-24 * dx <= u, so its dx_f >= dx - 2u; its fl(dx_f^2 + dy_f^2) >= (1 - 2^-24)^2 (dx_f^2 + dy_f^2);
               its threshold is fl(thr * fl(1.0001)) <= 1.0001 (1 + 2^-24)^2 thr.  A link therefore needs
               (dx - 2u)^2 + (dy - 2u)^2 <= 1.0001 (1 + 2^-24)^2 / (1 - 2^-24)^2 thr < 1.0002 thr.  This one only keeps the
               LET from silently growing.

Worlds 2, 5, 33 (above 32: the upper word of the need mask) and 64 (bit 63, the ~0ull branch of `everyone`; more than 56
trees: the one-wave walk), world 1, ranks without bodies, and a let_cap too small for exactly one pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import forest_ref as FR  # noqa: E402
import parity_classes as PC  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.distributed import partition_orb  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_STATS  # noqa: E402
from let_ranks import EmulatedRanks  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SEEN = {"buckets": 0}        # sender-side buckets met by walk_block (a test that is about them checks that it met some)


def walk_block(block, local, base, limit):
    """Follow the links of a packed block from slot 0: {slot: the sender's quad it must be a copy of}, checked on the way.
    base: the receiver's index of slot 0; limit: links must stay below base + limit."""
    match = {0: 0}
    todo = [0]
    while todo:
        o = todo.pop()
        k = match[o]
        rec, src = block[o], local[k]
        assert np.array_equal(_bits(rec["xy"]), _bits(src["xy"])) and np.array_equal(_bits(rec["m"]), _bits(src["m"])), (o, k)
        for s in range(4):
            c, link = int(src["child"][s]), int(rec["child"][s])
            if c <= -2:                                  # a bucket of the sender: an aggregate to everybody else
                assert link == -1 and rec["thr"][s] == 0.0 and np.isposinf(src["thr"][s]), (o, k, s)
                SEEN["buckets"] += 1
                continue
            assert _bits(rec["thr"])[s] == _bits(src["thr"])[s], (o, k, s)
            if c < 1:
                assert link == -1, (o, k, s)
            elif link != -1:
                assert base <= link < base + limit, (o, k, s, link, base, limit)
                assert link - base not in match, ("reached twice", link - base)
                match[link - base] = c
                todo.append(link - base)
    return match


def check_pair(er, r, q, local, bounds, count, complete=True):
    """The block sender r packed for peer q: well-formed, complete, tight.  Returns the number of reached records."""
    block = er.send_block(r, q)
    base = er.forest_base + r * er.let_cap
    match = walk_block(block, local, base, min(count, er.let_cap))
    assert len(match) <= count
    boxes = bounds[q]
    fin = boxes[np.isfinite(boxes).all(axis=1)]
    for o, k in match.items():
        src, rec = local[k], block[o]
        for s in range(4):
            if src["child"][s] < 1:
                continue
            cx, cy, thr = float(src["xy"][2 * s]), float(src["xy"][2 * s + 1]), float(src["thr"][s])
            linked = rec["child"][s] != -1
            d2 = float(FR.box_dist2([cx], [cy], boxes)[0])
            if complete and d2 <= thr:
                assert linked, ("a needed child quad is cut", r, q, k, s, d2, thr, count, er.let_cap, len(match))
            if linked:
                ux = 2.0 ** -23 * max(abs(cx), np.abs(fin[:, :2]).max())
                uy = 2.0 ** -23 * max(abs(cy), np.abs(fin[:, 2:]).max())
                dx = np.maximum(np.maximum(np.maximum(fin[:, 0] - cx, cx - fin[:, 1]), 0.0) - 2 * ux, 0.0)
                dy = np.maximum(np.maximum(np.maximum(fin[:, 2] - cy, cy - fin[:, 3]), 0.0) - 2 * uy, 0.0)
                assert (dx * dx + dy * dy).min() <= 1.0002 * thr, ("a link nobody can need", r, q, k, s, d2, thr)
    return len(match)


def clustered(n, seed):
    r = np.random.default_rng(seed)
    c = r.uniform(-1, 1, (5, 2))
    p = (c[r.integers(0, 5, n)] + r.normal(0, 0.15, (n, 2))).astype(np.float32).astype(np.float64)
    m = (10.0 ** r.uniform(-2, 0, n)).astype(np.float32).astype(np.float64)
    return m, p, np.zeros((n, 2))


def check_all_pairs(er, skip=()):
    """Every (sender, peer) block of the last step; returns the matrix of reported counts and the reached records."""
    W = er.world
    mine = np.stack([er.lbounds(r) for r in range(W)])
    counts, reached = np.zeros((W, W), dtype=np.int64), np.zeros((W, W), dtype=np.int64)
    flags = []
    for r in range(W):
        c, ov = er.engs[r].let_counts(with_overflow=True)
        counts[r] = c
        flags.append(ov)
    for r in range(W):
        bounds = er.all_bounds(r)
        assert np.array_equal(bounds, mine)                                  # (the all_gather this rank saw)
        local = er.local_quads(r)
        assert counts[r, r] == 0
        for q in range(W):
            if q != r and (r, q) not in skip:
                reached[r, q] = check_pair(er, r, q, local, bounds, counts[r, q])
    return counts, reached, flags


@pytest.mark.parametrize("world,n,theta", [(2, 6000, 0.5), (5, 9000, 0.5), (5, 5000, 0.9), (33, 33 * 150, 0.5), (64, 64 * 110, 0.5),
                                           (64, 64 * 110, 0.25)])
def test_every_block_is_well_formed_complete_and_tight(world, n, theta):
    m, p, v = clustered(n, 100 + world)
    parts = partition_orb(p, world)
    if world >= 33:
        assert 40 <= min(len(ix) for ix in parts) and max(len(ix) for ix in parts) <= 300
    er = EmulatedRanks(m, p, v, world, None, partition=lambda pp, w: parts, theta=theta, max_depth=21, reference_compat=False,
                       flags=FLAG_WALK_STATS)
    try:
        er.step(integrate=False)
        counts, reached, flags = check_all_pairs(er)
        assert not any(flags)
        off = ~np.eye(world, dtype=bool)
        assert (counts[off] >= 1).all() and (reached[off] >= 1).all()
        # pruning is exercised: some block is smaller than the sender's tree, and the highest rank is somebody's peer
        quads = np.array([e.stats().n_internal + 1 for e in er.engs])
        assert (counts < quads[:, None])[off].any() and (reached[:, world - 1] > 1).any()
        # and the receivers' walks of those blocks take the whole trees' terms
        a = er.gather(lambda e: e.accelerations())
        cnt = er.gather1(lambda e: e.interaction_counts())
    finally:
        er.close()
    rep = PC.classify(a, cnt, m, p, theta, n, diag=FR.forest_diag(m, p, parts, theta))
    assert rep.clean_count_mismatches == 0 and rep.clean_model_max <= PC.MODEL_MAX and rep.nonfinite == 0, rep
    assert rep.borderline_excess_max <= 5e-2 and rep.clean_fraction >= 0.9, rep


def test_sender_side_buckets_arrive_as_aggregates():
    """max_depth = 6, reference_compat off: the senders' depth-cap cells are buckets (child <= -2, thr = +inf); every block
    carries them as aggregates (child = -1, thr = 0: walk_block asserts it), and the receivers take them as point masses --
    the forest oracle with capped remote trees (tests/forest_ref.py: remote_capped)."""
    n, world, md = 6000, 3, 6
    m, p, v = clustered(n, 11)
    parts = partition_orb(p, world)
    er = EmulatedRanks(m, p, v, world, None, partition=lambda pp, w: parts, max_depth=md, reference_compat=False,
                       flags=FLAG_WALK_STATS)
    try:
        er.step(integrate=False)
        buckets = sum(int((er.local_quads(r)["child"] <= -2).sum()) for r in range(world))
        assert buckets > 100
        SEEN["buckets"] = 0
        counts, reached, flags = check_all_pairs(er)
        assert not any(flags) and SEEN["buckets"] > 0
        a = er.gather(lambda e: e.accelerations())
        cnt = er.gather1(lambda e: e.interaction_counts())
    finally:
        er.close()
    rep = PC.classify(a, cnt, m, p, 0.5, n, diag=FR.forest_diag(m, p, parts, 0.5, cap_depth=md, remote_capped=True))
    assert rep.clean_count_mismatches == 0 and rep.clean_model_max <= PC.MODEL_MAX and rep.nonfinite == 0, rep
    assert rep.borderline_excess_max <= 5e-2 and rep.clean_fraction >= 0.9, rep


def test_world_of_one():
    """No peer: nothing is packed, and the forest walk is the single context's walk bit for bit."""
    n = 20000                                            # (313 groups: 8 waves per group with and without LET mode)
    m, p, v = IC.make("plummer", n, 5, quasi_static=True)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=G.Precision.F32, max_depth=21, reference_compat=False)) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a1 = e.accelerations()
    er = EmulatedRanks(m, p, v, 1, 64, partition=lambda pp, w: [np.arange(n)], max_depth=21, reference_compat=False)
    try:
        er.step(integrate=False)
        assert er.engs[0].let_counts() == [0]
        a = er.gather(lambda e: e.accelerations())
    finally:
        er.close()
    assert np.array_equal(_bits(a.astype(np.float32)), _bits(a1.astype(np.float32))) and np.array_equal(a, a1)


def test_ranks_without_bodies_keep_empty_boxes_and_get_root_quads_only():
    n, world = 4000, 6
    m, p, v = clustered(n, 7)
    halves = partition_orb(p, 3)
    parts = [halves[0], np.zeros(0, dtype=np.int64), halves[1], np.zeros(0, dtype=np.int64), halves[2], np.zeros(0, dtype=np.int64)]
    er = EmulatedRanks(m, p, v, world, None, partition=lambda pp, w: parts, max_depth=21, reference_compat=False,
                       flags=FLAG_WALK_STATS)
    try:
        er.step(integrate=False)
        empty = np.tile([np.inf, -np.inf, np.inf, -np.inf], (8, 1))
        for r in (1, 3, 5):
            assert np.array_equal(er.lbounds(r), empty)                      # (+inf, -inf): matches nothing
        counts, reached, flags = check_all_pairs(er)
        assert not any(flags)
        for r in range(world):
            for q in (1, 3, 5):
                if q != r:
                    assert counts[r, q] == 1 and reached[r, q] == 1          # nobody there: the root quad alone
        assert (counts[[1, 3, 5]][:, [0, 2, 4]] == 1).all()                   # and an empty sender has a root quad to send:
        for r in (1, 3, 5):                                                   # an empty cell
            assert (er.send_block(r, 0)[0]["m"] == 0).all() and (er.send_block(r, 0)[0]["child"] == -1).all()
        a = er.gather(lambda e: e.accelerations())
        cnt = er.gather1(lambda e: e.interaction_counts() if e.n else np.zeros(0, dtype=np.uint32))
    finally:
        er.close()
    rep = PC.classify(a, cnt, m, p, 0.5, n, diag=FR.forest_diag(m, p, parts, 0.5))
    assert rep.clean_count_mismatches == 0 and rep.clean_model_max <= PC.MODEL_MAX and rep.nonfinite == 0, rep


def test_a_block_that_overflows_is_cut_inside_its_block():
    """let_cap too small for exactly one (sender, peer) pair: the sender raises the overflow flag, every link of every
    block -- the cut one included -- stays inside its block, and every other pair's block is still complete."""
    n, world = 9000, 5
    m, p, v = clustered(n, 105)
    parts = partition_orb(p, world)
    er = EmulatedRanks(m, p, v, world, None, partition=lambda pp, w: parts, max_depth=21, reference_compat=False)
    try:
        # (the first build re-orders the bodies physically, and the boxes of a rank that has not stepped are slices of its
        #  body array: from the second build on they, and with them the LET sizes, stay as they are)
        er.step(integrate=False)
        for e in er.engs:
            e.let_counts()
        er.step(integrate=False)
        counts = np.array([e.let_counts() for e in er.engs])
        order = np.sort(counts.ravel())
        assert order[-1] > order[-2] > 1                                      # one largest block
        cap = int(order[-2])
        r0, q0 = (int(x) for x in np.argwhere(counts == order[-1])[0])
        print("counts", counts.tolist(), "cap", cap, "cut pair", (r0, q0))
        er.configure(cap)
        er.step(integrate=False)
        c2, reached, flags = check_all_pairs(er, skip={(r0, q0)})
        assert np.array_equal(c2, counts)                                     # the sizes NEEDED are reported, cut or not
        assert flags == [r == r0 for r in range(world)]
        # the cut block: well-formed inside let_cap records (walk_block asserts every link), no promise of completeness
        got = check_pair(er, r0, q0, er.local_quads(r0), er.all_bounds(r0), cap, complete=False)
        assert 1 <= got <= cap
    finally:
        er.close()
