"""The bucket sort's direct input (csrc/bh_sort.hpp) on the device: bit for bit the counting pass, bit for
bit the LSD passes, and the path every build took pinned to the numpy twin.

The harness is tests/sort_direct_case.py: every case runs the same bodies three times and compares trees and state with ==, and
the build whose tree is exported is snapshotted -- the decision the device took, its list counters, the listed words and the
range keys are the twin's for the keys the device formed, and the sort's output is numpy's stable sort of them.  What a case's
docstring says about the path its build takes is asserted (path, k = crossers, why = the rule that sends it to the counting
pass).  N is between 8,200 and 20,000, so with 256 buckets a range holds 33 to 79 keys and every workgroup of bucket_sort_kernel
has work.  The decision's edges, the pile-ups and the range-length edges are in tests/test_gpu_sort_direct_edges.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from sort_direct_case import NB, compare, hull_slots, lattice, off_starts, send, state_order  # noqa: E402


def test_frozen_bodies_have_no_crosser(monkeypatch):
    m, p, v, _ = lattice(9001, 1)
    c = compare(monkeypatch, m, p, v, 3, path="direct", k=0)
    assert c.new.sort_spill_buckets == 0 and c.old.sort_spill_buckets == 0
    assert not c.snap.decision.any()


def test_a_dozen_bodies_cross_the_domain(monkeypatch):
    """Twelve bodies travel across the box in three steps: four into one bucket (two of them from below, two from above it),
    two into bucket 0, two into the last bucket that has a range (n = 10,000: 250 ranges of 40, six empty ones behind, which
    no key can reach -- their range key is above every key), the rest to scattered places; one of them leaves a range whose
    neighbours it will pass again.  Every build after the first meets them somewhere else."""
    n = 10000
    m, p, v, side = lattice(n, 2)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    movers = off_starts([7, 3 * L + 5, 180 * L + 9, 200 * L + 11, 100 * L + 3, 101 * L + 4, 5 * L + 6, 6 * L + 7, 40 * L + 1, 77 * L + 2,
                         150 * L + 13, 249 * L + 3], L)
    targets = [120 * L + 4, 120 * L + 9, 120 * L + 14, 120 * L + 19, 2, 5, n - 3, n - 6, 230 * L + 8, 20 * L + 8, 60 * L + 8, 9 * L + 8]
    v = send(p, v, order, movers, targets, 3)
    compare(monkeypatch, m, p, v, 3, path="direct", k=12)       # (all twelve have arrived, each in another bucket than its own)
    c = compare(monkeypatch, m, p, v, 1, path="direct")         # (the build that is compared is the first with crossers)
    assert 1 <= c.twin.k <= 12                                  # (a third of the way: nobody else can have left its range)


@pytest.mark.parametrize("movers", [8, 9])
def test_both_sides_of_the_capacity(monkeypatch, movers):
    """BH_SORT_DIRECT_MAX=8: eight bodies away from home fit the list, with the ninth the counter passes the capacity and the
    build takes the counting pass.  (The movers are away from their ranges at every build after the first.)"""
    n = 8200
    m, p, v, side = lattice(n, 3)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    src = off_starts([11 + 25 * L * k for k in range(movers)], L)
    dst = [(s + 120 * L) % n for s in src]
    v = send(p, v, order, src, dst, 4)
    want = dict(path="direct", why=()) if movers == 8 else dict(path="counting", why=("total",))
    c = compare(monkeypatch, m, p, v, 3, extra=dict(BH_SORT_DIRECT_MAX="8"), k=movers, **want)
    assert (c.snap.cap, c.snap.subcap, c.snap.nsub) == (8, 16, 64)


def test_a_third_of_the_bodies_cross_with_the_list_sized_for_all(monkeypatch):
    """BH_SORT_DIRECT=2: every third body that is not at a range start trades places with another one over four steps, so
    from the second build on thousands of keys are listed and most buckets merge dozens of arrivals from both sides."""
    n = 15000
    m, p, v, side = lattice(n, 4)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    rng = np.random.default_rng(5)
    src = np.array([s for s in range(n) if s % 3 == 1 and s % L != 0])
    dst = rng.permutation(src)
    v = send(p, v, order, src, dst, 4)
    c = compare(monkeypatch, m, p, v, 3, direct="2", path="direct")
    assert c.twin.k > n // 4 and (c.snap.cap, c.snap.subcap, c.snap.nsub) == (n, n, 1)
    compare(monkeypatch, m, p, v, 1, direct="2", path="direct")


def test_a_body_flung_far_moves_the_root_box(monkeypatch):
    """One body leaves at 40 box widths per step: the root box jumps, every key changes and so does the order along the curve --
    range keys out of order or crossers by the thousand, the builds take the counting pass, whatever the list holds; the same
    body on its way across the box -- inside the hull at every build, and not one of the bodies that carry the root box --
    leaves the later builds on the direct path, with one crosser.  (Sent to arrive in two steps, as this case first had it, the
    body is twice as far at the fourth and outside the hull: the box grows, the range keys fall out of order, and those builds
    take the counting pass too -- the snapshot says so.)"""
    n = 12000
    m, p, v, side = lattice(n, 6)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    far = v.copy()
    far[order[50 * L + 3]] = [80.0, 55.0]
    compare(monkeypatch, m, p, far, 4, path="counting")
    compare(monkeypatch, m, p, far, 4, direct="2", path="counting")
    compare(monkeypatch, m, p, send(p, v, order, [50 * L + 3], [200 * L + 3], 2), 4, path="counting")
    hull = hull_slots(p, order)
    mover = next(s for s in range(50 * L + 3, 51 * L) if s not in hull)
    compare(monkeypatch, m, p, send(p, v, order, [mover], [200 * L + 3], 6), 4, path="direct", k=1)


def test_coincident_bodies_on_a_range_boundary(monkeypatch):
    """Five bodies at one point astride a range start (equal keys: body order decides, and two range keys may be equal), with
    Plummer softening so that their mutual forces are finite; some of them then drift apart, one travels away."""
    n = 9000
    m, p, v, side = lattice(n, 7)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    p = p.copy()
    for s in (60 * L - 2, 60 * L - 1, 60 * L + 1, 60 * L + 2):
        p[order[s]] = p[order[60 * L]]
    # (also a whole range and its neighbour's start at one point: range keys 90 and 91 equal)
    for s in range(90 * L + 1, 91 * L + 1):
        p[order[s]] = p[order[90 * L]]
    v2 = send(p, v, order, [60 * L + 2, 90 * L + 5], [10 * L + 5, 200 * L + 7], 3)
    for direct in ("1", "2"):
        # (the path is whatever the twin says for the keys the device formed; a run of more than eight equal keys in a bucket
        # that spans more than 24 bits sends its workgroup through the LDS sort's re-run -- on the direct path from a buffer
        # that IS the input)
        for vel in (v, v2):
            c = compare(monkeypatch, m, p, vel, 3, direct=direct, softening=1e-3)
            assert c.new.sort_rerun_buckets > 0 and c.rise.reruns > 0


def test_reordering_every_second_build(monkeypatch):
    n = 11000
    m, p, v, side = lattice(n, 8)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    src = off_starts([9 + 13 * L * k for k in range(15)], L)
    v = send(p, v, order, src, [(s + 97 * L) % n for s in src], 6)
    # (a re-ordering may leave a mover at a range start: the path is the twin's for the keys the device formed)
    compare(monkeypatch, m, p, v, 5, extra=dict(BH_REORDER_EVERY="2"))
    compare(monkeypatch, m, p, v, 5, direct="2", extra=dict(BH_REORDER_EVERY="2"))


def test_ranges_of_unequal_length(monkeypatch):
    """N = 8,191 + 4 x 64 + 1 = 8,448 fills 256 ranges of 33 exactly; one body more or less leaves a shorter last range
    (8,447) or 249 ranges of 34 with seven empty ones behind (8,449)."""
    for n in (8191 + 4 * 64 + 1, 8447, 8449):
        m, p, v, side = lattice(n, 9)
        order = state_order(m, p, side)
        L = (n + NB - 1) // NB
        last = ((n - 1) // L) * L
        src = off_starts([5, last + 1, 100 * L + 2, n - 1], L)
        v = send(p, v, order, src, [last + 2, 3, n - 2, 30 * L + 2], 3)
        compare(monkeypatch, m, p, v, 3, path="direct", k=4)


def test_mixed_precision(monkeypatch):
    n = 9500
    m, p, v, side = lattice(n, 10)
    order = state_order(m, p, side, precision=G.Precision.MIXED)
    L = (n + NB - 1) // NB
    src = off_starts([4, 33 * L + 2, 99 * L + 7, 170 * L + 1, 240 * L + 9], L)
    v = send(p, v, order, src, [200 * L + 3, 1, 98 * L + 1, 171 * L + 4, 12 * L + 2], 3)
    compare(monkeypatch, m, p, v, 3, precision=G.Precision.MIXED, path="direct", k=5)
    compare(monkeypatch, m, p, v, 3, direct="2", precision=G.Precision.MIXED, path="direct", k=5)
