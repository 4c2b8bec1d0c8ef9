"""The bucket sort's placement path (csrc/bh_sort.hpp "Placement") on the device: bit for bit the byte
passes (BH_SORT_PLACE=0), the counting pass (BH_SORT_DIRECT=0) and the LSD sort (BH_SORT_BUCKET=0), and the path every bucket
took pinned to the numpy twin.

The bodies are tests/sort_direct_case.py's frozen lattice, sent where a case wants them.  Every case runs the same bodies four
times and compares the exported tree of a later build and the downloaded state with ==.  The build whose tree is exported is
snapshotted, the twin (tests/sort_place_ref.py) says for the keys THE DEVICE formed which buckets are tested and which of those
the rule places, and what that build added to the two counters of BarnesHutEngine.sort_paths is exactly that -- a path that is never taken fails its case.  With
placement off the build adds nothing to the first counter and every bucket that holds two different keys to the second."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
import sort_place_ref as P  # noqa: E402
from sort_direct_case import NB, check_snapshot, engine, hull_slots, lattice, send, state_order  # noqa: E402

W = P.WINDOW
ENV = ("BH_SORT_BUCKET", "BH_SORT_DIRECT", "BH_SORT_DIRECT_MAX", "BH_REORDER_EVERY", "BH_SORT_PLACE")


def run(monkeypatch, env, m, p, v, steps, precision=G.Precision.F32, **kw):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    n = len(m)
    with engine(n, precision=precision, **kw) as e:
        e.upload(p, v, m)
        e.step(steps)
        s0, p0 = e.stats(), e.sort_paths()
        e.build_tree()
        snap = e.sort_snapshot()
        s1, p1 = e.stats(), e.sort_paths()
        nodes, depth = e.export_tree()
        e.step(1)
        pos, vel = e.download()[:2]
    rise = SimpleNamespace(placed=p1[0] - p0[0], passed=p1[1] - p0[1], reruns=s1.sort_rerun_buckets - s0.sort_rerun_buckets,
                           spills=s1.sort_spill_buckets - s0.sort_spill_buckets)
    return SimpleNamespace(out=(nodes, depth, pos, vel), snap=snap, rise=rise)


def same(a, b):
    for x, y in zip(a.out, b.out):
        if x.dtype.names:
            for f in x.dtype.names:
                assert np.array_equal(x[f], y[f], equal_nan=True), f
        else:
            assert np.array_equal(x, y)


def bucket_inputs(snap):
    """the inputs of the in-LDS sorts of the snapshotted build (None: it took the counting pass, whose splitters nobody recorded)"""
    if not snap.offered:
        return P.single_input(snap.keys_sorted, snap.perm)
    tw = check_snapshot(snap)
    return P.bucket_inputs(snap.keys_in, tw) if tw.path == "direct" else None


def compare(monkeypatch, m, p, v, steps, direct="1", bucket="2", extra=None, **kw):
    """placement on, placement off, the counting pass, the LSD sort: equal results; the counters of the first two against the twin
    -> on, off, the bucket inputs of the snapshotted build, {bucket: rule} of the refused ones"""
    extra = extra or {}
    on = run(monkeypatch, dict(BH_SORT_BUCKET=bucket, BH_SORT_DIRECT=direct, **extra), m, p, v, steps, **kw)
    off = run(monkeypatch, dict(BH_SORT_BUCKET=bucket, BH_SORT_DIRECT=direct, BH_SORT_PLACE="0", **extra), m, p, v, steps, **kw)
    reorder = {k: val for k, val in extra.items() if k == "BH_REORDER_EVERY"}
    for env in (dict(BH_SORT_BUCKET="2", BH_SORT_DIRECT="0", **reorder), dict(BH_SORT_BUCKET="0", **reorder)):
        same(on, run(monkeypatch, env, m, p, v, steps, **kw))
    same(on, off)
    assert np.isfinite(on.out[2]).all() and np.isfinite(on.out[3]).all()
    assert off.rise.placed == 0
    assert np.array_equal(on.snap.keys_sorted, off.snap.keys_sorted) and np.array_equal(on.snap.perm, off.snap.perm)
    inputs = bucket_inputs(on.snap)
    why = None
    if inputs is not None:
        placed, passed, why = P.paths(inputs)
        print(f"twin: {placed} placed, {passed} through the passes {why}; device: on {vars(on.rise)} off {vars(off.rise)}")
        assert (on.rise.placed, on.rise.passed) == (placed, passed)
        assert off.rise.passed == sum(1 for _, w, _ in inputs if len(np.unique(w & P.MASK)) > 1)
    else:
        assert on.rise.placed == 0                              # the buckets of the counting pass are not tested
    return on, off, inputs, why


def descents(inputs):
    """buckets whose input has a descent"""
    return [b for b, w, _ in inputs if ((w[1:] & P.MASK) < (w[:-1] & P.MASK)).any()]


def off_hull(slots, p, order):
    hull = hull_slots(p, order)
    assert not hull & set(slots), (hull, slots)


def test_frozen_lattice_every_range_is_placed(monkeypatch):
    m, p, v, _ = lattice(9001, 1)
    on, off, inputs, why = compare(monkeypatch, m, p, v, 3)
    L = (9001 + NB - 1) // NB
    assert why == {} and on.rise.placed == len(inputs) == (9001 + L - 1) // L and on.rise.passed == 0
    assert off.rise.passed == len(inputs) - 1                   # (the last range holds one key: nothing to sort on either path)


def test_one_mover_inside_its_range_on_both_sides_of_the_window(monkeypatch):
    """n = 20,000: ranges of 79 keys straddle a wave's 64.  A body is sent beside the one W - 1, W, W + 1, W + 2 slots on: its key
    stands that far (give or take the side it lands on) from its place.  The twin decides each case; both outcomes occur."""
    n = 20000
    m, p, v, side = lattice(n, 2)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    a = 100 * L + 58
    off_hull([a], p, order)
    outcomes = []
    for d in (W - 1, W, W + 1, W + 2):
        on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, [a], [a + d], 3), 3)
        assert descents(inputs) == [100] and set(why) <= {100}
        outcomes.append(why.get(100))
    assert None in outcomes and "window" in outcomes and set(outcomes) <= {None, "window"}, outcomes


def test_swaps_at_the_ends_of_ranges_and_in_the_last_range(monkeypatch):
    """Movers from a range's second slot, to beside its last but one and back from its last, and inside the last range that holds
    keys (n = 10,000: 250 ranges of 40).  Nobody leaves its range: the build has no crosser and every range is tested."""
    n = 10000
    m, p, v, side = lattice(n, 3)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    last = ((n - 1) // L) * L
    src = [10 * L + 1, 20 * L + L - 5, 30 * L + L - 1, last + 2, n - 1]
    dst = [10 * L + 3, 20 * L + L - 2, 30 * L + L - 4, last + 5, n - 4]
    off_hull(src, p, order)
    on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, src, dst, 3), 3)
    assert inputs is not None and not on.snap.decision.any() and len(descents(inputs)) >= 3 and on.rise.placed > 200


@pytest.mark.parametrize("n", [1024, 1025, 2048, 2049, 4096])
def test_single_bucket_launches(monkeypatch, n):
    """BH_SORT_BUCKET=1: one workgroup sorts the launch, 1, 2 or 4 keys per thread; a wave owns 64, 128 or 256 consecutive keys.
    Frozen: placed.  Then a body is sent across the first 64-key boundary and one across the first wave's last key."""
    m, p, v, side = lattice(n, 4)
    on, off, inputs, why = compare(monkeypatch, m, p, v, 3, bucket="1")
    assert not on.snap.offered and (on.rise.placed, on.rise.passed) == (1, 0) and (off.rise.placed, off.rise.passed) == (0, 1)
    order = state_order(m, p, side)
    chunk = 64 * (1 if n <= 1024 else 2 if n <= 2048 else 4)
    src = sorted({62, chunk - 2, n - 4})
    dst = [s + 3 for s in src]
    off_hull(src, p, order)
    on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, src, dst, 3), 3, bucket="1")
    assert descents(inputs) == [0] and why == {}
    # (eleven slots on: further than the window)
    on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, [chunk - 6], [chunk + 5], 3), 3, bucket="1")
    assert why == {0: "window"} and (on.rise.placed, on.rise.passed) == (0, 1)


def test_one_range_with_a_crowd(monkeypatch):
    """Ten bodies at one point (softened forces): their range spans more than 24 bits and holds a run of more than kFixRun equal
    keys -- it keeps the passes and their re-run; every other range is placed."""
    n = 9000
    m, p, v, side = lattice(n, 5)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    p = p.copy()
    for s in range(60 * L + 6, 60 * L + 15):
        p[order[s]] = p[order[60 * L + 5]]
    on, off, inputs, why = compare(monkeypatch, m, p, v, 3, softening=1e-3)
    assert list(why.values()) == ["crowd"] and on.rise.passed == 1 and on.rise.reruns == 1 and off.rise.reruns == 1
    assert on.rise.placed == len(inputs) - 1


def test_every_body_drifting_is_not_placed(monkeypatch):
    """Every body moves a sixty-fourth of the box per step in a direction of its own.  One bucket of 4,096: nowhere near ordered,
    not placed.  256 buckets of 20,000: the build takes the counting pass, whose buckets are not tested: nothing placed."""
    m, p, v = IC.make("plummer", 4096, 3, quasi_static=True, drift_cells=1.0, drift_depth=6)
    on, off, inputs, why = compare(monkeypatch, m, p, v, 3, bucket="1")
    assert (on.rise.placed, on.rise.passed) == (0, 1) and why[0] in ("descents", "window")
    m, p, v = IC.make("plummer", 20000, 3, quasi_static=True, drift_cells=1.0, drift_depth=6)
    on, off, inputs, why = compare(monkeypatch, m, p, v, 3, direct="2")
    assert inputs is None and on.snap.counting and on.rise.placed == 0 and 200 < on.rise.passed <= NB
    assert on.rise.passed == off.rise.passed


def test_a_build_with_crossers_is_not_tested(monkeypatch):
    """One body travels into the middle of another range: the direct path with one crosser.  No range of such a build is tested
    (bodies on their way cost the test more than it saves: profiles/sort_place), every bucket takes the passes, and the results
    are those of the other sorts."""
    n = 12000
    m, p, v, side = lattice(n, 6)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    a = 50 * L + 5
    off_hull([a], p, order)
    on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, [a], [120 * L + 30], 3), 3)
    assert on.snap.offered and not on.snap.counting and int(on.snap.decision[1:].sum()) == 1
    assert set(why.values()) == {"crossers"} and len(why) == len(inputs) and on.rise.placed == 0
    assert on.rise.passed == off.rise.passed == len(inputs)


def test_twenty_steps_reordering_every_second_build(monkeypatch):
    """Fifteen bodies each on their way past five neighbours inside their range, the state re-ordered at every second build:
    twenty steps of placement on against off and the other sorts, then one more, so that the snapshotted build is not one that
    re-orders the state (such a build leaves the identity in perm, and the snapshot's output no longer tells where a key came
    from)."""
    n = 11000
    m, p, v, side = lattice(n, 8)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    src = [9 + 13 * L * k for k in range(15)]
    off_hull(src, p, order)
    v = send(p, v, order, src, [s + 5 for s in src], 21)          # (they arrive at the snapshotted build; on the way some cross)
    on, off, inputs, why = compare(monkeypatch, m, p, v, 21, extra=dict(BH_REORDER_EVERY="2"))
    assert inputs is not None and on.rise.placed > 200


def test_mixed_precision(monkeypatch):
    n = 9500
    m, p, v, side = lattice(n, 10)
    order = state_order(m, p, side, precision=G.Precision.MIXED)
    L = (n + NB - 1) // NB
    src, dst = [33 * L + 7, 99 * L + 7, 170 * L + 4], [33 * L + 11, 99 * L + 20, 170 * L + 9]
    off_hull(src, p, order)
    on, off, inputs, why = compare(monkeypatch, m, p, send(p, v, order, src, dst, 3), 3, precision=G.Precision.MIXED)
    assert inputs is not None and len(descents(inputs)) >= 2 and on.rise.placed > 200
