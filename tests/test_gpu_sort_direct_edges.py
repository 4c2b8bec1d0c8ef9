"""The bucket sort's direct input on the device, where it decides and where its rare branches begin (csrc/bh_sort.hpp, keys_kernel
in csrc/bh_tree.hpp).  The harness is tests/sort_direct_case.py: three runs compared with ==, and the build
under test pinned to the numpy twin through BarnesHutEngine.sort_snapshot -- so every case asserts the path it is about.

  * the decision's edges with the default switches (T = 1,024, 64 lists of 64, list = (slot >> 6) & 63): a list that holds its
    room and one that does not, half a wave and one body more, T crossers and T + 1;
  * pile-ups with BH_SORT_DIRECT=2: more than kMineCap = 3,072 arrivals in one bucket (listed a second time, into the output
    stretch), a bucket of more than kBucketCap = 12,288 keys (staged in the scratch array, sorted through memory), each with the
    bucket in the middle, at the front and at the end of the array; arrivals that share a key under a span of more than 24 bits
    (the LDS sort's re-run from a buffer that is the input).  The thresholds are asserted on the twin's routing of the device's
    keys: a geometry that misses them fails;
  * the range lengths at the sizes where they occur: N = 1,048,576 (256 ranges of 4,096 = four keys in every thread) and
    N = 1,048,577 (1,024 ranges of 1,025);
  * behind the carry: a warm context re-uploaded, and walks in n_threads passes;
  * the snapshot itself: it changes nothing, and says no where it cannot answer.

All movers arrive in ONE step (dt = 1), each at a landing point of its own beside a body of another range, so the build under
test meets every one of them away from home.  The four bodies that carry the root box never travel: the box and with it the key
of every body at rest stay what they were, and the crossers are the movers exactly (let one of the four leave and a handful of
bodies that never moved change sides of a range key -- 1,026 crossers where 1,024 were sent)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
import quiet_case  # noqa: E402
from sort_direct_case import NB, check_snapshot, compare, engine, hull_slots, lattice, send, send_each, state_order  # noqa: E402

ERR_STATE = -5
K_MINE_CAP, K_BUCKET_CAP = 3072, 12288            # bh_sort.hpp: kMineCap, kBucketCap


@pytest.fixture(scope="module")
def frozen():
    """n -> (m, p, v, order, L, hull = the slots that carry the root box: they stay) of the lattice of n bodies, made once per
    module and left unchanged"""
    made = {}

    def get(n, nb=NB):
        if n not in made:
            m, p, v, side = lattice(n, 20 + n % 7)
            order = state_order(m, p, side)
            for a in (m, p, v, order):
                a.setflags(write=False)
            made[n] = (m, p, v, order, (n + nb - 1) // nb, hull_slots(p, order))
        return made[n]

    return get


def in_wave(w, count, L, hull):
    """the first `count` slots of wave w that are no range starts and do not carry the root box"""
    return [s for s in range(64 * w, 64 * (w + 1)) if s % L != 0 and s not in hull][:count]


def far_targets(movers, L, n):
    """for every mover a slot in the middle of a full range a hundred to a hundred and fifty ranges from its own"""
    full = n // L
    assert full > 160
    return [((s // L + 100 + i % 50) % full) * L + L // 2 for i, s in enumerate(movers)]


# ---- the decision's edges (default switches) ---------------------------------------------------------------------------------
N_EDGE = 20000                                        # L = 79, 313 waves


def decide(monkeypatch, frozen, waves, **want):
    """waves: (wave, movers out of it) pairs"""
    m, p, v, order, L, hull = frozen(N_EDGE)
    assert L == 79
    movers = sum((in_wave(w, count, L, hull) for w, count in waves), [])
    assert len(movers) == sum(count for _, count in waves)
    c = compare(monkeypatch, m, p, send_each(p, v, order, movers, far_targets(movers, L, N_EDGE)), 1, k=len(movers), **want)
    assert (c.snap.cap, c.snap.subcap, c.snap.nsub) == (1024, 64, 64)
    return c


@pytest.mark.parametrize("per_wave,want", [(16, dict(path="direct", why=())), (20, dict(path="counting", why=("list",)))])
def test_a_list_holds_its_room_and_no_more(monkeypatch, frozen, per_wave, want):
    """waves 5, 69, 133 and 197 share list 5: 4 x 16 = 64 crossers fill it, 4 x 20 = 80 -- far below T -- do not fit"""
    decide(monkeypatch, frozen, [(w, per_wave) for w in (5, 69, 133, 197)], **want)


@pytest.mark.parametrize("count,want", [(32, dict(path="direct", why=())), (33, dict(path="counting", why=("wave",)))])
def test_half_a_wave_may_cross_and_no_more(monkeypatch, frozen, count, want):
    decide(monkeypatch, frozen, [(7, count)], **want)


@pytest.mark.parametrize("extra,want", [(0, dict(path="direct", why=())), (1, dict(path="counting", why=("total",)))])
def test_t_crossers_and_no_more(monkeypatch, frozen, extra, want):
    """16 in each of the waves 0 .. 63, one list each: no list over 64, no wave over 32, 1,024 in all; the 1,025th is one too many"""
    decide(monkeypatch, frozen, [(w, 16) for w in range(64)] + [(100, extra)], **want)


# ---- pile-ups (BH_SORT_DIRECT=2) -----------------------------------------------------------------------------------------
def landing_slots(T, L, n):
    """the slots of range T whose bodies the movers land beside: no range start, not the range's last slot, and all of them
    between the same two of the counting run's splitter samples (ranks j * n / 256), so that the pile is one bucket's in that
    run too"""
    r0, r1 = T * L, min((T + 1) * L, n)
    slots = np.arange(r0 + 1, r1 - 1)
    ranks = (np.arange(256, dtype=np.int64) * n) >> 8
    slots = slots[~np.isin(slots, ranks) & ~np.isin(slots - 1, ranks)]
    group = np.searchsorted(ranks, slots, side="right")
    best = np.bincount(group).argmax()
    return slots[group == best]


def pile(monkeypatch, frozen, n, T, travels):
    m, p, v, order, L, hull = frozen(n)
    last = (n - 1) // L
    T = {"first": 0, "middle": last // 2, "last": last}[T]
    movers = np.array([s for s in range(n) if s % L != 0 and s // L != T and s not in hull and travels(s)])
    land = landing_slots(T, L, n)
    assert len(land) >= 8
    c = compare(monkeypatch, m, p, send_each(p, v, order, movers, land[np.arange(len(movers)) % len(land)]), 1, direct="2",
                path="direct")
    tw = c.twin
    # (the bodies that carry the root box stay, so nobody but a mover crosses; a landing point now and then lies across a coarse
    # cell boundary from its target and belongs to a neighbouring bucket -- its mover's own, once in a while: the crossers are
    # the movers but for a handful, and the thresholds below are asserted)
    assert 0.98 * len(movers) <= tw.k <= len(movers)
    print(f"pile n {n} bucket {T}: below {tw.below[T]} above {tw.above[T]} left {tw.left[T]} m {tw.m[T]}; "
          f"spills +{c.rise.spills} / +{c.rise_old.spills} re-runs +{c.rise.reruns} / +{c.rise_old.reruns}")
    assert (tw.below[T] > 0) == (T > 0) and (tw.above[T] > 0) == (T < last)
    return c, tw, T


@pytest.mark.parametrize("where", ["middle", "first", "last"])
def test_more_arrivals_than_lds_holds(monkeypatch, frozen, where):
    """every third slot travels into one range: more than kMineCap arrivals, a bucket that still fits LDS"""
    c, tw, T = pile(monkeypatch, frozen, 20000, where, lambda s: s % 3 == 1)
    assert tw.below[T] + tw.above[T] > K_MINE_CAP and tw.m[T] <= K_BUCKET_CAP


@pytest.mark.parametrize("where", ["middle", "first", "last"])
def test_a_bucket_too_large_for_lds(monkeypatch, frozen, where):
    """every odd slot travels into one range (at most 32 of a wave): more keys than one workgroup sorts in LDS"""
    c, tw, T = pile(monkeypatch, frozen, 30000, where, lambda s: s % 2 == 1)
    assert tw.m[T] > K_BUCKET_CAP
    assert c.rise.spills == c.rise_old.spills and c.rise.spills >= 1


def test_arrivals_that_share_a_key_under_a_wide_span(monkeypatch, frozen):
    """forty bodies land on ONE point (Plummer softening keeps their forces finite) in a bucket whose keys span more than 24
    bits: a run of more than eight keys equal in the top 24 bits of the span, the LDS sort runs again in full"""
    n = 20000
    m, p, v, order, L, hull = frozen(n)
    T = 126
    movers = [(T + 40 + 2 * i) % (n // L) * L + 7 + i for i in range(40)]
    c = compare(monkeypatch, m, p, send(p, v, order, movers, [T * L + L // 2] * 40, 1), 1, direct="2", path="direct", k=40,
                softening=1e-3)
    tw = c.twin
    a = int(tw.m[:T].sum())
    span = int(c.snap.keys_sorted[a + int(tw.m[T]) - 1] - c.snap.keys_sorted[a])
    print(f"shared key: bucket {T} m {tw.m[T]} arrivals {tw.below[T] + tw.above[T]} span {span:#x}; re-runs +{c.rise.reruns} / +{c.rise_old.reruns}")
    assert tw.below[T] + tw.above[T] == 40 and span >= 1 << 24
    assert c.rise.reruns > 0 and c.rise.reruns == c.rise_old.reruns


# ---- range lengths at the sizes where they occur ------------------------------------------------------------------------
@pytest.mark.parametrize("n,nb,L", [(1 << 20, 256, 4096), ((1 << 20) + 1, 1024, 1025)])
def test_range_length_edges(monkeypatch, n, nb, L):
    """N = 1,048,576: 256 ranges of exactly 4,096, four keys in every thread of a bucket's workgroup; one body more: 1,024
    ranges of 1,025 (the last holds two bodies).  Three dozen movers, among them the last slot of a range, ranges of every
    quarter of the array (indices >= 256 in the wide layout), the first and the last bucket as home and as destination."""
    m, p, v, side = lattice(n, 31)
    order = state_order(m, p, side)
    R = (n + L - 1) // L
    assert (n + nb - 1) // nb == L and R == nb
    movers = [5, L - 1, 3 * L - 1, (R - 1) * L + 1] + [(k * R // 32) * L + 11 + k for k in range(1, 32)]
    targets = [min((R - 1) * L + 9, n - 1), (R // 2) * L + 3, 9, 13] + [((k * R // 32 + R // 2) % (R - 1)) * L + L // 2 for k in range(1, 32)]
    assert max(movers) < n and all(s % L for s in movers)
    c = compare(monkeypatch, m, p, send_each(p, v, order, movers, targets, steps=2), 2, path="direct", k=len(movers))
    assert (c.snap.nb, c.snap.L) == (nb, L)
    tw = c.twin
    assert tw.above[0] >= 1 and tw.left[0] >= 2 and tw.left[R - 1] == 1 and tw.below[R - 1] >= 1


# ---- behind the carry ---------------------------------------------------------------------------------------------------------
def sorted_output(s):
    """what can be said of a build that was not offered direct input: its output is in order, and a permutation"""
    mask = np.uint64((1 << 40) - 1)
    assert not s.offered and s.keys_in is None and s.decision is None
    assert (np.diff((s.keys_sorted & mask).astype(np.int64)) >= 0).all()
    return s


def test_a_warm_context_uploaded_again(monkeypatch, frozen):
    """the same n, the bodies in another order: nothing of the earlier run's sorted order is theirs, so the first build is not
    offered direct input (carry.samples_n) and the second is -- with the movers under way --, and the run is bit for bit that of
    a fresh context which took no snapshot"""
    for k in ("BH_SORT_BUCKET", "BH_SORT_DIRECT", "BH_SORT_DIRECT_MAX", "BH_REORDER_EVERY"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_SORT_BUCKET", "2")
    n = 20000
    m, p, v, order, L, hull = frozen(n)
    movers = [s for s in (7 + 19 * L * k for k in range(13)) if s not in hull][:12]
    v = send_each(p, v, order, movers, far_targets(movers, L, n))
    shuffle = np.random.default_rng(41).permutation(n)
    with engine(n) as warm, engine(n) as fresh:
        warm.upload(p, np.zeros((n, 2)), m)
        warm.step(2)
        check_snapshot(warm.sort_snapshot(), path="direct", k=0)
        for e in (warm, fresh):
            e.upload(p[shuffle], v[shuffle], m[shuffle])
            e.build_tree()
        sorted_output(warm.sort_snapshot())
        for e in (warm, fresh):
            e.step(1)
            e.build_tree()
        check_snapshot(warm.sort_snapshot(), path="direct", k=12)
        for e in (warm, fresh):
            e.step(1)
        (x1, v1), (x0, v0) = warm.download()[:2], fresh.download()[:2]
        assert np.array_equal(x1, x0) and np.array_equal(v1, v0)


def test_walks_in_passes(monkeypatch, frozen):
    """n_threads = 2,048: ten walk launches per step, the bounds come from bounds_partial and not from the walk"""
    n = 20000
    m, p, v, order, L, hull = frozen(n)
    movers = [s for s in (7 + 19 * L * k for k in range(13)) if s not in hull][:12]
    c = compare(monkeypatch, m, p, send_each(p, v, order, movers, far_targets(movers, L, n)), 1, path="direct", k=12, n_threads=2048)
    assert c.new.walk_launches == 10


# ---- the snapshot itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,n_threads", quiet_case.CASES, ids=quiet_case.IDS)
def test_the_snapshot_changes_nothing(prec, n_threads):
    quiet_case.check(prec, n_threads, lambda e: e.sort_snapshot())


def code_and_text(f, *a, **kw):
    try:
        f(*a, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_where_the_snapshot_says_no():
    m, p, v, _ = lattice(5000, 51)
    with engine(5000) as e:
        e.upload(p, v, m)
        assert code_and_text(e.sort_snapshot)[0] == ERR_STATE                    # no build yet
        e.step(2)
        assert e.sort_snapshot().offered
        e.upload(p, v, m)
        assert code_and_text(e.sort_snapshot)[0] == ERR_STATE                    # another body set, no build yet
        e.build_tree()
        sorted_output(e.sort_snapshot())
        # LET mode: bh_migrate_pack reuses the sort's buffers (keys[0] among them)
        e.let_configure(0, 2, 1024)
        code, text = code_and_text(e.sort_snapshot)
        assert code == ERR_STATE and "LET" in text, (code, text)
    with engine(5000, precision=G.Precision.F64) as e:                           # an fp64 tree is never offered direct input
        e.upload(p, v, m)
        e.step(2)
        s = sorted_output(e.sort_snapshot())
        assert np.array_equal(np.sort(s.perm), np.arange(5000, dtype=np.uint32))
