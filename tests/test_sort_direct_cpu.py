"""The numpy twin of the bucket sort's direct input (tests/sort_direct_ref.py: the algorithm and the device's decision rules are
described there) against np.argsort(kind="stable"), the loop version against the vectorised one, and both sides of every rule
of the decision."""
import numpy as np
import pytest

from sort_direct_ref import WAVE, direct_sort, direct_sort_fast, expect, pack


def same(a, b):
    """two Twins agree in everything"""
    assert a.path == b.path and a.k == b.k and a.why == b.why and a.L == b.L
    for f in ("out", "rk", "crossers", "below", "above", "left", "m"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        assert x is None or np.array_equal(x, y), f


def check(keys40, nb=256, cap=1 << 30, want=None, subcap=None, nsub=1, half_wave=WAVE // 2):
    words = pack(keys40)
    tw = direct_sort(words, nb, cap, subcap, nsub, half_wave)
    same(tw, direct_sort_fast(words, nb, cap, subcap, nsub, half_wave))
    assert np.array_equal(tw.out, expect(words))
    # (the body index in the word: equal keys must come out in body order, which array_equal on the words checks)
    if want is not None:
        assert tw.path == want, (tw.path, tw.k, tw.why)
    if tw.path == "direct":
        assert tw.below.sum() + tw.above.sum() == tw.left.sum() == tw.k == len(tw.crossers)
    return tw.path, tw.k


RNG = np.random.default_rng(17)


def sorted_keys(n, distinct=True):
    k = np.sort(RNG.integers(0, 1 << 40, n, dtype=np.uint64))
    return k


@pytest.mark.parametrize("n", [4097, 8192, 8191 + 4 * 64 + 1, 10000])
def test_sorted_input_has_no_crosser(n):
    path, k = check(sorted_keys(n), want="direct")
    assert k == 0


@pytest.mark.parametrize("n,swaps", [(4100, 1), (9000, 12), (9000, 300), (20000, 3000)])
def test_random_swaps(n, swaps):
    keys = sorted_keys(n)
    L = (n + 255) // 256
    for _ in range(swaps):
        # (not the bodies at range starts: out-of-order range keys are the other test)
        i, j = RNG.integers(0, n, 2)
        if i % L == 0 or j % L == 0:
            continue
        keys[i], keys[j] = keys[j], keys[i]
    path, k = check(keys, want="direct")
    assert k > 0


def test_range_keys_out_of_order_take_the_counting_pass():
    n = 9000
    keys = sorted_keys(n)
    L = (n + 255) // 256
    keys[3 * L], keys[200 * L] = keys[200 * L], keys[3 * L]
    check(keys, want="counting")


def test_both_sides_of_the_capacity():
    n = 9000
    keys = sorted_keys(n)
    L = (n + 255) // 256
    movers = [5, L + 7, 9 * L + 3, 40 * L + 1, 41 * L + 2, 100 * L + 9, 180 * L + 5, 240 * L + 3]
    far = [200 * L + 1, 3, 90 * L + 1, 90 * L + 2, 90 * L + 3, 245 * L + 4, 2 * L + 2, 10 * L + 1]
    for i, j in zip(movers, far):
        keys[i] = keys[j]                     # lands beside body j, in j's bucket (an equal key: body order decides)
    path, k = check(keys, cap=1 << 30, want="direct")
    assert k == 8
    check(keys, cap=8, want="direct")
    check(keys, cap=7, want="counting")


def test_all_keys_equal():
    for n in (4097, 9000):
        # every range key but the first is the one value: bucket_of sends every body to the LAST range that has that key,
        # and only the bodies of that range stay
        # (whole waves cross: the device's wave rule sends such a build to the counting pass; the routing is checked without it)
        path, k = check(np.full(n, 123456789, dtype=np.uint64), want="direct", half_wave=WAVE)
        L = (n + 255) // 256
        assert k == ((n - 1) // L) * L
        assert check(np.full(n, 123456789, dtype=np.uint64), want="counting") == ("counting", k)


def test_runs_of_equal_keys_across_range_boundaries():
    n = 9000
    L = (n + 255) // 256
    keys = sorted_keys(n)
    keys[5 * L - 3:7 * L + 4] = keys[5 * L - 3]            # one value across two boundaries: range keys 5, 6 and 7 are equal
    keys[20 * L - 1:20 * L + 1] = keys[20 * L - 1]           # ... and a pair astride one
    # (2 L = 70 neighbours cross, more than half of some wave: routed without the wave rule, the counting pass with it)
    path, k = check(keys, want="direct", half_wave=WAVE)
    assert k > 0                                              # (the run's bodies left of the last equal range key cross)
    check(keys, want="counting")
    # the same with some of the run moved to the far end of the array
    keys2 = keys.copy()
    keys2[240 * L + 1:240 * L + 6] = keys[5 * L]
    check(keys2, want="direct", half_wave=WAVE)
    # a run short enough for the rule: a dozen equal keys astride one boundary
    keys3 = sorted_keys(n)
    keys3[30 * L - 6:30 * L + 6] = keys3[30 * L - 6]
    assert check(keys3, want="direct") == ("direct", 6)


@pytest.mark.parametrize("n", [4097, 4099, 8191 + 4 * 64 + 1, 12345])
def test_uneven_ranges_and_empty_trailing_ranges(n):
    keys = sorted_keys(n)
    L = (n + 255) // 256
    # (4,097 and 4,099: 241 ranges of 17, the last one shorter, 15 empty ones behind; 8,448 = 256 x 33 divides evenly;
    #  12,345: 253 ranges of 49, the last one shorter, three empty)
    # a body of the first range into the last non-empty one and back, and one to the very end
    last = (n - 1) // L
    keys[1], keys[last * L + 1] = keys[last * L + 1], keys[1]
    keys[L + 1] = (1 << 40) - 1
    path, k = check(keys, want="direct")
    assert k == 3


def test_a_third_of_the_bodies_crossing():
    n = 12000
    keys = sorted_keys(n)
    L = (n + 255) // 256
    idx = np.array([i for i in RNG.permutation(n)[:n // 3] if i % L != 0])
    keys[idx] = keys[RNG.permutation(idx)]
    path, k = check(keys, want="direct")
    assert k > n // 5


# ---- the decision in full: T crossers in all, 64 lists of `subcap`, no wave with more than half its bodies crossing ----------------
N, NB, T, SUBCAP, NSUB = 20000, 256, 1024, 64, 64            # the device's defaults: list = (slot >> 6) & 63
LEN = (N + NB - 1) // NB                                      # 79


def moved(slots):
    """sorted distinct keys in which the bodies of `slots` (no range starts) have the key of a body half the array away"""
    keys = np.sort(np.random.default_rng(23).choice(1 << 40, N, replace=False).astype(np.uint64))
    orig = keys.copy()
    slots = np.asarray(slots, dtype=np.int64)
    assert len(set(slots.tolist())) == len(slots) and (slots % LEN != 0).all()
    keys[slots] = orig[(slots + 120 * LEN) % N]
    return keys, slots


def in_wave(w, count):
    """the first `count` slots of wave w that are no range starts"""
    return [s for s in range(WAVE * w, WAVE * (w + 1)) if s % LEN != 0][:count]


def decide(slots, want, why=()):
    keys, slots = moved(slots)
    words = pack(keys)
    for f in (direct_sort, direct_sort_fast):
        tw = f(words, NB, T, SUBCAP, NSUB)
        assert (tw.path, tw.why, tw.k) == (want, why, len(slots))
        assert np.array_equal(tw.crossers, np.sort(slots))
        assert np.array_equal(tw.out, expect(words))
    same(direct_sort(words, NB, T, SUBCAP, NSUB), direct_sort_fast(words, NB, T, SUBCAP, NSUB))


def test_a_list_holds_its_room_and_not_one_more():
    # waves 5, 69, 133 and 197 share list 5
    four = sum((in_wave(w, 16) for w in (5, 69, 133, 197)), [])
    decide(four, "direct")
    decide(four + [in_wave(261, 1)[0]], "counting", ("list",))
    decide(four + [in_wave(6, 1)[0]], "direct")                # (the 65th crosser in ANOTHER list changes nothing)


def test_half_a_wave_may_cross_and_not_one_more():
    decide(in_wave(7, 32), "direct")
    decide(in_wave(7, 33), "counting", ("wave",))
    decide(in_wave(7, 32) + in_wave(8, 32), "direct")          # (two neighbouring waves, half of each)


def test_the_total_holds_t_and_not_one_more():
    full = sum((in_wave(w, 16) for w in range(64)), [])        # 16 in every list: no list over 64, no wave over 32
    assert len(full) == T
    decide(full, "direct")
    decide(full + [in_wave(100, 1)[0]], "counting", ("total",))


def test_range_keys_out_of_order_are_named():
    keys, _ = moved([])
    keys[3 * LEN], keys[200 * LEN] = keys[200 * LEN], keys[3 * LEN]
    for f in (direct_sort, direct_sort_fast):
        tw = f(pack(keys), NB, T, SUBCAP, NSUB)
        assert (tw.path, tw.why, tw.k, tw.crossers) == ("counting", ("order",), None, None)


@pytest.mark.parametrize("seed", range(6))
def test_the_two_twins_agree_on_random_small_inputs(seed):
    """random sizes, bucket counts, rooms and disorder -- range starts included, so every rule fires in some case"""
    rng = np.random.default_rng(100 + seed)
    fired = set()
    for _ in range(12):
        nb = int(rng.choice([4, 16, 64]))
        n = int(rng.integers(nb + 1, 1500))
        keys = np.sort(rng.integers(0, 1 << int(rng.choice([6, 40])), n, dtype=np.uint64))
        for _ in range(int(rng.choice([0, 1, 3, 40, 400]))):
            i, j = rng.integers(0, n, 2)
            keys[i] = keys[j]
        nsub = int(rng.choice([1, 4, 64]))
        cap = int(rng.choice([2, 8, 64, 1 << 20]))
        subcap = None if nsub == 1 else int(rng.choice([1, 4, 16]))
        words = pack(keys)
        a, b = direct_sort(words, nb, cap, subcap, nsub), direct_sort_fast(words, nb, cap, subcap, nsub)
        same(a, b)
        assert np.array_equal(a.out, expect(words))
        fired.update(a.why or ("none",))
    assert len(fired) >= 3
