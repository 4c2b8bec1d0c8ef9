"""The placement rule of the bucket sort (csrc/bh_sort.hpp "Placement"; tests/sort_place_ref.py is its numpy twin) against
numpy's stable sort: a bucket the rule takes comes out in the stable order by key, and the rule refuses exactly the buckets that
have an inversion further apart than the window (or too many descents, or a crowd under a wide span)."""
import numpy as np
import pytest

import sort_direct_ref as R
import sort_place_ref as P

W = P.WINDOW


def words_of(keys):
    return R.pack(np.asarray(keys, dtype=np.uint64))


def widest_inversion(keys):
    """the largest i - j over the pairs j < i with K_j > K_i (0: none)"""
    k = np.asarray(keys, dtype=np.int64)
    worst = 0
    for i in range(len(k)):
        j = np.flatnonzero(k[:i] > k[i])
        if len(j):
            worst = max(worst, i - int(j[0]))
    return worst


def check(keys, **kw):
    words = words_of(keys)
    taken, why, out = P.place(words, **kw)
    if taken:
        assert why is None and np.array_equal(out, R.expect(words))
    else:
        assert out is None and why in ("crossers", "size", "descents", "window", "crowd")
    return taken, why


def nearly_ordered(rng, m, moves, reach, span_bits=20):
    """m sorted keys (equal ones among them), `moves` of which are then taken out and put back up to `reach` places away"""
    k = np.sort(rng.integers(0, 1 << span_bits, m)).tolist()
    for _ in range(moves):
        a = int(rng.integers(0, m))
        b = int(np.clip(a + rng.integers(-reach, reach + 1), 0, m - 1))
        k.insert(b, k.pop(a))
    return np.array(k, dtype=np.uint64)


def test_random_nearly_ordered_sequences_against_the_stable_sort():
    rng = np.random.default_rng(1)
    took = refused = 0
    for _ in range(3000):
        m = int(rng.integers(1, 200))
        keys = nearly_ordered(rng, m, int(rng.integers(0, 6)), int(rng.integers(1, 14)))
        taken, why = check(keys)
        assert taken == (widest_inversion(keys) <= W), (keys, why)          # (span <= 20 bits, a descent per move at most: only the window rule)
        took += taken
        refused += not taken
    assert took > 1000 and refused > 200


def test_an_inversion_at_the_window_is_taken_and_one_place_further_refused():
    base = np.arange(100, 164, dtype=np.uint64) * 10
    for at in (0, 1, 20, 64 - W - 2):
        for d, want in ((W, True), (W + 1, False)):
            # a large key d places before a small one
            k = base.copy()
            if at + d >= len(k):
                continue
            k[at] = k[at + d] + 5                                            # larger than everything up to at + d, nothing beyond
            assert widest_inversion(k) == d
            assert check(k) == (want, None if want else "window")
            # a small key d places behind a large one
            k = base.copy()
            k[at + d] = k[at] - 5 if at else 0
            assert widest_inversion(k) == d
            assert check(k) == (want, None if want else "window")


def test_inversions_at_both_ends_of_a_bucket():
    k = np.arange(1, 80, dtype=np.uint64) * 3
    k[[0, 1]] = k[[1, 0]]
    k[[-1, -2]] = k[[-2, -1]]
    assert check(k) == (True, None)
    k = np.arange(1, 80, dtype=np.uint64) * 3
    k[0], k[-1] = k[W] + 1, k[-1 - W] - 1                                    # each W places from where it belongs
    assert check(k) == (True, None)
    k[0] = k[W + 1] + 1
    assert check(k) == (False, "window")


def test_short_buckets():
    assert check([7]) == (True, None)
    assert check([7, 7]) == (True, None)
    rng = np.random.default_rng(2)
    for m in range(2, W + 2):                                                # every inversion of a bucket this short is inside the window
        for _ in range(50):
            assert check(rng.integers(0, 50, m)) == (True, None)
    assert check([50] + list(range(1, W + 2))) == (False, "window")          # (m = W + 2: the first is larger than the last, W + 1 on)
    assert check(list(range(W + 2, 0, -1))) == (False, "descents")           # (reversed: W + 1 descents)


def test_equal_keys_inside_the_window_keep_their_input_order():
    k = np.array([5, 9, 9, 9, 7, 9, 9, 7, 7, 12, 9, 12], dtype=np.uint64)
    words = words_of(k)
    taken, why, out = P.place(words)
    assert taken and np.array_equal(out, R.expect(words))
    idx = (out >> np.uint64(R.PACK_SHIFT)).astype(np.int64)
    for v in (7, 9, 12):
        assert (np.diff(idx[(out & P.MASK) == v]) > 0).all()


def test_more_descents_than_the_list_holds_go_to_the_passes():
    k = np.arange(200, dtype=np.uint64) * 4
    for s in range(P.MAX_DESCENTS):
        k[[5 * s, 5 * s + 1]] = k[[5 * s + 1, 5 * s]]
    assert check(k) == (True, None)                                          # as many adjacent swaps as the list holds
    k[[190, 191]] = k[[191, 190]]
    assert check(k) == (False, "descents")


def test_the_crowd_rule():
    F = P.FIX_RUN
    wide = 1 << 30                                                           # span 31 bits: the top 24 drop the low 7
    spread = np.arange(60, dtype=np.uint64) * np.uint64(1 << 10)
    # F + 1 keys inside one 2^7 cell under the wide span: refused; F of them: taken; the same F + 1 under a span of 24 bits: taken
    crowd = np.uint64((5 << 10) + 512) + np.arange(F + 1, dtype=np.uint64)
    k = np.sort(np.concatenate([spread, crowd, [np.uint64(wide)]]))
    assert check(k) == (False, "crowd")
    assert check(np.sort(np.concatenate([spread, crowd[:F], [np.uint64(wide)]]))) == (True, None)
    assert check(np.sort(np.concatenate([spread, crowd, [np.uint64((1 << 24) - 1)]]))) == (True, None)
    # equal keys crowd like any others; all keys equal is a span of no bits
    k = np.sort(np.concatenate([spread, np.full(F + 1, 777, dtype=np.uint64), [np.uint64(wide)]]))
    assert check(k) == (False, "crowd")
    assert check(np.full(40, 777)) == (True, None)
    # the cells are counted from the smallest key: nine keys that straddle a multiple of 2^7 share a cell of the span all the same
    low = np.uint64((1 << 20) + 125)
    k = np.concatenate([[low], low + np.uint64(1 << 12) + np.arange(F + 1, dtype=np.uint64), [low + np.uint64(wide)]])
    assert check(k) == (False, "crowd")


def test_paths_counts_buckets_and_names_the_rules():
    ordered = words_of(np.arange(50, dtype=np.uint64))
    far = words_of(np.concatenate([[np.uint64(99)], np.arange(50, dtype=np.uint64)]))
    placed, passed, why = P.paths([(0, ordered, 0), (3, far, 0), (4, ordered[:1], 0)])
    assert (placed, passed, why) == (2, 1, {3: "window"})
    # a single-bucket launch's input is recovered from its output
    rng = np.random.default_rng(3)
    w = words_of(nearly_ordered(rng, 300, 4, 5))
    s = R.expect(w)
    (b, words, arrivals), = P.single_input(s & P.MASK, (s >> np.uint64(R.PACK_SHIFT)).astype(np.uint32))
    assert (b, arrivals) == (0, 0) and np.array_equal(words, w)


def test_a_build_with_crossers_and_a_bucket_beyond_the_tiers_are_not_tested():
    ordered = words_of(np.arange(50, dtype=np.uint64))
    assert P.place(ordered)[:2] == (True, None)
    assert P.place(ordered, crossers=1)[:2] == (False, "crossers")           # in order all the same: who is tested, not what is found
    assert P.paths([(7, ordered, 2)]) == (0, 1, {7: "crossers"})
    assert P.place(words_of(np.arange(P.PLACE_CAP, dtype=np.uint64)))[:2] == (True, None)
    assert P.place(words_of(np.arange(P.PLACE_CAP + 1, dtype=np.uint64)))[:2] == (False, "size")


def test_bucket_inputs_of_a_direct_build():
    # four ranges of four; the key at slot 1 belongs into range 2, the key at slot 13 into range 0: nothing is placed
    keys = np.array([0, 95, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, 5, 140, 150], dtype=np.uint64)
    words = words_of(keys)
    tw = R.direct_sort_fast(words, 4, 16)
    assert tw.path == "direct" and tw.k == 2
    got = {b: (w & P.MASK).tolist() for b, w, _ in P.bucket_inputs(words, tw)}
    assert got == {0: [0, 20, 30, 5], 1: [40, 50, 60, 70], 2: [95, 80, 90, 100, 110], 3: [120, 140, 150]}
    assert P.paths(P.bucket_inputs(words, tw)) == (0, 4, dict.fromkeys(range(4), "crossers"))
    # without crossers the ranges as they stand, one swap in range 1: all placed
    keys = np.array([0, 10, 20, 30, 40, 60, 50, 70, 80, 90, 100, 110, 120, 130, 140, 150], dtype=np.uint64)
    tw = R.direct_sort_fast(words_of(keys), 4, 16)
    assert tw.path == "direct" and tw.k == 0
    assert P.paths(P.bucket_inputs(words_of(keys), tw)) == (4, 0, {})
