"""A numpy twin of the bucket sort's direct input (csrc/bh_sort.hpp, "direct input") against np.argsort(kind="stable").

The twin follows the device code statement by statement: bucket b owns the array range [b * L, (b + 1) * L), L = ceil(n / nb);
range key j is the key at j * L (0 for j = 0, "infinity" for a range that starts at or beyond n); a key stays iff
range key b <= key < range key b + 1 -- which is bucket_of(key) == b while the range keys are in order --, every other key is
a crosser, routed by bucket_of; a bucket's input is its arrivals from lower ranges, its stayers, its arrivals from higher
ranges, each in body order; the bucket is sorted stably on the 40 key bits; its place in the output follows from what the
buckets before it gained and lost.  Range keys out of order, or more crossers than the list holds: the counting pass, i.e.
the stable order by bucket among the SORTED range keys and then the same sort of every bucket."""
import numpy as np
import pytest

PACK_SHIFT = 40
KEY_MASK = (1 << PACK_SHIFT) - 1
INF = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack(keys40):
    keys40 = np.asarray(keys40, dtype=np.uint64)
    return keys40 | (np.arange(len(keys40), dtype=np.uint64) << np.uint64(PACK_SHIFT))


def bucket_of(key40, spl):
    """largest j with spl[j] <= key: the device's binary search (spl in order, spl[0] = 0, len a power of two)"""
    b, s = 0, len(spl) >> 1
    while s >= 1:
        b += s if spl[b + s] <= key40 else 0
        s >>= 1
    return b


def range_keys(words, nb):
    n = len(words)
    L = (n + nb - 1) // nb
    rk = np.full(nb, INF, dtype=np.uint64)
    for j in range(nb):
        if j == 0:
            rk[j] = 0
        elif j * L < n:
            rk[j] = words[j * L] & np.uint64(KEY_MASK)
    return rk, L


def sort_bucket_stable(words):
    """what bucket_sort_kernel does to one bucket's input: the stable order by the 40 key bits"""
    words = np.asarray(words, dtype=np.uint64)
    return words[np.argsort(words & np.uint64(KEY_MASK), kind="stable")]


def direct_sort(words, nb, cap):
    """-> (sorted packed words, 'direct' | 'counting', number of crossers or None)"""
    words = np.asarray(words, dtype=np.uint64)
    n = len(words)
    rk, L = range_keys(words, nb)
    in_order = bool(np.all(rk[:-1] <= rk[1:]))
    key40 = words & np.uint64(KEY_MASK)
    crossers = []
    if in_order:
        for i in range(n):
            b = i // L
            hi = rk[b + 1] if b + 1 < nb else INF
            if not (rk[b] <= key40[i] < hi):
                crossers.append(i)
    if not in_order or len(crossers) > cap:
        spl = np.sort(rk)
        dest = np.array([bucket_of(k, spl) for k in key40], dtype=np.int64)
        out = []
        for b in range(nb):
            out.append(sort_bucket_stable(words[dest == b]))               # (boolean mask: body order, as the stable scatter leaves it)
        return np.concatenate(out), "counting", (len(crossers) if in_order else None)
    # the direct path
    dest = {i: bucket_of(key40[i], rk) for i in crossers}
    for i, d in dest.items():
        assert d != i // L                                                   # stays_in and bucket_of agree
    gone = set(crossers)
    out = np.empty(n, dtype=np.uint64)
    starts = []
    pos = 0
    for b in range(nb):
        r0, r1 = min(n, b * L), min(n, (b + 1) * L)
        arrivals = sorted(i for i, d in dest.items() if d == b)
        lower = [words[i] for i in arrivals if i < r0]
        upper = [words[i] for i in arrivals if i >= r0]
        stay = [words[i] for i in range(r0, r1) if i not in gone]
        left = sum(1 for i in crossers if i // L == b)
        assert len(stay) == (r1 - r0) - left
        m = len(lower) + len(stay) + len(upper)
        # the device's start: range start + net arrivals of the buckets before
        net_before = sum(1 for i, d in dest.items() if d < b) - sum(1 for i in crossers if i // L < b)
        assert r0 + net_before == pos
        starts.append(pos)
        out[pos:pos + m] = sort_bucket_stable(np.array(lower + stay + upper, dtype=np.uint64))
        pos += m
    assert pos == n
    return out, "direct", len(crossers)


def expect(words):
    words = np.asarray(words, dtype=np.uint64)
    return words[np.argsort(words & np.uint64(KEY_MASK), kind="stable")]


def check(keys40, nb=256, cap=1 << 30, want=None):
    words = pack(keys40)
    got, path, k = direct_sort(words, nb, cap)
    assert np.array_equal(got, expect(words))
    # (the body index in the word: equal keys must come out in body order, which array_equal on the words checks)
    if want is not None:
        assert path == want, (path, k)
    return path, k


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
        path, k = check(np.full(n, 123456789, dtype=np.uint64), want="direct")
        L = (n + 255) // 256
        assert k == ((n - 1) // L) * L


def test_runs_of_equal_keys_across_range_boundaries():
    n = 9000
    L = (n + 255) // 256
    keys = sorted_keys(n)
    keys[5 * L - 3:7 * L + 4] = keys[5 * L - 3]            # one value across two boundaries: range keys 5, 6 and 7 are equal
    keys[20 * L - 1:20 * L + 1] = keys[20 * L - 1]           # ... and a pair astride one
    path, k = check(keys, want="direct")
    assert k > 0                                              # (the run's bodies left of the last equal range key cross)
    # the same with some of the run moved to the far end of the array
    keys2 = keys.copy()
    keys2[240 * L + 1:240 * L + 6] = keys[5 * L]
    check(keys2, want="direct")


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
