"""A numpy twin of the bucket sort's direct input (csrc/bh_sort.hpp "direct input", keys_kernel in csrc/bh_tree.hpp; DESIGN.md
section 3.1), for tests/test_sort_direct_cpu.py (keys made up in Python) and tests/test_gpu_sort_direct*.py (the device's own keys,
through BarnesHutEngine.sort_snapshot).

The twin follows the device code statement by statement: bucket b owns the array range [b * L, (b + 1) * L), L = ceil(n / nb);
range key j is the key at j * L (0 for j = 0, "infinity" for a range that starts at or beyond n); a key stays iff
range key b <= key < range key b + 1 -- which is bucket_of(key) == b while the range keys are in order --, every other key is
a crosser, routed by bucket_of; a bucket's input is its arrivals from lower ranges, its stayers, its arrivals from higher
ranges, each in body order; the bucket is sorted stably on the 40 key bits; its place in the output follows from what the
buckets before it gained and lost.

The decision is the device's in full.  The build takes the counting pass iff
  "order": the range keys are out of order, or
  "wave":  some wave of 64 consecutive slots (slot >> 6) has more than 32 crossers, or
  "list":  some list -- the crossers of wave w go to list w & (nsub - 1) -- holds more than subcap crossers, or
  "total": there are more than cap crossers in all;
and then its output is the stable sort whatever the splitters were.

direct_sort is the loop version (small inputs), direct_sort_fast the same with searchsorted / bincount / lexsort (a million keys);
both return a Twin.  (half_wave = 64 switches the wave rule off, for the tests of the routing in which whole ranges cross.)"""
from dataclasses import dataclass

import numpy as np

PACK_SHIFT = 40
KEY_MASK = (1 << PACK_SHIFT) - 1
INF = np.uint64(0xFFFFFFFFFFFFFFFF)
WAVE = 64


@dataclass
class Twin:
    out: np.ndarray              # the sorted packed words
    path: str                    # "direct" | "counting"
    k: int                       # crossers (None when the range keys are out of order: nobody is routed then)
    why: tuple                   # the rules that send the build to the counting pass, in the order above; () on the direct path
    rk: np.ndarray               # (nb,) range keys
    L: int
    crossers: np.ndarray = None  # slots of the crossers, ascending (None when the range keys are out of order)
    # per bucket, on the direct path only: arrivals from lower ranges, from higher ranges, departures, keys to sort
    below: np.ndarray = None
    above: np.ndarray = None
    left: np.ndarray = None
    m: np.ndarray = None


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


def range_keys_fast(words, nb):
    n = len(words)
    L = (n + nb - 1) // nb
    rk = np.full(nb, INF, dtype=np.uint64)
    j = np.arange(nb, dtype=np.int64)
    has = (j > 0) & (j * L < n)
    rk[has] = words[j[has] * L] & np.uint64(KEY_MASK)
    rk[0] = 0
    return rk, L


def sort_bucket_stable(words):
    """what bucket_sort_kernel does to one bucket's input: the stable order by the 40 key bits"""
    words = np.asarray(words, dtype=np.uint64)
    return words[np.argsort(words & np.uint64(KEY_MASK), kind="stable")]


def expect(words):
    words = np.asarray(words, dtype=np.uint64)
    return words[np.argsort(words & np.uint64(KEY_MASK), kind="stable")]


def rooms(cap, subcap, nsub):
    """(cap, subcap, nsub) with the defaults of a build that lists every body: one list as large as the total"""
    return cap, (cap if subcap is None else subcap), nsub


def direct_sort(words, nb, cap, subcap=None, nsub=1, half_wave=WAVE // 2):
    words = np.asarray(words, dtype=np.uint64)
    cap, subcap, nsub = rooms(cap, subcap, nsub)
    n = len(words)
    rk, L = range_keys(words, nb)
    in_order = bool(np.all(rk[:-1] <= rk[1:]))
    key40 = words & np.uint64(KEY_MASK)
    why = [] if in_order else ["order"]
    crossers = []
    if in_order:
        for i in range(n):
            b = i // L
            hi = rk[b + 1] if b + 1 < nb else INF
            if not (rk[b] <= key40[i] < hi):
                crossers.append(i)
        waves, lists = {}, {}
        for i in crossers:
            waves[i >> 6] = waves.get(i >> 6, 0) + 1
            lists[(i >> 6) & (nsub - 1)] = lists.get((i >> 6) & (nsub - 1), 0) + 1
        if any(v > half_wave for v in waves.values()):
            why.append("wave")
        if any(v > subcap for v in lists.values()):
            why.append("list")
        if len(crossers) > cap:
            why.append("total")
    if why:
        # (the counting pass routes by splitters of its own; whatever they are, the result is the stable sort)
        return Twin(expect(words), "counting", len(crossers) if in_order else None, tuple(why), rk, L,
                    np.array(crossers, dtype=np.int64) if in_order else None)
    # the direct path
    dest = {i: bucket_of(key40[i], rk) for i in crossers}
    for i, d in dest.items():
        assert d != i // L                                                   # stays_in and bucket_of agree
    gone = set(crossers)
    out = np.empty(n, dtype=np.uint64)
    below, above, left, ms = (np.zeros(nb, dtype=np.int64) for _ in range(4))
    pos = 0
    for b in range(nb):
        r0, r1 = min(n, b * L), min(n, (b + 1) * L)
        arrivals = sorted(i for i, d in dest.items() if d == b)
        lower = [words[i] for i in arrivals if i < r0]
        upper = [words[i] for i in arrivals if i >= r0]
        stay = [words[i] for i in range(r0, r1) if i not in gone]
        left[b] = sum(1 for i in crossers if i // L == b)
        assert len(stay) == (r1 - r0) - left[b]
        m = len(lower) + len(stay) + len(upper)
        below[b], above[b], ms[b] = len(lower), len(upper), m
        # the device's start: range start + net arrivals of the buckets before
        net_before = sum(1 for i, d in dest.items() if d < b) - sum(1 for i in crossers if i // L < b)
        assert r0 + net_before == pos
        out[pos:pos + m] = sort_bucket_stable(np.array(lower + stay + upper, dtype=np.uint64))
        pos += m
    assert pos == n
    return Twin(out, "direct", len(crossers), (), rk, L, np.array(crossers, dtype=np.int64), below, above, left, ms)


def direct_sort_fast(words, nb, cap, subcap=None, nsub=1, half_wave=WAVE // 2):
    """direct_sort without a Python loop over keys or buckets"""
    words = np.asarray(words, dtype=np.uint64)
    cap, subcap, nsub = rooms(cap, subcap, nsub)
    n = len(words)
    rk, L = range_keys_fast(words, nb)
    key40 = words & np.uint64(KEY_MASK)
    if not bool(np.all(rk[:-1] <= rk[1:])):
        return Twin(expect(words), "counting", None, ("order",), rk, L)
    slot = np.arange(n, dtype=np.int64)
    home = slot // L
    hi = np.append(rk, INF)[home + 1]
    crossers = np.flatnonzero(~((rk[home] <= key40) & (key40 < hi)))
    waves = np.bincount(crossers >> 6, minlength=1)
    lists = np.bincount((crossers >> 6) & (nsub - 1), minlength=nsub)
    why = []
    if (waves > half_wave).any():
        why.append("wave")
    if (lists > subcap).any():
        why.append("list")
    if len(crossers) > cap:
        why.append("total")
    if why:
        return Twin(expect(words), "counting", len(crossers), tuple(why), rk, L, crossers)
    dest = home.copy()
    to = np.searchsorted(rk, key40[crossers], side="right").astype(np.int64) - 1     # largest j with rk[j] <= key
    assert not (to == home[crossers]).any()
    dest[crossers] = to
    below = np.bincount(to[to > home[crossers]], minlength=nb)
    above = np.bincount(to[to < home[crossers]], minlength=nb)
    left = np.bincount(home[crossers], minlength=nb)
    size = np.clip(n - np.arange(nb, dtype=np.int64) * L, 0, L)
    m = size - left + below + above
    assert m.sum() == n and (m >= 0).all()
    # a bucket's input -- arrivals from below, stayers, arrivals from above, each in body order -- IS the body order of the
    # keys it is sent (arrivals from below stand before its range, those from above behind it); its sort is stable on the key
    out = words[np.lexsort((key40, dest))]
    return Twin(out, "direct", len(crossers), (), rk, L, crossers, below, above, left, m)
