"""A numpy twin of the bucket sort's placement path (csrc/bh_sort.hpp "Placement"), for
tests/test_sort_place_cpu.py (keys made up in Python) and tests/test_gpu_sort_place.py (the device's own keys, through
BarnesHutEngine.sort_snapshot and sort_paths).

Only two kinds of bucket are tested at all: the one bucket of a single-bucket launch, and the ranges of a direct build in which no
body changed bucket.  The buckets of a build that took the counting pass go through the byte passes untested.

One bucket's input is its packed words in input order, K_i the 40 key bits.  A pair j < i with K_j > K_i is an inversion (equal
keys are none: the sort is stable).  The bucket is finished by placement iff none of these refuses it, looked at in this order:
  "crossers": its build has crossers (bodies on their way: the test then costs more than it saves);
  "size":     it holds more than PLACE_CAP keys (the tiers of the in-LDS sort that have the path; a range of a direct build
              and a single-bucket launch never do);
  "descents": more than MAX_DESCENTS positions i have K_i < K_{i-1};
  "window":   some inversion has i - j > window;
  "crowd":    the span max K - min K needs more than 24 bits and some K_i, K_{i + fix_run} (input order) are equal in the top
              24 bits of (K - min K) -- such a bucket keeps the byte passes and their re-run;
and then key i goes to  i - #{j in [i - window, i): K_j > K_i} + #{j in (i, i + window]: K_j < K_i},  which is its stable rank.
Everything else goes through the byte passes.  The order is the stable order by key on either path."""
import numpy as np

import sort_direct_ref as R

WINDOW = 8                  # kPlaceWindow
FIX_RUN = 8                 # kFixRun
MAX_DESCENTS = 8            # kPlaceMaxDescents
PLACE_CAP = 4 * 1024        # kPlaceItemsMax keys per thread of 1,024
MASK = np.uint64(R.KEY_MASK)


def place(words, window=WINDOW, fix_run=FIX_RUN, max_descents=MAX_DESCENTS, crossers=0):
    """-> (taken, why, out_words): why is None when the bucket is placed; out_words is the rule's own write-out then (every
    key at the rank the two window counts give it) and None when it is refused.  crossers: those of the bucket's build"""
    words = np.asarray(words, dtype=np.uint64)
    m = len(words)
    k = (words & MASK).astype(np.int64)
    if crossers:
        return False, "crossers", None
    if m > PLACE_CAP:
        return False, "size", None
    if int((k[1:] < k[:-1]).sum()) > max_descents:
        return False, "descents", None
    # the largest key at least window + 1 places before i
    if m > window + 1:
        before = np.maximum.accumulate(k)[:m - window - 1]
        if (before > k[window + 1:]).any():
            return False, "window", None
    span = int(k.max() - k.min()) if m else 0
    bits = span.bit_length()
    if bits > 24 and m > fix_run:
        top = (k - k.min()) >> (bits - 24)
        if (top[:-fix_run] == top[fix_run:]).any():
            return False, "crowd", None
    rank = np.arange(m, dtype=np.int64)
    for d in range(1, window + 1):
        if d >= m:
            break
        inv = k[:-d] > k[d:]                         # pair (i - d, i)
        rank[d:] -= inv
        rank[:-d] += inv
    out = np.empty(m, dtype=np.uint64)
    assert np.array_equal(np.sort(rank), np.arange(m))
    out[rank] = words
    return True, None, out


def bucket_inputs(keys_in, twin):
    """[(bucket, words, crossers of the build)] of a direct build (twin: sort_direct_ref's answer for keys_in, on the direct path), empty buckets
    left out: arrivals from lower ranges, stayers, arrivals from higher ranges, each in body order -- which is the body order of
    the keys a bucket is sent"""
    assert twin.path == "direct"
    n, nb, L = len(keys_in), len(twin.rk), twin.L
    key40 = keys_in & MASK
    dest = np.arange(n, dtype=np.int64) // L
    if twin.k:
        dest[twin.crossers] = np.searchsorted(twin.rk, key40[twin.crossers], side="right").astype(np.int64) - 1
    by = np.argsort(dest, kind="stable")
    cuts = np.searchsorted(dest[by], np.arange(nb + 1))
    return [(b, keys_in[by[cuts[b]:cuts[b + 1]]], int(twin.k)) for b in range(nb) if cuts[b + 1] > cuts[b]]


def single_input(keys_sorted, perm):
    """a single-bucket launch's input from its output: slot i held body i's word, key | i << 40"""
    n = len(perm)
    words = np.empty(n, dtype=np.uint64)
    words[perm] = keys_sorted | (perm.astype(np.uint64) << np.uint64(R.PACK_SHIFT))
    return [(0, words, 0)]


def paths(inputs, **kw):
    """-> (placed, passed, why): how many of the buckets are placed, how many take the passes, and {bucket: rule} of the refused;
    every placed bucket's write-out is checked against the stable sort on the way"""
    placed, passed, why = 0, 0, {}
    for b, words, crossers in inputs:
        taken, rule, out = place(words, crossers=crossers, **kw)
        if taken:
            assert np.array_equal(out, R.expect(words)), b
            placed += 1
        else:
            why[b] = rule
            passed += len(np.unique(words & MASK)) > 1       # (equal keys are written out as they stand: neither counter)
    return placed, passed, why
