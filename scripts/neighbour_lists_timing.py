"""What a neighbour-list query costs: the passes of bh_neighbour_lists by HIP events, beside count_within at the same radius.

    python scripts/neighbour_lists_timing.py [--n 1048576] [--repeats 7] [--ks 1 8 32] [--precision F32] [--kind plummer]

One context on the quasi-static Plummer state of scripts/neighbours_timing.py (scale radius 0.02, max_depth 21), 5 + 16 untimed
steps, so that the fp32 state has been physically re-ordered as in a run.  The radii are the median distances of the k-th
neighbour for the k of --ks, from one neighbours(max k) call.  Per radius, after one untimed call, `repeats` calls of
neighbours_within(radius, with_stats=True) over all bodies; the times are the library's own HIP events of the filling call
(bh_neighbour_lists_times):
  build: bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes;
  count: the counting traversal of every launch of 2^20 queries;
  fill:  the scan of a launch's row lengths and the filling traversal, summed over the launches of BH_LISTS_ENTRIES entries;
  sort:  the row sorts of those launches (rows of up to 8 entries are in order when the fill pass ends: they cost nothing here);
  call:  the host clock around neighbours_within: both calls, downloads and the host's placing of the rows included.
Then `repeats` calls of count_within at the same radius -- the floor: one traversal, no entries -- and, once, of neighbours(8).
A row is the median over the repeats with their minimum and maximum.  Prints one JSON line per radius and one for neighbours(8).
Development aid, not a bench."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--kind", choices=["plummer", "uniform"], default="plummer")
ap.add_argument("--no-reorder", action="store_true", help="query the state in upload order (no steps at all)")
a = ap.parse_args()


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 4), round(float(x.min()), 4), round(float(x.max()), 4)]


prec = G.Precision[a.precision]
m, p, v = IC.make(a.kind, a.n, 1, quasi_static=True)
reordered = not a.no_reorder and prec != G.Precision.F64
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                  reference_compat=prec == G.Precision.F64)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    if not a.no_reorder:
        e.step(5 + 16)
    common = {"precision": prec.name, "kind": a.kind, "n": a.n, "reordered": reordered, "repeats": a.repeats}
    d2 = e.neighbours(max(a.ks))[1]
    radii = {k: float(np.sqrt(np.median(d2[:, k - 1]))) for k in a.ks}
    del d2
    for k, radius in radii.items():
        e.neighbours_within(radius)
        t = {name: [] for name in ("build", "count", "fill", "sort", "call", "floor_build", "floor_query")}
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            nl = e.neighbours_within(radius, with_stats=True)
            t["call"].append((time.perf_counter() - t0) * 1e3)
            for name, ms in zip(("build", "count", "fill", "sort"), e.neighbour_lists_times()):
                t[name].append(ms)
        evals, opened, entries, longest = nl.stats
        long_rows = int((nl.counts > 8).sum())
        del nl
        for _ in range(a.repeats):
            e.count_within(radius)
            b, q = e.neighbours_times()
            t["floor_build"].append(b)
            t["floor_query"].append(q)
        fill, sort, floor = (float(np.median(t[name])) for name in ("fill", "sort", "floor_query"))
        print(json.dumps({**common, "query": "neighbours_within", "radius_of_k": k, "radius": radius, "entries": entries,
                          "longest_row": longest, "rows_over_8": long_rows, "evals_mean": round(evals / a.n, 2),
                          "opened_mean": round(opened / a.n, 2),
                          **{name + "_ms [median, min, max]": row(x) for name, x in t.items()},
                          "entries_per_ms_of_fill_and_sort": round(entries / (fill + sort), 1),
                          "count_over_floor": round(float(np.median(t["count"])) / floor, 3),
                          "fill_over_floor": round(fill / floor, 3), "sort_over_floor": round(sort / floor, 3)}), flush=True)
    build, query = [], []
    for _ in range(a.repeats):
        e.neighbours(8)
        b, q = e.neighbours_times()
        build.append(b)
        query.append(q)
    print(json.dumps({**common, "query": "neighbours", "k": 8, "build_ms [median, min, max]": row(build),
                      "query_ms [median, min, max]": row(query)}), flush=True)
