"""What a neighbour query costs: the structure's build and the searches of bh_neighbours / bh_count_within by HIP events.

    python scripts/neighbours_timing.py [--n 1048576] [--repeats 7] [--ks 1 8 32] [--precision F32] [--kind plummer]

One context on the quasi-static Plummer state of scripts/moment_map_timing.py (scale radius 0.02, max_depth 21), 5 + 16 untimed
steps, so that the fp32 state has been physically re-ordered as in a run.  Per k, after one untimed call, `repeats` calls of
neighbours(k, with_evals=True) over all bodies; then count_within over all bodies at the radius, found by bisection, that
encloses about 8 bodies on average.  The times are the library's own HIP events (bh_neighbours_times):
  build: bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes;
  query: the search kernel of every launch of 2^20 queries (downloads and the host's scatter into caller order excluded);
  call:  the host clock from the call to its return, downloads and scatter included.
A row is the median over the repeats with their minimum and maximum.  Algorithmic bytes:
  build: per body 2 reads of the position (bounds, keys), 8 for the key, 24 per sort pass (histogram read, scatter read and
         write), 4 + position + 20 for the sorted copies (+ 4 for the caller index of a re-ordered state), 16 + 32 * (4 / 3) / 8
         for the boxes;
  query: per query 20 bytes per evaluation (an upper bound: a leaf's bodies are loaded once per wavefront, through the scalar
         unit) and 16 k + 4 of results.
Prints one JSON line per k and one for the count.  Development aid, not a bench."""
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
pos_bytes = 8 if prec == G.Precision.F32 else 16
reordered = not a.no_reorder and prec != G.Precision.F64
build_bytes = a.n * (2 * pos_bytes + 8 + 4 * 24 + 4 + pos_bytes + 20 + (4 if reordered else 0) + 16 + 32 * 4 // 3 // 8)
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                  reference_compat=prec == G.Precision.F64)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    if not a.no_reorder:
        e.step(5 + 16)
    common = {"precision": prec.name, "kind": a.kind, "n": a.n, "reordered": reordered, "repeats": a.repeats}
    for k in a.ks:
        e.neighbours(k)
        build, query, call = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            idx, d2, ev = e.neighbours(k, with_evals=True)
            call.append((time.perf_counter() - t0) * 1e3)
            b, q = e.neighbours_times()
            build.append(b)
            query.append(q)
        print(json.dumps({**common, "query": "neighbours", "k": k, "build_ms [median, min, max]": row(build),
                          "query_ms [median, min, max]": row(query), "call_ms [median, min, max]": row(call),
                          "evals_mean": round(float(ev.mean()), 2), "evals_max": int(ev.max()),
                          "build_bytes": build_bytes, "query_bytes": int(20 * int(ev.sum(dtype=np.uint64)) + a.n * (16 * k + 4)),
                          "median_r_k": float(np.sqrt(np.median(d2[:, k - 1])))}), flush=True)
        del idx, d2, ev
    # the radius that encloses about 8 bodies on average (the mean count grows with the radius)
    lo, hi = 0.0, float(np.abs(e.download()[0]).max())
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        mean = float(e.count_within(mid).mean())
        if 7.5 <= mean <= 8.5:
            break
        lo, hi = (mid, hi) if mean < 8.0 else (lo, mid)
    build, query, call = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        cnt = e.count_within(mid)
        call.append((time.perf_counter() - t0) * 1e3)
        b, q = e.neighbours_times()
        build.append(b)
        query.append(q)
    print(json.dumps({**common, "query": "count_within", "radius": mid, "count_mean": round(float(cnt.mean()), 3),
                      "count_max": int(cnt.max()), "build_ms [median, min, max]": row(build),
                      "query_ms [median, min, max]": row(query), "call_ms [median, min, max]": row(call),
                      "build_bytes": build_bytes}), flush=True)
