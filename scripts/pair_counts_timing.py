"""What the pair counts cost: the structure's build and the traversal of bh_pair_counts by HIP events, beside the only route
there was before it: one bh_count_within per edge.

    python scripts/pair_counts_timing.py [--n 1048576] [--repeats 7] [--bins 16] [--ranges 1e-4 1e-3 1e-4 1e-1]
                                         [--precision F32] [--kind plummer] [--baseline-repeats 3]

One context on the quasi-static Plummer state of scripts/neighbours_timing.py (scale radius 0.02, max_depth 21), 5 + 16 untimed
steps, so that the fp32 state has been physically re-ordered as in a run.  Per range (RMIN RMAX, `bins` log bins), after one
untimed call, `repeats` calls of pair_counts(edges, with_evals=True) in auto mode.  The times are the library's own HIP events
(bh_pair_counts_times):
  build: bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes;
  query: the traversal kernel of every launch of 2^20 rows (the download of the nb + 2 counts excluded);
  call:  the host clock from the call to its return.
Then the baseline on the same state: count_within(edges[k]) over all bodies for every one of the bins + 1 edges,
`baseline-repeats` times; a repeat's figure is the sum over the edges of build + query of bh_neighbours_times.  The cumulative
counts of the two routes are compared.  A row is the median over the repeats with their minimum and maximum.
Prints one JSON line per range.  Development aid, not a bench."""
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
ap.add_argument("--baseline-repeats", type=int, default=3)
ap.add_argument("--bins", type=int, default=16)
ap.add_argument("--ranges", type=float, nargs="+", default=[1e-4, 1e-3, 1e-4, 1e-1], metavar="R", help="RMIN RMAX pairs")
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--kind", choices=["plummer", "uniform"], default="plummer")
a = ap.parse_args()
if len(a.ranges) % 2:
    ap.error("--ranges: RMIN RMAX pairs")


def row(x):
    x = np.asarray(x)
    if x.size == 0:
        return None
    return [round(float(np.median(x)), 4), round(float(x.min()), 4), round(float(x.max()), 4)]


prec = G.Precision[a.precision]
m, p, v = IC.make(a.kind, a.n, 1, quasi_static=True)
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                  reference_compat=prec == G.Precision.F64)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    e.step(5 + 16)
    for r_min, r_max in zip(a.ranges[::2], a.ranges[1::2]):
        edges = G.radial_edges(r_min, r_max, a.bins)
        e.pair_counts(edges)
        build, query, call = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            pc = e.pair_counts(edges, with_evals=True)
            call.append((time.perf_counter() - t0) * 1e3)
            b, q = e.pair_counts_times()
            build.append(b)
            query.append(q)
        print(f"# pair_counts {r_min:g} .. {r_max:g}: build + query {row(np.add(build, query))} ms", file=sys.stderr, flush=True)
        base, base_build, base_call, cumulative = [], [], [], None
        for _ in range(a.baseline_repeats):
            total = total_build = 0.0
            cumulative = []
            t0 = time.perf_counter()
            for edge in edges:
                cumulative.append(int(e.count_within(float(edge)).sum(dtype=np.int64)) // 2)
                b, q = e.neighbours_times()
                total += b + q
                total_build += b
            base_call.append((time.perf_counter() - t0) * 1e3)
            base.append(total)
            base_build.append(total_build)
        agree = None if cumulative is None else bool(np.array_equal(np.array(cumulative, dtype=np.int64), pc.cumulative))
        print(json.dumps({"precision": prec.name, "kind": a.kind, "n": a.n, "bins": a.bins, "r_min": r_min, "r_max": r_max,
                          "repeats": a.repeats, "build_ms [median, min, max]": row(build), "query_ms [median, min, max]": row(query),
                          "build_plus_query_ms [median, min, max]": row(np.add(build, query)),
                          "call_ms [median, min, max]": row(call), "evals": pc.evals,
                          "evals_share_of_all_pairs": pc.evals / (a.n * (a.n - 1) / 2), "evals_per_body": round(pc.evals / a.n, 1),
                          "pairs_in_bins": int(pc.counts.sum()), "baseline_repeats": a.baseline_repeats,
                          "baseline_count_within_calls": len(edges), "baseline_build_plus_query_ms [median, min, max]": row(base),
                          "baseline_build_ms [median, min, max]": row(base_build),
                          "baseline_call_ms [median, min, max]": row(base_call), "routes_agree": agree}), flush=True)
