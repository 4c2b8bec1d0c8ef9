"""What friends-of-friends groups cost: the index's build, the linking and the catalogue of bh_groups by HIP events, beside
bh_count_within -- the traversal's parent -- at the same radius on the same state.

    python scripts/groups_timing.py [--n 1048576] [--repeats 7] [--friends 1 8 64] [--precision F32] [--kind plummer]

One context on the quasi-static Plummer state of scripts/neighbours_timing.py (scale radius 0.02, max_depth 21), 5 + 16 untimed
steps, so that the fp32 state has been physically re-ordered as in a run.  Per target f of --friends: the linking length b at
which count_within averages about f bodies, found by bisection; after one untimed call, `repeats` calls of groups(b, 2,
with_stats=True) and `repeats` calls of count_within(b).  The times are the library's own HIP events (bh_groups_times,
bh_neighbours_times):
  build:     bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes;
  link:      the pre-linking of the clique nodes, the link kernel, flatten and label;
  catalogue: the maxima (and the host's look at them), the numbering of the kept groups, the fixed-point sums;
  call:      the host clock from the call to its return, downloads and the ordering of the records included;
  count:     the search kernel of count_within over all bodies.
A row is the median over the repeats with their minimum and maximum.  Prints one JSON line per linking length.  Development aid,
not a bench."""
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
ap.add_argument("--friends", type=float, nargs="+", default=[1.0, 8.0, 64.0])
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--kind", choices=["plummer", "uniform"], default="plummer")
ap.add_argument("--no-reorder", action="store_true", help="link the state in upload order (no steps at all)")
a = ap.parse_args()


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 4), round(float(x.min()), 4), round(float(x.max()), 4)]


prec = G.Precision[a.precision]
m, p, v = IC.make(a.kind, a.n, 1, quasi_static=True)
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                  reference_compat=prec == G.Precision.F64)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    if not a.no_reorder:
        e.step(5 + 16)
    common = {"precision": prec.name, "kind": a.kind, "n": a.n, "reordered": not a.no_reorder and prec != G.Precision.F64,
              "repeats": a.repeats}
    extent = float(np.abs(e.download()[0]).max())
    for f in a.friends:
        # the radius that encloses about f bodies on average (the mean count grows with the radius)
        lo, hi = 0.0, extent
        for _ in range(50):
            b = 0.5 * (lo + hi)
            mean = float(e.count_within(b).mean())
            if abs(mean - f) <= f / 16:
                break
            lo, hi = (b, hi) if mean < f else (lo, b)
        count = []
        for _ in range(a.repeats):
            cnt = e.count_within(b)
            count.append(e.neighbours_times()[1])
        e.groups(b, 2)
        build, link, cat, call = [], [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            g = e.groups(b, 2, with_stats=True)
            call.append((time.perf_counter() - t0) * 1e3)
            t = e.groups_times()
            build.append(t[0]); link.append(t[1]); cat.append(t[2])
        print(json.dumps({**common, "linking_length": b, "friends_mean": round(float(cnt.mean()), 3), "friends_max": int(cnt.max()),
                          "build_ms [median, min, max]": row(build), "link_ms [median, min, max]": row(link),
                          "catalogue_ms [median, min, max]": row(cat), "call_ms [median, min, max]": row(call),
                          "count_within_query_ms [median, min, max]": row(count),
                          "stats [distances, pairs, hooks]": list(g.stats), "n_groups": g.n_groups, "records": int(len(g.id)),
                          "largest_group": int(g.count[0]) if len(g.count) else 0}), flush=True)
