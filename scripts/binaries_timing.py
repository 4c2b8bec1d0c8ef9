"""What the bound-pair search costs: the index's build with the sorted velocities, masses and mass bounds, the partner search and
the catalogue of bh_binaries, beside bh_count_within at the same radius in the same process -- the same traversal of the same
index without energies, the natural yardstick for the search.

    python scripts/binaries_timing.py [--n 1048576] [--repeats 7] [--precision F32] [--kind plummer]

One context per size on the quasi-static Plummer state of scripts/neighbours_timing.py (scale radius 0.02, max_depth 21), 5 + 16
untimed steps, so that the fp32 state has been physically re-ordered as in a run.  max_separation is the median distance of the
6th neighbour (one neighbours(6) call).  After one untimed call, `repeats` calls of binaries(R, with_stats=True); the times are the
library's own (bh_binaries_times):
  build:      bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes; then the sorted
              velocities and masses and the levels of mass bounds (HIP events);
  search:     the partner search (HIP events);
  catalogue:  the mutual pairs and their elements (HIP events), and the host's ordering of the records by lo (host clock);
  call:       the host clock from the call to its return, downloads included.
Then `repeats` calls of count_within(R) (bh_neighbours_times: build, query).  A row is the median over the repeats with their
minimum and maximum; search_over_count is the ratio of the two medians.  Prints one JSON line per size.  Development aid, not a
bench."""
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
ap.add_argument("--n", type=int, nargs="+", default=[1 << 20])
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--kind", choices=["plummer", "uniform"], default="plummer")
a = ap.parse_args()


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 4), round(float(x.min()), 4), round(float(x.max()), 4)]


prec = G.Precision[a.precision]
for n in a.n:
    m, p, v = IC.make(a.kind, n, 1, quasi_static=True)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, theta=0.5, max_depth=21, precision=prec,
                                      reference_compat=prec == G.Precision.F64)) as e:
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.upload(p, v, m)
        e.step(5 + 16)
        R = float(np.sqrt(np.median(e.neighbours(6)[1][:, 5])))
        e.binaries(R)
        build, search, cat, call, stats = [], [], [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            b = e.binaries(R, with_stats=True)
            call.append((time.perf_counter() - t0) * 1e3)
            ms = e.binaries_times()
            build.append(ms[0]); search.append(ms[1]); cat.append(ms[2]); stats.append(b.stats)
        e.count_within(R)
        cbuild, count = [], []
        for _ in range(a.repeats):
            c = e.count_within(R)
            ms = e.neighbours_times()
            cbuild.append(ms[0]); count.append(ms[1])
        print(json.dumps({"precision": prec.name, "kind": a.kind, "n": n, "repeats": a.repeats, "max_separation": R,
                          "build_ms [median, min, max]": row(build), "search_ms [median, min, max]": row(search),
                          "catalogue_ms [median, min, max]": row(cat), "call_ms [median, min, max]": row(call),
                          "stats [energies, most by one body, nodes opened, pairs] of every repeat": [list(s) for s in stats],
                          "energies_per_body": round(b.stats[0] / n, 2), "nodes_opened_per_body": round(b.stats[2] / n, 2),
                          "bodies_with_a_partner": int((b.partner >= 0).sum()), "pairs": len(b.lo),
                          "count_within_mean": round(float(c.mean()), 2),
                          "count_within_build_ms [median, min, max]": row(cbuild),
                          "count_within_query_ms [median, min, max]": row(count),
                          "search_over_count": round(float(np.median(search)) / float(np.median(count)), 3)}), flush=True)
