"""What the minimum spanning tree costs: the index's build, the Boruvka rounds and the final sort of bh_spanning_tree, beside
bh_groups -- one traversal of the same index, the natural yardstick for a round -- and the subset kernel of
bh_spanning_tree_subsets.

    python scripts/spanning_tree_timing.py [--n 65536 1048576] [--repeats 5] [--precision F32] [--kind plummer] [--subsets 20 100 512]

One context per size on the quasi-static Plummer state of scripts/neighbours_timing.py (scale radius 0.02, max_depth 21), 5 + 16
untimed steps, so that the fp32 state has been physically re-ordered as in a run.  After one untimed call, `repeats` calls of
spanning_tree(with_stats=True); the times are the library's own (bh_spanning_tree_times):
  build:   bounds pass (and the host's look at it), keys, the four sort passes, the sorted copies, the boxes (HIP events);
  rounds:  every round's node components, nearest, pick, hook and flatten kernels and its 8-byte read-back (HIP events);
  sort:    the eight radix passes over the n - 1 edges' d2 and the gather of their pairs (HIP events), and the host's ordering of
           edges of equal d2 (host clock);
  call:    the host clock from the call to its return, downloads included.
Then `repeats` calls of groups(b, 1) at b = the median edge length of the tree (bh_groups_times: link).  Then, per k of
--subsets, 500 random sets of k bodies: the kernel (HIP events) and the call (host clock).  A row is the median over the repeats
with their minimum and maximum.  Prints one JSON line per size and one per k.  Development aid, not a bench (DESIGN.md section
25)."""
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
ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--kind", choices=["plummer", "uniform"], default="plummer")
ap.add_argument("--subsets", type=int, nargs="*", default=[20, 100, 512])
ap.add_argument("--sets", type=int, default=500)
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
        common = {"precision": prec.name, "kind": a.kind, "n": n, "repeats": a.repeats}
        e.spanning_tree()
        build, rounds, sort, call, stats = [], [], [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            t = e.spanning_tree(with_stats=True)
            call.append((time.perf_counter() - t0) * 1e3)
            ms = e.spanning_tree_times()
            build.append(ms[0]); rounds.append(ms[1]); sort.append(ms[2]); stats.append(t.stats)
        b = float(np.median(t.length))
        e.groups(b, 1)
        link = []
        for _ in range(a.repeats):
            g = e.groups(b, 1, with_stats=True)
            link.append(e.groups_times()[1])
        nr = t.stats[0]
        print(json.dumps({**common, "build_ms [median, min, max]": row(build), "rounds_ms [median, min, max]": row(rounds),
                          "sort_ms [median, min, max]": row(sort), "call_ms [median, min, max]": row(call), "rounds": nr,
                          "ms_per_round": round(float(np.median(rounds)) / max(nr, 1), 4),
                          "stats [rounds, distances, skipped nodes, edges] of every repeat": [list(s) for s in stats],
                          "distances_per_body_per_round": round(t.stats[1] / n / max(nr, 1), 2),
                          "median_edge": b, "groups_at_median_edge": g.n_groups, "groups_link_ms [median, min, max]": row(link),
                          "groups_stats [distances, pairs, hooks]": list(g.stats)}), flush=True)
        rng = np.random.default_rng(2)
        for k in a.subsets:
            members = np.stack([rng.choice(n, k, replace=False) for _ in range(a.sets)])
            e.subset_spanning_trees(members)
            kern, srt, call = [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                e.subset_spanning_trees(members)
                call.append((time.perf_counter() - t0) * 1e3)
                ms = e.spanning_tree_times()
                kern.append(ms[1]); srt.append(ms[2])
            print(json.dumps({**common, "subsets": a.sets, "k": k, "kernel_ms [median, min, max]": row(kern),
                              "row_sort_ms [median, min, max]": row(srt), "call_ms [median, min, max]": row(call)}), flush=True)
