"""What a radial profile and the Lagrangian radii cost, beside a moment map of the same state in the same process.

    python scripts/radial_timing.py [--n 1048576] [--repeats 7] [--bins 64 4096] [--precision F32] [--blocks 256 512 1024 2048]

One context on the quasi-static Plummer state of scripts/moment_map_timing.py (scale radius 0.02, max_depth 21, bucket leaves),
5 + 16 untimed steps so that the state lies in curve order as in a run.  The centre is the centre of mass; the edges are log
spaced from a thousandth of the radius that holds every body.  After one untimed call each, `repeats` times:
  profile:    radial_profile(raw=True) on the host clock from the call to its return, and bh_radial_times' HIP-event times
              of its two passes;
  radii:      lagrangian_radii of four fractions on the host clock, the first pass and the eight rounds by HIP events;
  moment_map: moment_map("ngp", 64 x 64) over the box of the same radius, on the host clock -- it reads the same bytes.
A row is the median over the repeats with their minimum and maximum.  --blocks: the profile's deposit pass and the select rounds
again in a fresh context per value of BH_RADIAL_BLOCKS (the state in upload order).  Prints one JSON line per measurement.
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
ap.add_argument("--bins", type=int, nargs="+", default=[64, 4096])
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--blocks", type=int, nargs="*", default=[])
a = ap.parse_args()
FRACTIONS = (0.01, 0.1, 0.5, 0.9)


def row(x):
    x = np.asarray(x, dtype=np.float64)
    return [round(float(np.median(x)), 5), round(float(x.min()), 5), round(float(x.max()), 5)]


def config(prec):
    return G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec, reference_compat=prec == G.Precision.F64)


def measure(e, centre, r_max, bins, what, with_map):
    for nb in bins:
        edges = G.radial_edges(1e-3 * r_max, r_max, nb)
        e.radial_profile(edges, centre)
        full, first, second = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            pr = e.radial_profile(edges, centre, raw=True)
            full.append((time.perf_counter() - t0) * 1e3)
            t = e.radial_times()
            first.append(t[0]); second.append(t[1])
        print(json.dumps({**what, "profile_bins": nb, "call_ms [median, min, max]": row(full), "max_pass_ms": row(first),
                          "deposit_pass_ms": row(second), "bodies_in_bins": int(pr.count.sum())}), flush=True)
    e.lagrangian_radii(FRACTIONS, centre)
    full, first, rounds = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        lr = e.lagrangian_radii(FRACTIONS, centre)
        full.append((time.perf_counter() - t0) * 1e3)
        t = e.radial_times()
        first.append(t[0]); rounds.append(t[2])
    rounds = np.array(rounds)
    print(json.dumps({**what, "fractions": list(FRACTIONS), "call_ms [median, min, max]": row(full), "max_pass_ms": row(first),
                      "round_ms": [row(rounds[:, k]) for k in range(8)], "rounds_ms": row(rounds.sum(axis=1)),
                      "r": [float(x) for x in lr.r]}), flush=True)
    if with_map:
        box = (centre[0] - r_max, centre[0] + r_max, centre[1] - r_max, centre[1] + r_max)
        e.moment_map(box, 64, 64, "ngp")
        full = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            mm = e.moment_map(box, 64, 64, "ngp", raw=True)
            full.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({**what, "moment_map": "ngp 64 x 64", "call_ms [median, min, max]": row(full), "n_deposited": mm.n_deposited}),
              flush=True)


prec = G.Precision[a.precision]
m, p, v = IC.make("plummer", a.n, 1, quasi_static=True)
os.environ.pop("BH_RADIAL_BLOCKS", None)
with G.BarnesHutEngine(config(prec)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    e.step(5 + 16)
    centre = np.array(e.energy().com)
    pos, _ = e.download()
    r_max = float(np.nextafter(np.sqrt(((pos - centre) ** 2).sum(axis=1).max()), np.inf))
    measure(e, centre, r_max, a.bins, {"precision": prec.name, "n": a.n, "blocks": "default", "repeats": a.repeats}, True)
for b in a.blocks:
    os.environ["BH_RADIAL_BLOCKS"] = str(b)
    with G.BarnesHutEngine(config(prec)) as e:
        e.upload(p, v, m)
        measure(e, centre, r_max, a.bins, {"precision": prec.name, "n": a.n, "blocks": b, "repeats": a.repeats}, False)
