"""What a moment map costs: both passes of bh_moment_map_deposit by HIP events, and bh_moment_map with its download.

    python scripts/moment_map_timing.py [--n 1048576] [--repeats 7] [--grids 512 4096] [--precision F32] [--skip-map]

One context on the quasi-static Plummer state of scripts/split_timing.py (scale radius 0.02, max_depth 21, bucket leaves),
5 untimed steps and, unless --no-reorder, enough further steps for a physical re-order, so that the state lies in curve order
as in a run.  The box is the central square that holds the innermost 90 % of the bodies per axis.  Per grid (G x G cells) and
scheme, after one untimed call:
  deposit: moment_map_deposit -- the maxima pass, the host's look at them, the memset of the grid and the deposit pass; the grid
           stays on the device -- between two events on the engine's stream (torch's current stream), `repeats` times;
  map:     moment_map with raw=True -- the same plus the download of the 4 planes and the conversion to fp64 maps on the host --
           on the host clock from the call to its return.
A row is the median over the repeats with their minimum and maximum.  roofline = the algorithmic bytes (the state read once,
the four int64 planes written once) / the deposit's median / 8 TB/s.  Prints one JSON line per grid and scheme.  Development
aid, not a bench."""
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
from gpu_nbody_simulation_amd.engine import moment_exponents  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--grids", type=int, nargs="+", default=[512, 4096])
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--skip-map", action="store_true", help="time the deposit only")
ap.add_argument("--no-reorder", action="store_true", help="map the state in upload order (no steps at all)")
a = ap.parse_args()

PEAK = 8e12          # bytes per second


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 5), round(float(x.min()), 5), round(float(x.max()), 5)]


prec = G.Precision[a.precision]
m, p, v = IC.make("plummer", a.n, 1, quasi_static=True)
state_bytes = a.n * (20 if prec == G.Precision.F32 else 40)
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                  reference_compat=prec == G.Precision.F64)) as e:
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.upload(p, v, m)
    if not a.no_reorder:
        e.step(5 + 16)
    pos, _ = e.download()
    lo, hi = np.quantile(pos, 0.05, axis=0), np.quantile(pos, 0.95, axis=0)
    box = (lo[0], hi[0], lo[1], hi[1])
    ex = moment_exponents(e.moment_map_max(), a.n)
    for g in a.grids:
        for scheme in ("ngp", "cic"):
            _, n_dep = e.moment_map_deposit(box, g, g, scheme, ex)
            dep, full = [], []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                e.moment_map_deposit(box, g, g, scheme, ex)
                e1.record()
                e1.synchronize()
                dep.append(e0.elapsed_time(e1))
            for _ in range(0 if a.skip_map else a.repeats):
                t0 = time.perf_counter()
                mm = e.moment_map(box, g, g, scheme, raw=True)
                full.append((time.perf_counter() - t0) * 1e3)
            if a.skip_map:
                mm = e.moment_map(box, g, g, scheme)
            algo = state_bytes + 4 * 8 * g * g
            print(json.dumps({"precision": prec.name, "n": a.n, "grid": [g, g], "scheme": scheme, "n_deposited": n_dep,
                              "reordered": not a.no_reorder, "repeats": a.repeats,
                              "deposit_ms [median, min, max]": row(dep), **({} if a.skip_map else {"map_ms [median, min, max]": row(full)}),
                              "algorithmic_bytes": algo, "roofline_fraction": round(algo / (np.median(dep) * 1e-3) / PEAK, 4),
                              "mass_inside": float(mm.mass.sum())}), flush=True)
            del mm
