"""What the azimuthal modes cost, beside a radial profile of the same state in the same process.

    python scripts/modes_timing.py [--n 1048576] [--repeats 7] [--precision F32] [--blocks 256 512 1024 2048]

One context on the quasi-static Plummer state of scripts/radial_timing.py (scale radius 0.02, max_depth 21, bucket leaves),
5 + 16 untimed steps so that the state lies in curve order as in a run.  The centre is the centre of mass; the edges are log
spaced from a thousandth of the radius that holds every body.  After one untimed call each, `repeats` times:
  modes:   azimuthal_modes(raw=True) on the host clock from the call to its return, and bh_modes_times' HIP-event times of its
           two passes, for (M, rates, bins) = (2, no, 64), (4, yes, 64), (16, yes, 64) -- private histograms -- and (4, yes, 4096),
           whose 19 planes leave a tile of 431 slots: workgroups whose bodies span more go to memory directly;
  profile: radial_profile(raw=True) with 64 bins likewise, the yardstick.
A row is the median over the repeats with their minimum and maximum.  --blocks: the modes again in a fresh context per value of
BH_RADIAL_BLOCKS (the state in upload order).  Prints one JSON line per measurement.  Development aid, not a bench (DESIGN.md
section 30)."""
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
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
ap.add_argument("--blocks", type=int, nargs="*", default=[])
a = ap.parse_args()
CASES = [(2, False, 64), (4, True, 64), (16, True, 64), (4, True, 4096)]


def row(x):
    x = np.asarray(x, dtype=np.float64)
    return [round(float(np.median(x)), 5), round(float(x.min()), 5), round(float(x.max()), 5)]


def config(prec):
    return G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec, reference_compat=prec == G.Precision.F64)


def measure(e, centre, r_max, what, with_profile):
    for M, rates, nb in CASES:
        edges = G.radial_edges(1e-3 * r_max, r_max, nb)
        e.azimuthal_modes(edges, M, centre, rates=rates)
        full, first, second = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            md = e.azimuthal_modes(edges, M, centre, rates=rates, raw=True)
            full.append((time.perf_counter() - t0) * 1e3)
            t = e.modes_times()
            first.append(t[0]); second.append(t[1])
        print(json.dumps({**what, "m_max": M, "rates": rates, "bins": nb, "planes": G.modes_planes(M, rates),
                          "call_ms [median, min, max]": row(full), "max_pass_ms": row(first), "deposit_pass_ms": row(second),
                          "bodies_in_bins": int(md.count.sum()), "bar_strength": md.total(min(2, M)).amplitude}), flush=True)
    if with_profile:
        edges = G.radial_edges(1e-3 * r_max, r_max, 64)
        e.radial_profile(edges, centre)
        full, first, second = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            e.radial_profile(edges, centre, raw=True)
            full.append((time.perf_counter() - t0) * 1e3)
            t = e.radial_times()
            first.append(t[0]); second.append(t[1])
        print(json.dumps({**what, "radial_profile_bins": 64, "call_ms [median, min, max]": row(full), "max_pass_ms": row(first),
                          "deposit_pass_ms": row(second)}), flush=True)


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
    measure(e, centre, r_max, {"precision": prec.name, "n": a.n, "blocks": "default", "repeats": a.repeats}, True)
for b in a.blocks:
    os.environ["BH_RADIAL_BLOCKS"] = str(b)
    with G.BarnesHutEngine(config(prec)) as e:
        e.upload(p, v, m)
        measure(e, centre, r_max, {"precision": prec.name, "n": a.n, "blocks": b, "repeats": a.repeats}, False)
