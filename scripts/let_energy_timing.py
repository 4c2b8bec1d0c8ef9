"""Cost of the distributed diagnostics, rehearsed on ONE GPU (tests/let_energy_ranks.py: W contexts stand in for W ranks,
the collectives are device copies):

  per rank, HIP events on the engine's stream, median of --reps after a warm-up:
    force    : the forest force walk of the rank (bh_let_forces), in the shape the engine picks for the rank's size
    one wave : the same walk with BH_FLAG_WALK_NO_SPLIT -- one wavefront per 64 bodies, tree after tree, the shape and tree
               order of the potential walk (hand-scheduled loop, two quads in flight)
    potential: the forest potential walk of the same forest (bh_let_potential: the kernel and its 64-byte counter read-back)
    sums     : bh_let_energy with the potential current (the two reduction launches and the 64-byte read-back)
  and the wall time of one whole energy() of the emulated run: quiet bounds + build + block copies + walk + reductions of
  all W ranks one after the other, every host synchronisation included.

  python scripts/let_energy_timing.py [--n 1048576] [--world 8] [--init plummer] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_WALK_NO_SPLIT  # noqa: E402
from let_energy_ranks import EnergyRanks  # noqa: E402


def timed(fn, reps):
    """Median milliseconds between two events on the current stream around fn(), after one warm-up call."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--init", default="plummer")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", choices=["f32", "mixed"], default="f32")
    a = ap.parse_args()
    m, p, v = IC.make(a.init, a.n, 1, quasi_static=True)
    cfg = dict(theta=0.5, max_depth=21, reference_compat=False,
               precision=G.Precision.MIXED if a.precision == "mixed" else G.Precision.F32)
    er = EnergyRanks(m, p, v, a.world, None, flags=FLAG_WALK_NO_SPLIT, **cfg)
    try:
        er.step(integrate=False)
        one_wave = [timed(e.let_forces, a.reps) for e in er.engs]
    finally:
        er.close()
    er = EnergyRanks(m, p, v, a.world, None, **cfg)
    rows = []
    try:
        er.step(integrate=False)                                # the forest of the state, on every rank
        for r, e in enumerate(er.engs):
            force = timed(e.let_forces, a.reps)
            pot = timed(lambda: e._check(e._lib.bh_let_potential(e._h)), a.reps)
            sums = timed(e.let_energy_sums, a.reps)
            rows.append({"rank": r, "bodies": e.n, "force_ms": force, "force_one_wave_ms": one_wave[r], "potential_ms": pot,
                         "sums_ms": sums})
            print(f"rank {r}: {e.n:8d} bodies  force walk {force:.3f} ms (one wave per group {one_wave[r]:.3f})  "
                  f"potential walk {pot:.3f} ms ({pot / force:.2f} x)  reductions {sums:.3f} ms", flush=True)
        er.energy()
        wall = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            er.energy()
            wall.append((time.perf_counter() - t0) * 1e3)
        whole = statistics.median(wall)
        print(f"energy() of the emulated run ({a.world} ranks one after the other): {whole:.2f} ms wall")
    finally:
        er.close()
    print(json.dumps({"n": a.n, "world": a.world, "init": a.init, "precision": a.precision, "ranks": rows,
                      "energy_wall_ms": whole}))


if __name__ == "__main__":
    main()
