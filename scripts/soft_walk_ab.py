"""What Plummer softening costs the walks: walk_ms and step_ms per step at eps = 0 and eps > 0 on one build, interleaved.

    python scripts/soft_walk_ab.py [--n 1048576] [--eps-over-a 1e-3] [--repeats 5] [--steps 30]

Per precision (F32, F64) and repeat, a fresh context per eps on the same quasi-static Plummer state (scale radius a = 0.02,
theta 0.5, max_depth 21; F32 with bucket leaves as scripts/run_steps.py runs it, F64 with the reference's depth-cap rules as
tests/test_gpu_f64.py's full-size case -- without them the unsoftened fp64 walk meets a body ON an aggregate, the reference's
0 * inf, and the eps = 0 row would time a run of NaNs), `warmup` untimed steps, then `steps` steps timed with the engine's
own events (bh_step_times).  A repeat's figure is the median over its steps; a row is the median over the repeats with their
minimum and maximum -- the run-to-run spread the difference has to be read against; "finite" says that every position was
finite at the end.  The order eps = 0 / eps > 0 alternates between repeats.
Prints one JSON line per (precision, eps).  Development aid, not a bench (DESIGN.md section 16 quotes its table)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--eps-over-a", type=float, default=1e-3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

PLUMMER_A = 0.02
m, p, v = IC.make("plummer", a.n, 1, quasi_static=True)
for prec in (G.Precision.F32, G.Precision.F64):
    rows = {}
    for rep in range(a.repeats):
        order = (0.0, a.eps_over_a * PLUMMER_A) if rep % 2 == 0 else (a.eps_over_a * PLUMMER_A, 0.0)
        for eps in order:
            with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                              reference_compat=prec == G.Precision.F64, softening=eps)) as e:
                e.upload(p, v, m)
                e.step(a.warmup)
                e.step(a.steps)
                e.sync()
                st, wk = e.step_times()
                finite = bool(np.isfinite(e.download()[0]).all())
            rows.setdefault(eps, []).append((float(np.median(wk)), float(np.median(st)), float(finite)))
    for eps, r in sorted(rows.items()):
        wk, st, fin = np.array(r).T
        print(json.dumps({"precision": prec.name, "n": a.n, "eps": eps, "repeats": a.repeats, "steps": a.steps, "finite": bool(fin.all()),
                          "walk_ms": round(float(np.median(wk)), 4), "walk_ms_min": round(float(wk.min()), 4),
                          "walk_ms_max": round(float(wk.max()), 4), "step_ms": round(float(np.median(st)), 4),
                          "step_ms_min": round(float(st.min()), 4), "step_ms_max": round(float(st.max()), 4)}), flush=True)
