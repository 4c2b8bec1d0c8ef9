"""What the split operators and the leapfrog cost: kick and drift passes, step_kdk(K) per step against step(K).

    python scripts/split_timing.py [--n 1048576] [--repeats 7] [--steps 100] [--passes 20]

Per precision (F32, F64) one context on the quasi-static Plummer state of scripts/soft_walk_ab.py (scale radius 0.02, theta
0.5, max_depth 21; F32 with bucket leaves, F64 with the reference's depth-cap rules), 5 untimed steps, then per repeat:
  step(K) and step_kdk(K), alternating which goes first, each timed on the host from the call to the end of sync(), per step;
  `passes` kick(+h) / kick(-h) pairs and as many drift(+h) / drift(-h) pairs (the state returns to where it was up to
  rounding), each batch timed from the first call to the end of sync(), per pass: launch overhead included, the figure of a
  caller who enqueues them back to back.
A row is the median over the repeats with their minimum and maximum.  On a build without the operators (the parent commit)
only step(K) is measured.  Prints one JSON line per precision.  Development aid, not a bench."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--passes", type=int, default=20)
a = ap.parse_args()


def timed(e, call, per):
    e.sync()
    t0 = time.perf_counter()
    call()
    e.sync()
    return (time.perf_counter() - t0) * 1e3 / per


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 5), round(float(x.min()), 5), round(float(x.max()), 5)]


m, p, v = IC.make("plummer", a.n, 1, quasi_static=True)
for prec in (G.Precision.F32, G.Precision.F64):
    with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=prec,
                                      reference_compat=prec == G.Precision.F64)) as e:
        split = hasattr(e, "step_kdk")
        h = 1e-3 * e.cfg.dt
        e.upload(p, v, m)
        e.step(5)
        out = {"step": [], "step_kdk": [], "kick": [], "drift": []}

        def kicks():
            for _ in range(a.passes):
                e.kick(h)
                e.kick(-h)

        def drifts():
            for _ in range(a.passes):
                e.drift(h)
                e.drift(-h)

        for rep in range(a.repeats):
            for which in (("step", "step_kdk") if rep % 2 == 0 else ("step_kdk", "step")):
                if which == "step":
                    out["step"].append(timed(e, lambda: e.step(a.steps), a.steps))
                elif split:
                    out["step_kdk"].append(timed(e, lambda: e.step_kdk(a.steps), a.steps))
            if split:
                e.compute_forces()
                out["kick"].append(timed(e, kicks, 2 * a.passes))
                out["drift"].append(timed(e, drifts, 2 * a.passes))
        finite = bool(np.isfinite(e.download()[0]).all())
    print(json.dumps({"precision": prec.name, "n": a.n, "repeats": a.repeats, "steps": a.steps, "finite": finite,
                      **{k + "_ms [median, min, max]": row(x) for k, x in out.items() if x}}), flush=True)
