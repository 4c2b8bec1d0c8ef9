"""What the bucket sort's placement test costs and gains against the number of bodies under way: the step time
of N bodies of which k travel across the cloud, adaptive direct input, with placement (BH_SORT_PLACE=1) against without (=0) --
the byte passes for every bucket, the parent's path.  One process, one set of bodies, `--reps` timings of `--steps` steps per point,
alternating, so that the two columns share whatever the process and the machine add.  Development aid, not a bench."""
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
ap.add_argument("--ks", default="0,128,512,1024,2048,4096,8192,16384,32768,65536,131072")
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

m, p, v0 = IC.make("plummer", a.n, 1, quasi_static=True)
rng = np.random.default_rng(3)
f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def timed(mode, v):
    os.environ["BH_SORT_PLACE"] = mode                      # (read when the context is created)
    out = []
    with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, max_depth=21, precision=G.Precision.F32,
                                      reference_compat=False)) as e:
        e.upload(p, v, m)
        e.step(5)
        e.sync()
        t0 = time.perf_counter()
        e.step(a.steps)
        e.sync()
        out.append((time.perf_counter() - t0) / a.steps * 1e3)
        st = e.stats()
    return out[0], st.keys_ms, st.sort_ms, st.sort_spill_buckets


for k in [int(x) for x in a.ks.split(",")]:
    v = v0.copy()
    if k:
        who = rng.choice(a.n, k, replace=False)
        # towards the place of another body, a 400th of the way per step: inside the cloud for the whole run
        v[who] = f32((p[rng.permutation(who)] - p[who]) / 400.0)
    modes = ["0", "1"]
    res = {mode: [] for mode in modes}
    last = {}
    for _ in range(a.reps):
        for mode in modes:
            ms, keys_ms, sort_ms, spills = timed(mode, v)
            res[mode].append(ms)
            last[mode] = (keys_ms, sort_ms, spills)
    name = {"0": "passes", "1": "placement"}
    out = {"n": a.n, "movers": k}
    for mode in modes:
        out[name[mode] + "_ms_per_step"] = [round(x, 4) for x in res[mode]]
        out[name[mode] + "_keys_sort_ms_last_step"] = [round(x, 4) for x in last[mode][:2]]
        out[name[mode] + "_spills"] = last[mode][2]
    print(json.dumps(out), flush=True)
