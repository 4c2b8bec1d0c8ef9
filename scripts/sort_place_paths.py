"""How the bucket sort's buckets end, build by build: K single steps of one workload on cuda:0, after each
the rise of the two counters of BarnesHutEngine.sort_paths -- buckets finished by placement, buckets that went through the byte
passes -- and, with --why, the rule that refused each of the latter according to the numpy twin (tests/sort_place_ref.py) on the
keys the device formed.  Development aid, not a bench."""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--init", default="plummer")
ap.add_argument("--drift", type=float, default=0.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--why", action="store_true", help="ask the twin which rule refused the buckets that took the passes (slow: a snapshot per build)")
a = ap.parse_args()
if a.why:
    import sort_direct_ref as R
    import sort_place_ref as P
m, p, v = IC.make(a.init, a.n, 1, quasi_static=True, drift_cells=a.drift)
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=a.theta, max_depth=21, precision=G.Precision.F32,
                                  reference_compat=False)) as e:
    e.upload(p, v, m)
    e.step(a.warmup)
    last = e.sort_paths()
    for k in range(a.steps):
        e.step(1)
        now = e.sort_paths()
        line = {"build": a.warmup + k, "placed": now[0] - last[0], "passed": now[1] - last[1]}
        last = now
        if a.why:
            # (a build of its own at the positions the step left: the keys the next step's build will form)
            e.build_tree()
            s = e.sort_snapshot()
            last = e.sort_paths()
            line.update(offered=bool(s.offered), probe_placed=last[0] - now[0], probe_passed=last[1] - now[1])
            if s.offered and not s.counting:
                tw = R.direct_sort_fast(s.keys_in, s.nb, s.cap, s.subcap, s.nsub)
                placed, passed, why = P.paths(P.bucket_inputs(s.keys_in, tw))
                line.update(crossers=int(tw.k), twin_placed=placed, twin_passed=passed, refused_by=dict(collections.Counter(why.values())))
            elif s.offered:
                line["counting"] = True
        print(json.dumps(line))
