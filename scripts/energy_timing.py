"""Cost of the diagnostics against the step they observe: per precision and size, HIP events on the context's stream
(the engine is put on torch's current stream) around bh_compute_potential (tree build + potential walk) and around the
reductions of bh_energy (potential current), next to the same run's step build_ms / walk_ms (bh_stats).  Plummer
sphere, quasi-static masses, theta 0.5, default max_depth.  One JSON line per (precision, n).

    python scripts/energy_timing.py [n ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [65536, 1 << 20]
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    for n in sizes:
        m, p, v = IC.make("plummer", n, 1, quasi_static=True)
        for prec in G.Precision:
            with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec)) as e:
                e.set_stream(stream)
                e.upload(p, v, m)
                e.step(3)
                e.sync()
                reps = 5 if n > 200000 else 20
                step_ms = timed(lambda: e.step(1), reps)
                st = e.stats()
                pot_ms = timed(lambda: e._check(e._lib.bh_compute_potential(e._h)), reps)
                red_ms = timed(lambda: e.energy(), reps)
                print(json.dumps({"n": n, "precision": prec.name, "step_ms": round(step_ms, 4),
                                  "build_ms": round(st.build_ms, 4), "walk_ms": round(st.walk_ms, 4),
                                  "potential_ms": round(pot_ms, 4), "potential_walk_ms": round(pot_ms - st.build_ms, 4),
                                  "reduction_ms": round(red_ms, 4),
                                  "walk_ratio": round((pot_ms - st.build_ms) / st.walk_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
