"""Cost of BarnesHutEngine.field on the benchmark's state (Plummer, N = 1,048,576, theta 0.5, max_depth 21, after the
benchmark's warm-up steps), per precision, for three sets of as many points as there are bodies:

    grid      a 1,024 x 1,024 cell-centred grid over the bounding box, row-major
    shuffled  the same points in random order
    bodies    the bodies' own positions (caller order)

and, beside them, the potential() call of the same state: it walks one point per body over a near-identical term set.
A call is timed with HIP events on the engine's stream (after one warm-up call; median, min and max of --reps calls): it
holds the quiet tree build, the upload of the points, key + sort, the walk and the download of the results.  The split
into kernels comes from a separate run under the profiler's kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/field_timing.py --reps 3 --precisions f32

where field_keys_kernel and the radix_* rows are key + sort, field_f32_kernel / field_f64_kernel the walk, and
potential_f32_kernel / potential_f64_kernel the yardstick.  Prints one table and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.project import field_grid_points  # noqa: E402

PRECISIONS = {"f32": G.Precision.F32, "mixed": G.Precision.MIXED, "f64": G.Precision.F64, "exact": G.Precision.F64_EXACT}


class Hip:
    """The few HIP runtime calls of an event timer."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p()
        self.check(self.lib.hipStreamCreate(C.byref(self.stream)))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            self.check(self.lib.hipEventCreate(C.byref(e)))

    @staticmethod
    def check(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def timed(self, fn) -> float:
        self.check(self.lib.hipEventRecord(self.ev[0], self.stream))
        fn()
        self.check(self.lib.hipEventRecord(self.ev[1], self.stream))
        self.check(self.lib.hipEventSynchronize(self.ev[1]))
        ms = C.c_float()
        self.check(self.lib.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]))
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-bodies", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precisions", default="f32,mixed,f64,exact")
    a = ap.parse_args()
    hip = Hip()
    n = a.n_bodies
    m, p, v = IC.make("plummer", n, a.seed, quasi_static=True)
    rows = []
    for name in a.precisions.split(","):
        # (the benchmark's contexts: reference_compat off in F32 / MIXED, on in the fp64 precisions)
        cfg = G.BhConfig(capacity=n, theta=0.5, max_depth=21, precision=PRECISIONS[name], reference_compat=name in ("f64", "exact"))
        with G.BarnesHutEngine(cfg) as e:
            e.set_stream(hip.stream.value)
            e.upload(p, v, m)
            e.step(a.warmup_steps)
            pos = e.download()[0]
            grid = field_grid_points((a.grid, a.grid), None, pos)
            sets = {"grid": grid, "shuffled": grid[np.random.default_rng(0).permutation(len(grid))], "bodies": pos}
            sets["potential()"] = None
            for label, pts in sets.items():
                call = (lambda: e.potential()) if pts is None else (lambda: e.field(pts))
                call()
                t = [hip.timed(call) for _ in range(a.reps)]
                rows.append({"precision": name, "set": label, "points": n if pts is None else len(pts),
                             "call_ms_median": statistics.median(t), "call_ms_min": min(t), "call_ms_max": max(t)})
                print("%-6s %-12s %9d points  call %8.3f ms (min %8.3f, max %8.3f)"
                      % (name, label, rows[-1]["points"], rows[-1]["call_ms_median"], min(t), max(t)), flush=True)
    print(json.dumps({"workload": f"plummer_N{n}_theta0.5_depth21", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
