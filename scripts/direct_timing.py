"""The two tables of DESIGN.md section 13.

1. Direct-sum call time (bh_direct_forces: target copy-in, the slot map where the state is re-ordered, the kernel, the
   copy-out; HIP events on the context's stream, median of the repetitions after one warm-up call) on a Plummer sphere:
   N = 65,536 all targets; N = 1M with 65,536 sampled targets and with all targets (once after the warm-up).
2. Barnes-Hut force error (BarnesHutEngine.force_error) against theta in {0.3, 0.5, 0.7, 1.0} in all four precisions on
   a 1M Plummer sphere, 65,536 sampled bodies (seed 0), reference_compat on, max_depth 21 (the benchmark's); and at
   theta 0.5 with the reference's default max_depth 10, where the depth-capped cells of the core dominate.

One JSON line per measurement.

    python scripts/direct_timing.py [timing|error ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.engine import sample_targets  # noqa: E402

M = 1 << 20


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                                   # (warm-up: code objects, first-use buffers)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def timing(stream):
    for n, k, reps in ((65536, 65536, 10), (M, 65536, 5), (M, M, 1)):
        m, p, v = IC.plummer(n, 1)
        t = None if k == n else sample_targets(n, k, 0)
        for prec in (G.Precision.F64, G.Precision.F32):
            with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec)) as e:
                e.set_stream(stream)
                e.upload(p, v, m)
                ms = timed(lambda: e.direct_forces(t), reps)
            print(json.dumps({"table": "direct_ms", "n": n, "targets": k, "precision": prec.name, "ms": round(ms, 3),
                              "pairs_per_s": float("%.3g" % (n * k / (ms * 1e-3)))}), flush=True)


def error():
    m, p, v = IC.plummer(M, 1)
    t = sample_targets(M, 65536, 0)
    for prec in G.Precision:
        for theta, depth in ((0.3, 21), (0.5, 21), (0.7, 21), (1.0, 21), (0.5, 10)):
            with G.BarnesHutEngine(G.BhConfig(capacity=M, precision=prec, theta=theta, max_depth=depth)) as e:
                e.upload(p, v, m)
                r = e.force_error(targets=t)
            print(json.dumps({"table": "force_error", "n": M, "sample": len(t), "precision": prec.name, "theta": theta,
                              "max_depth": depth,
                              "median": float("%.3g" % r.median), "p90": float("%.3g" % r.p90),
                              "p99": float("%.3g" % r.p99), "p999": float("%.3g" % r.p999),
                              "max": float("%.3g" % r.max), "worst": r.worst, "rms": float("%.3g" % r.rms),
                              "n_zero": r.n_zero, "n_nonfinite": r.n_nonfinite}), flush=True)


def main():
    what = sys.argv[1:] or ["timing", "error"]
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    if "timing" in what:
        timing(stream)
    if "error" in what:
        error()


if __name__ == "__main__":
    main()
