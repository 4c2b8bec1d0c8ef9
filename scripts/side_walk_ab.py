"""Bit-for-bit A/B of the side walks (potential, energy, field, force check) and of the steps around them between two
builds of libbhgpu, on the GPU box: one fresh subprocess per library (BHGPU_LIB / BHGPU_LIB_OPT_IN), each under its own
timeout, the parent variant first, nothing more started after a timeout or a non-zero exit.

    python -m gpu_nbody_simulation_amd.build --variant parent      # from the parent commit's sources
    python scripts/side_walk_ab.py [--libs parent.so new.so] [--timeout 300]

Cases: the golden init1024 state; 4,096 clumped bodies with 2,048 points around them and one point exactly on a body; the
deep chain of tests/field_ref.py (second tier of the lane stack); n = 1 and n = 0.  Each in the four precisions and in
F64_EXACT with FLAG_WALK_PORTABLE, reference_compat on and off, FLAG_WALK_STATS set, once after upload and once after
step(3): potential with counts, energy, field with counts, force_check on 64 targets, interaction_counts, the stats()
counters before and after those calls; then step(5) and download().  The workers write every array to an .npz; the
driver compares raw bits (a point on a body gives inf and NaN) and prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COUNTERS = ["n_bodies", "n_nodes", "n_internal", "steps_done", "visits", "interactions", "wave_nodes", "wave_quads",
            "wave_accepts", "walk_launches", "device_bytes", "sort_spill_buckets", "sort_rerun_buckets"]


def worker(path):
    import numpy as np
    import gpu_nbody_simulation_amd as G
    from gpu_nbody_simulation_amd.engine import FLAG_WALK_PORTABLE, FLAG_WALK_STATS, BhError
    import field_ref as FR

    P = G.Precision
    gold = os.path.join(ROOT, "tests", "golden", "init1024")
    m0, p0, v0 = (np.loadtxt(os.path.join(gold, f + "_init.txt")) for f in ("masses", "positions", "velocities"))
    pc, mc = FR.clumped(4096, 7)
    pd, md = FR.deep_chain()
    z2 = np.zeros((0, 2))
    few = FR.points_around(p0, 64, 2)
    # name -> positions, velocities, masses, points, theta, max_depth
    cases = {
        "init1024": (p0, v0, m0, FR.points_around(p0, 512, 1), 0.5, 21),
        "clumped4096": (pc, np.zeros_like(pc), mc, np.concatenate([FR.points_around(pc, 2048, 3), pc[17:18]]), 0.5, 21),
        "deep_chain": (pd, np.zeros_like(pd), md, np.concatenate([FR.DEEP_POINT, FR.points_around(pd, 24, 0)[16:24]]),
                       FR.DEEP_THETA, FR.DEEP_DEPTH),
        "one": (p0[:1], v0[:1], m0[:1], few, 0.5, 21),
        "none": (z2, z2, np.zeros(0), few, 0.5, 21),
    }
    configs = [("exact", P.F64_EXACT, 0), ("portable", P.F64_EXACT, FLAG_WALK_PORTABLE), ("f64", P.F64, 0),
               ("mixed", P.MIXED, 0), ("f32", P.F32, 0)]
    out = {}

    def counters(e):
        st = e.stats()
        return np.array([getattr(st, k) for k in COUNTERS], dtype=np.int64)

    def side_walks(e, key, pts):
        out[key + "/stats_before"] = counters(e)
        out[key + "/phi"], out[key + "/phi_counts"] = e.potential(with_counts=True)
        en = e.energy()
        out[key + "/energy"] = np.array([en.kinetic, en.potential, en.total, *en.momentum, en.angular_momentum, *en.com,
                                         en.mass, float(en.n_bodies)])
        out[key + "/field_accel"], out[key + "/field_phi"], out[key + "/field_counts"] = e.field(pts, with_counts=True)
        targets = np.random.default_rng(9).permutation(e.n)[:64] if e.n else None
        out[key + "/check_tree"], out[key + "/check_direct"] = e.force_check(targets)
        try:
            out[key + "/interaction_counts"] = e.interaction_counts()
        except BhError as err:                                    # (no counts in the bit-exact mode, none before a walk)
            out[key + "/interaction_counts"] = np.array([err.code], dtype=np.int64)
        out[key + "/stats_after"] = counters(e)

    for cname, (p, v, m, pts, theta, depth) in cases.items():
        for label, prec, flags in configs:
            for compat in (True, False):
                key = "%s/%s/compat%d" % (cname, label, compat)
                cfg = G.BhConfig(capacity=max(len(m), 1), theta=theta, max_depth=depth, precision=prec,
                                 reference_compat=compat, flags=flags | FLAG_WALK_STATS)
                with G.BarnesHutEngine(cfg) as e:
                    e.upload(p, v, m)
                    side_walks(e, key + "/uploaded", pts)
                    e.step(3)
                    side_walks(e, key + "/stepped", pts)
                    e.step(5)
                    out[key + "/pos"], out[key + "/vel"] = e.download()
                    out[key + "/stats_end"] = counters(e)
    np.savez(path, **out)
    print(json.dumps({"lib": os.path.basename(os.environ.get("BHGPU_LIB", "libbhgpu.so")), "arrays": len(out)}))


def raw(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def main():
    ap = argparse.ArgumentParser()
    pkg = os.path.join(ROOT, "gpu-nbody-simulation_amd")
    ap.add_argument("--libs", nargs=2, default=[os.path.join(pkg, "build", "libbhgpu_parent.so"), os.path.join(pkg, "libbhgpu.so")])
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for i, lib in enumerate(a.libs):
            files.append(os.path.join(tmp, "lib%d.npz" % i))
            env = dict(os.environ, BHGPU_LIB=os.path.abspath(lib), BHGPU_LIB_OPT_IN="1")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", files[-1]], env=env,
                                   capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"lib": os.path.basename(lib), "error": "timeout"}), flush=True)
                return 1                                          # a hung kernel: run nothing else on this box
            print(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "", flush=True)
            if r.returncode != 0:
                print(json.dumps({"lib": os.path.basename(lib), "error": "rc=%d" % r.returncode, "stderr": r.stderr[-600:]}),
                      flush=True)
                return 1
        x, y = (np.load(f) for f in files)
        different = sorted(set(x.files) ^ set(y.files))
        for k in sorted(set(x.files) & set(y.files)):
            if x[k].shape != y[k].shape or x[k].dtype != y[k].dtype or not np.array_equal(raw(x[k]), raw(y[k])):
                different.append(k)
        nonfinite = sum(int((~np.isfinite(x[k])).sum()) for k in x.files if x[k].dtype == np.float64)
        print(json.dumps({"libs": [os.path.basename(l) for l in a.libs], "arrays": len(x.files), "values": int(sum(x[k].size for k in x.files)),
                          "nonfinite_values": nonfinite, "different": different[:20], "n_different": len(different),
                          "bitwise_equal": not different}))
        return 0 if not different else 2


if __name__ == "__main__":
    sys.exit(main())
