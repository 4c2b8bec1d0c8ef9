"""Measured parity of the distributed step's forest walk against the forest oracle (tests/forest_ref.py), body by body,
for the fixed cases of tests/test_gpu_let_parity.py.  One JSON line per case; that module's tolerances are <= 2x these
measurements.
    python scripts/let_parity_measure.py [case ...]           on an MI355X: the whole report
    python scripts/let_parity_measure.py --cpu [case ...]     no GPU: the oracle's classification alone -- the clean
                                                              fraction every fixed case must keep >= 0.995"""
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    cpu = "--cpu" in argv
    import forest_ref as FR
    import parity_classes as PC
    import test_gpu_let_parity as T
    names = [a for a in argv if not a.startswith("--")] or list(T.CASES)
    for name in names:
        kind, n, theta, partition, world, precision, two, flags, n_threads, waves, tol = T.CASES[name]
        t0 = time.time()
        m, p, v, parts = T.case_state(name)
        ref = FR.forest_diag(m, p, parts, theta, pos_rounded=precision == T.MIXED)
        out = {"case": name, "ranks": [len(ix) for ix in parts], "oracle_s": round(time.time() - t0, 1)}
        ok = np.isfinite(ref.forces).all(axis=1)
        out["clean_fraction"] = float((ref.flip[ok] == 0).mean())
        out["cap_affected"] = int((ref.cap[ok] > 0).sum())
        if not cpu:
            a, cnt, _ = T.forest_step(m, p, v, world, lambda pp, w: parts, theta, precision, two, flags | T.FLAG_WALK_STATS,
                                      n_threads)
            out.update(dataclasses.asdict(PC.classify(a, cnt, m, p, theta, n, diag=ref)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
