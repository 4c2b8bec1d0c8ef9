"""The work counters of the five traversals of the neighbour index (nb_walk, csrc/bh_neighbours.hpp) at the smallest sizes that
have every case: what tests/golden/index_walk_counters.json records and tests/test_gpu_index_walk.py holds the product library to.

    BHGPU_LIB=.../libbhgpu_parent.so BHGPU_LIB_OPT_IN=1 python scripts/index_walk_counters.py > tests/golden/index_walk_counters.json

The counters depend on which nodes and bodies every lane meets, in which order and under which conditions -- the results do
not -- so a record taken with the library of one commit pins the traversal of the next.  States:
tests/neighbours_ref.uniform(n) at n = 65 (three levels, a ragged last leaf, a last wave of one lane), 513 and 4,096, F64 and
F32, straight after upload.  Per case:
  knn      evals of neighbours(k) at k = 1 and 8 as sum, max and the SHA-256 of the caller-order uint32 array, for the bodies and
           for the first 100 bodies' positions as points;
  pairs    evals of pair_counts over eight log bins from the median first-neighbour distance to the box diagonal, bodies and the
           same points;
  groups   stats of groups(b) at b = the median second-neighbour distance;
  mst      stats of spanning_tree().
The edges and b are part of the record (they come out of pow and sqrt): a replay passes the record's own.  Prints one JSON
record.  count_within has no counter."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gpu_nbody_simulation_amd as G  # noqa: E402
import neighbours_ref as NR  # noqa: E402

SIZES = (65, 513, 4096)
PRECISIONS = ("F64", "F32")
KS = (1, 8)
N_POINTS, N_BINS = 100, 8


def evals_record(ev):
    ev = np.ascontiguousarray(ev, dtype="<u4")
    return {"sum": int(ev.sum(dtype=np.uint64)), "max": int(ev.max()), "sha256": hashlib.sha256(ev.tobytes()).hexdigest()}


def case(n, precision, edges=None, linking_length=None):
    """the record of one state; edges, linking_length: those of an earlier record instead of this run's own"""
    prec = G.Precision[precision]
    kw = {"max_depth": 21, "reference_compat": False} if prec == G.Precision.F32 else {}
    m, p, v = NR.uniform(n)
    with G.BarnesHutEngine(G.BhConfig(capacity=n, precision=prec, **kw)) as e:
        e.upload(p, v, m)
        pos = e.download()[0]
        pts = pos[:N_POINTS].copy()
        rec = {"n": n, "precision": precision, "knn": {}}
        d2 = {}
        for k in KS:
            _, d2[k], ev = e.neighbours(k, with_evals=True)
            rec["knn"][f"bodies_k{k}"] = evals_record(ev)
            rec["knn"][f"points_k{k}"] = evals_record(e.neighbours(k, pts, with_evals=True)[2])
        if edges is None:
            diagonal = float(np.hypot(*(pos.max(axis=0) - pos.min(axis=0))))
            edges = G.radial_edges(float(np.sqrt(np.median(d2[1][:, 0]))), diagonal, N_BINS).tolist()
        if linking_length is None:
            linking_length = float(np.sqrt(np.median(d2[8][:, 1])))
        rec["edges"], rec["linking_length"] = list(edges), linking_length
        rec["pairs"] = {"bodies": int(e.pair_counts(edges, with_evals=True).evals),
                        "points": int(e.pair_counts(edges, pts, with_evals=True).evals)}
        rec["groups [distances, pairs, hooks]"] = list(e.groups(linking_length, with_stats=True).stats)
        rec["mst [rounds, distances, skipped nodes, edges]"] = list(e.spanning_tree(with_stats=True).stats)
    return rec


if __name__ == "__main__":
    print(json.dumps({"cases": [case(n, prec) for n in SIZES for prec in PRECISIONS]}, indent=1))
