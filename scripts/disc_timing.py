"""What the disc kernels cost, by the HIP events of bh_disc_times: the initialiser, the two passes of the rotation curve, the
velocities -- and, beside them, the two passes of the radial profile on the same state and bins (bh_radial_times).

    python scripts/disc_timing.py [--n 1048576] [--repeats 7] [--bins 32 1022] [--table 32] [--precision F32]

One context (max_depth 21, bucket leaves, softening a tenth of the scale): initialize_disc(n, scale 1, r_max 10) `repeats` times
after one untimed call; then one compute_forces(), which also puts the state in curve order when the re-order cadence says so;
per bin count, after one untimed call each, `repeats` calls of rotation_curve and of radial_profile about the origin on log bins
from 0.01 to 10; then `repeats` calls of set_disc_velocities with a table of --table radii.  A row is the median over the repeats
with their minimum and maximum, in milliseconds.  Prints one JSON line per measurement.  Development aid, not a bench."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_nbody_simulation_amd as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--bins", type=int, nargs="+", default=[32, 1022])
ap.add_argument("--table", type=int, default=32)
ap.add_argument("--precision", choices=["F32", "MIXED", "F64"], default="F32")
a = ap.parse_args()


def row(x):
    x = np.asarray(x)
    return [round(float(np.median(x)), 5), round(float(x.min()), 5), round(float(x.max()), 5)]


def out(what, **kw):
    print(json.dumps({"precision": prec.name, "n": a.n, "repeats": a.repeats, "what": what, **kw}), flush=True)


prec = G.Precision[a.precision]
with G.BarnesHutEngine(G.BhConfig(capacity=a.n, theta=0.5, G=1.0, max_depth=21, precision=prec, softening=0.1,
                                  reference_compat=prec == G.Precision.F64)) as e:
    init = []
    for k in range(a.repeats + 1):
        e.initialize_disc(a.n, 1, 1.0, 1.0, 10.0)
        init.append(e.disc_times()[0])
    out("disc_init_kernel", **{"ms [median, min, max]": row(init[1:])})
    e.compute_forces()
    for nb in a.bins:
        edges = G.radial_edges(0.01, 10.0, nb)
        mx, dep, rmx, rdep = [], [], [], []
        for k in range(a.repeats + 1):
            e.rotation_curve(edges, (0.0, 0.0))
            t = e.disc_times()
            e.radial_profile(edges, (0.0, 0.0))
            r = e.radial_times()
            if k:
                mx.append(t[1]); dep.append(t[2]); rmx.append(r[0]); rdep.append(r[1])
        out("curve_max_kernel", bins=nb, **{"ms [median, min, max]": row(mx)})
        out("curve_deposit_kernel", bins=nb, **{"ms [median, min, max]": row(dep)})
        out("radial_max_kernel", bins=nb, **{"ms [median, min, max]": row(rmx)})
        out("radial_deposit_kernel", bins=nb, **{"ms [median, min, max]": row(rdep)})
    radii = np.geomspace(0.05, 10.0, a.table)
    vel = []
    for k in range(a.repeats + 1):
        e.set_disc_velocities(radii, radii / (1.0 + radii * radii) ** 0.75, 0.1 / (1.0 + radii), 0.07 / (1.0 + radii), seed=1)
        vel.append(e.disc_times()[3])
    out("disc_velocities_kernel", table=a.table, **{"ms [median, min, max]": row(vel[1:])})
