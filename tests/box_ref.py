"""The root box of a position set as ComputeRootBounds (project.cu:536-573) forms it -- a helper of
tests/test_box_ref_cpu.py, tests/test_gpu_next_rows.py and tests/test_gpu_walk_bounds.py, not a test file.

min/max start from +-inf and a NaN coordinate never wins a compare, so NaN coordinates are skipped axis by axis; the
box is padded on every side by a tenth of the larger extent (1e-6 when both extents are zero).  Every operation is one
IEEE fp64 operation as the reference writes it, so the result is bitwise the reference's (tests/test_box_ref_cpu.py
pins it against the oracle's tree)."""
from __future__ import annotations

import numpy as np


def box_ref(p) -> np.ndarray:
    """[xmin, xmax, ymin, ymax] of the root cell for positions p [n, 2]."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    xs, ys = p[:, 0][~np.isnan(p[:, 0])], p[:, 1][~np.isnan(p[:, 1])]
    lo = np.array([xs.min(initial=np.inf), ys.min(initial=np.inf)])
    hi = np.array([xs.max(initial=-np.inf), ys.max(initial=-np.inf)])
    ex, ey = hi - lo
    span = ey if ex < ey else ex
    pad = 1e-6 if span == 0.0 else 0.1 * span
    return np.array([lo[0] - pad, hi[0] + pad, lo[1] - pad, hi[1] + pad])


def root_box(nodes) -> np.ndarray:
    """[xmin, xmax, ymin, ymax] of node 0 of a tree (the oracle's NODE_DTYPE or the engine's export)."""
    return np.array([nodes[0]["xmin"], nodes[0]["xmax"], nodes[0]["ymin"], nodes[0]["ymax"]], dtype=np.float64)
