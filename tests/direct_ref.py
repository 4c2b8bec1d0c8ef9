"""Exact numpy reference of the direct-sum forces (main_approach_1.cpp:53-75) for a few targets at any N -- a helper of
tests/test_direct_cpu.py and tests/test_gpu_direct.py, not a test file.

For a target i the per-j terms are formed as the reference forms them (dx = p[j].x - p[i].x; d2 = 0.0 + dx*dx;
d2 += dy*dy; d = sqrt(d2); k = ((G*m_i)*m_j) / (d2*d); k*dx, k*dy), element by element in IEEE fp64 (numpy neither fuses
nor reorders an elementwise expression), the j == i term is dropped by index, and the terms are summed SEQUENTIALLY in j
order: np.cumsum over [0.0, t_0, t_1, ...] is the reference's left-to-right `sum[k] += ...` (np.sum is pairwise and
would not match)."""
from __future__ import annotations

import numpy as np


def direct_ref(pos, mass, targets, G: float = 6.67e-11) -> np.ndarray:
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    mass = np.asarray(mass, dtype=np.float64).reshape(-1)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    out = np.empty((len(targets), 2))
    for r, i in enumerate(targets):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dx = pos[:, 0] - pos[i, 0]
            d2 = 0.0 + dx * dx
            dy = pos[:, 1] - pos[i, 1]
            d2 = d2 + dy * dy
            d = np.sqrt(d2)
            k = ((G * mass[i]) * mass) / (d2 * d)
            tx, ty = np.delete(k * dx, i), np.delete(k * dy, i)
            out[r, 0] = np.cumsum(np.concatenate(([0.0], tx)))[-1]
            out[r, 1] = np.cumsum(np.concatenate(([0.0], ty)))[-1]
    return out


def same_bits(a, b) -> bool:
    """Bit for bit, except that any NaN equals any NaN (the payload of a NaN made from inf * 0 is not specified: x86
    makes the negative default NaN, the GPU the positive one)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
