"""Direct-sum forces and the force-error statistics, without a GPU: the C-ABI declarations and bindings, the host-side
reduction force_error_stats, and the numpy reference tests/direct_ref.py against the oracle's direct sum."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from oracle import bh_oracle as O
from gpu_nbody_simulation_amd import _lib
from gpu_nbody_simulation_amd.engine import BhForceError, force_error_stats, sample_targets
from direct_ref import direct_ref, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bh_direct_forces", "bh_force_check")


def test_header_declares_library_exports_and_binding_binds_the_new_calls():
    hdr = open(os.path.join(ROOT, "include", "bhgpu.h")).read()
    assert re.search(r"int bh_direct_forces\(bh_ctx \*ctx, const int64_t \*targets, int64_t n_targets, double \*forces\);", hdr)
    assert re.search(r"int bh_force_check\(bh_ctx \*ctx, const int64_t \*targets, int64_t n_targets, double \*tree, "
                     r"double \*direct\);", hdr)
    lib = C.CDLL(_lib.PRODUCT_LIB)
    for name in NEW:
        getattr(lib, name)                                   # AttributeError if not exported
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["bh_direct_forces"][1][2] is C.c_int64
    assert len(_lib.SIGNATURES["bh_force_check"][1]) == 5
    assert _lib.ABI_VERSION == 4


def _order_stat(rel, num, den):
    """The sorted value at index ceil(q m) - 1, q = num / den exactly."""
    return sorted(rel)[math.ceil(Fraction(num, den) * len(rel)) - 1]


def test_force_error_stats_order_statistics_and_worst_index():
    rng = np.random.default_rng(3)
    for m in (1, 2, 3, 7, 10, 100, 999, 1000, 1001, 4096):
        direct = rng.normal(size=(m, 2))
        tree = direct * (1.0 + rng.normal(scale=1e-3, size=(m, 1))) + rng.normal(scale=1e-4, size=(m, 2))
        targets = rng.permutation(10 * m)[:m]
        r = force_error_stats(tree, direct, targets)
        rel = np.hypot(*(tree - direct).T) / np.hypot(*direct.T)
        assert r.n == m and r.n_zero == 0 and r.n_nonfinite == 0
        assert r.median == _order_stat(rel, 1, 2)
        assert r.p90 == _order_stat(rel, 9, 10)
        assert r.p99 == _order_stat(rel, 99, 100)
        assert r.p999 == _order_stat(rel, 999, 1000)
        assert r.max == rel.max() and r.worst == targets[np.argmax(rel)]
        df, fd = np.hypot(*(tree - direct).T), np.hypot(*direct.T)
        assert r.rms == pytest.approx(math.sqrt(np.mean(df ** 2)) / math.sqrt(np.mean(fd ** 2)), rel=1e-14)
    # without targets the worst index is the row
    r = force_error_stats([[1.0, 0.0], [3.0, 0.0], [2.0, 0.0]], [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
    assert (r.worst, r.max, r.median, r.p90) == (1, 2.0, 1.0, 2.0)


def test_force_error_stats_excludes_zero_and_nonfinite_bodies():
    tree = np.array([[1.0, 0.0], [np.nan, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 0.0], [0.0, 0.0], [1.0, np.inf]])
    direct = np.array([[1.0, 0.5], [1.0, 1.0], [np.inf, 1.0], [0.0, 0.0], [1.0, 0.0], [-0.0, 0.0], [1.0, 1.0]])
    r = force_error_stats(tree, direct, [10, 11, 12, 13, 14, 15, 16])
    assert (r.n, r.n_zero, r.n_nonfinite) == (2, 2, 3)
    rel = [0.5 / math.hypot(1.0, 0.5), 1.0]
    assert r.median == min(rel) and r.max == 1.0 and r.worst == 14
    assert all(np.isfinite([r.median, r.p90, r.p99, r.p999, r.max, r.rms]))
    e = force_error_stats(np.zeros((2, 2)), np.zeros((2, 2)))
    assert (e.n, e.n_zero, e.worst) == (0, 2, -1) and math.isnan(e.median)
    assert isinstance(force_error_stats(np.zeros((0, 2)), np.zeros((0, 2))), BhForceError)


def test_sample_targets_are_distinct_seeded_and_capped():
    a = sample_targets(100000, 4096, 7)
    assert len(a) == 4096 and len(np.unique(a)) == 4096 and a.dtype == np.int64
    assert np.array_equal(a, sample_targets(100000, 4096, 7))
    assert np.array_equal(np.sort(sample_targets(50, 65536, 0)), np.arange(50))


def test_direct_ref_equals_the_oracle_on_init1024(init1024):
    m, p, _ = init1024
    full = O.direct_forces(p, m)
    t = np.random.default_rng(0).choice(len(m), 64, replace=False)
    assert np.array_equal(direct_ref(p, m, t), full[t])
    assert np.array_equal(direct_ref(p, m, [0, 1023, 512]), full[[0, 1023, 512]])


@pytest.mark.parametrize("seed", [1, 2])
def test_direct_ref_equals_the_oracle_on_random_systems_with_coincident_bodies(seed):
    r = np.random.default_rng(seed)
    n = 3000
    p = r.uniform(-1.0, 1.0, (n, 2)) * 10.0 ** r.uniform(-4, 0, (n, 1))
    m = r.uniform(0.1, 0.5, n)
    m[5] = 0.0                                               # a massless body: no special case
    p[7] = p[8] = p[9]                                       # three coincident bodies: inf * 0 = NaN rows
    full = O.direct_forces(p, m)
    t = np.concatenate([[5, 7, 8, 9, 0, n - 1], r.choice(n, 40, replace=False)])
    got = direct_ref(p, m, t)
    assert same_bits(got, full[t])
    assert np.isnan(got[1:4]).all() and np.isfinite(got[4:6]).all()
    assert same_bits(direct_ref(p, m, t, G=1.0), O.direct_forces(p, m, G=1.0)[t])
