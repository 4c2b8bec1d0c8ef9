"""tests/reduction_ref.py on the CPU: that sum2_tolerance, the bound tests/test_gpu_reductions.py holds the device's
energy sums to, tells the summation tree of csrc/bh_diag.hpp apart from its broken variants.

On the nearly cancelling sums of mirrored_state, at every size beyond one grid-stride trip, the exact tree (per-lane
Neumaier pairs, the halving folds with their `c += c2`, a second launch, s + c) meets the bound against math.fsum; a
plain left-to-right sum, numpy's pairwise sum and the tree without `c += c2` miss it at every size, the tree whose
lanes sum plainly from three trips on.  The measured misses: the docstring of tests/reduction_ref.py."""
import math

import numpy as np
import pytest

import reduction_ref as R

CANCELLING = [3, 4, 1, 2]            # m vx, m vy, m x, m y of reduction_ref.terms


@pytest.fixture(scope="module", params=R.SIZES)
def case(request):
    """(n, [(name, term, fsum, tolerance)] of the four cancelling terms)."""
    n = request.param
    m, x, v = R.state(n)
    tt = R.terms(m, x, v, np.zeros(n))
    out = []
    for k in CANCELLING:
        ref, scale = math.fsum(tt[k]), math.fsum(np.abs(tt[k]))
        out.append((R.NAMES[k], tt[k], ref, R.sum2_tolerance(ref, scale, n)))
    return n, out


def test_the_state_is_what_the_helper_says(case):
    n, _ = case
    m, x, v = R.state(n)
    assert len(m) == n and x.shape == v.shape == (n, 2)
    for a in (m, x, v):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))          # one state for all four precisions
    assert len(np.unique(x, axis=0)) == n                                          # no two bodies coincide
    tt = R.terms(m, x, v, np.zeros(n))
    for k in (3, 4):
        assert R.condition(tt[k]) >= R.MIN_CONDITION, (R.NAMES[k], R.condition(tt[k]))
    for k in (1, 2):
        assert R.condition(tt[k]) >= R.MIN_CONDITION_POSITION, (R.NAMES[k], R.condition(tt[k]))
    assert n > R.STRIDE and n % R.STRIDE != 0                                      # a second trip, and a ragged one


def test_the_exact_tree_meets_the_bound(case):
    n, rows = case
    for name, t, ref, tol in rows:
        err = abs(R.device_sum(t) - ref)
        print(f"n {n} {name}: exact tree |err| {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol, (n, name, err, tol)


@pytest.mark.parametrize("variant", ["cumsum", "np.sum", "drop_fold_c"])
def test_the_uncompensated_sums_miss_it(case, variant):
    n, rows = case
    broken = {"cumsum": lambda t: float(np.cumsum(t)[-1]), "np.sum": lambda t: float(np.sum(t)),
              "drop_fold_c": lambda t: R.device_sum(t, drop_fold_c=True)}[variant]
    for name, t, ref, tol in rows:
        err = abs(broken(t) - ref)
        print(f"n {n} {name}: {variant} |err| {err:.3g} = {err / tol:.3g} tolerances")
        assert err > tol, (n, name, variant, err, tol)


def test_lanes_without_compensation_miss_it_from_three_trips_on():
    n = 196909
    m, x, v = R.state(n)
    tt = R.terms(m, x, v, np.zeros(n))
    for k in CANCELLING:
        ref, scale = math.fsum(tt[k]), math.fsum(np.abs(tt[k]))
        tol = R.sum2_tolerance(ref, scale, n)
        err = abs(R.device_sum(tt[k], drop_lane_c=True) - ref)
        print(f"n {n} {R.NAMES[k]}: drop_lane_c |err| {err:.3g} = {err / tol:.3g} tolerances")
        assert err > tol, (R.NAMES[k], err, tol)


def test_the_tolerance_is_the_stated_formula():
    assert R.sum2_tolerance(1.0, 0.0, 5) == 2.0 * 2.0 ** -52
    assert R.sum2_tolerance(-3.0, 4.0, 2 ** 20) == 2.0 * 2.0 ** -51 + (2.0 ** -32) ** 2 * 4.0
    assert R.sum2_tolerance(0.0, 1.0, 1) == 2.0 * 5e-324 + 2.0 ** -104
    # the quotient: exact sums give one rounding and nothing else
    assert R.quotient_tolerance(1.0, 4.0, 0.0, 0.0) == float(np.spacing(0.25))
    assert R.quotient_tolerance(1.0, 4.0, 0.5, 0.0) == 0.125 + float(np.spacing(0.25))
    assert R.quotient_tolerance(1.0, 4.0, 0.0, 2.0) == 0.25 + float(np.spacing(0.25))


def test_the_emulation_is_the_plain_sum_where_nothing_rounds():
    t = np.arange(1.0, 70001.0)
    assert R.device_sum(t) == R.device_sum(t, True, False) == R.device_sum(t, False, True) == 70000 * 70001 / 2
