"""tests/box_ref.py -- the root-box reference of the GPU box tests -- against the oracle's tree, without a GPU: the root
node's xmin / xmax / ymin / ymax of oracle.bh_oracle.build_tree (ComputeRootBounds, project.cu:536-573) bit for bit, on
seeded sets at the edges of the formula."""
import numpy as np
import pytest

from oracle import bh_oracle as O
from box_ref import box_ref, root_box


def _case(name, seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(50, 400))
    if name == "n1":
        return r.uniform(-1, 1, (1, 2))
    if name == "n2":
        return r.uniform(-1, 1, (2, 2))
    if name == "coincident":                                     # both extents zero: pad 1e-6
        return np.repeat(r.uniform(-1, 1, (1, 2)), n, axis=0)
    if name == "one_nan":
        p = r.uniform(-1, 1, (n, 2))
        p[r.integers(0, n)] = np.nan
        return p
    if name == "several_nan":                                    # whole bodies and single coordinates
        p = r.uniform(-1, 1, (n, 2))
        p[r.choice(n, 5, replace=False)] = np.nan
        p[r.choice(n, 3, replace=False), 0] = np.nan
        p[r.choice(n, 3, replace=False), 1] = np.nan
        return p
    if name == "wide_x":                                         # x extent 1e6 times the y extent
        return np.column_stack([r.uniform(-1e3, 1e3, n), r.uniform(-1e-3, 1e-3, n)])
    if name == "wide_y":
        return np.column_stack([r.uniform(-1e-3, 1e-3, n), r.uniform(-1e3, 1e3, n)])
    if name == "offset":                                         # coordinates near 1e8: the pad is a few hundred ulps
        return 1e8 + r.uniform(-1.0, 1.0, (n, 2)) * np.array([1.0, 0.25])
    if name == "fp32":                                           # fp32-widened, as the fp32 modes hold them
        return r.normal(0, 0.3, (n, 2)).astype(np.float32).astype(np.float64)
    raise ValueError(name)


CASES = ["n1", "n2", "coincident", "one_nan", "several_nan", "wide_x", "wide_y", "offset", "fp32"]


@pytest.mark.parametrize("name", CASES)
def test_box_ref_is_the_oracle_root_box(name):
    for seed in range(4):
        p = _case(name, 100 * seed + CASES.index(name))
        m = np.random.default_rng(seed).uniform(0.1, 0.5, len(p))
        expect = root_box(O.build_tree(p, m, 10))
        got = box_ref(p)
        assert np.array_equal(got.view(np.uint64), expect.view(np.uint64)), (name, seed, got, expect)
        assert np.array_equal(got.view(np.uint64), O.root_bounds(p).view(np.uint64))
        assert np.isfinite(got).all()
    if name == "coincident":
        assert got[1] - got[0] > 0 and got[1] == p[0, 0] + 1e-6


def test_box_ref_all_nan_is_the_empty_box():
    """No coordinate ever wins a compare: the box stays {+inf, -inf, +inf, -inf}, as the reference's does."""
    p = np.full((3, 2), np.nan)
    assert np.array_equal(box_ref(p), [np.inf, -np.inf, np.inf, -np.inf])
    assert np.array_equal(box_ref(p), O.root_bounds(p))
