"""Neighbour queries without a GPU.

  * the numpy twin tests/neighbours_ref.py (what tests/test_gpu_neighbours.py compares the device with) is held to an
    independent plain-Python version -- float arithmetic, `sorted` on (d2, j) tuples -- on random bodies, a lattice full of
    ties, duplicates and n < k; the host-side density estimate of the package is held to the twin's loop;
  * every kernel of csrc/bh_neighbours.hpp meets the resource conditions: no scratch, no spills, no dynamic stack, at most
    64 VGPRs (hipcc cross-compiles);
  * header, binding and Python names are there."""
import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
from gpu_nbody_simulation_amd import engine as E
import kernel_meta as KM
import neighbours_ref as R


def cases():
    rng = np.random.default_rng(2)
    rnd = rng.normal(size=(150, 2))
    dup = rng.normal(size=(60, 2))
    dup[20:45] = dup[3]                                           # 26 bodies at one place
    few = rng.normal(size=(5, 2))
    return {"random": rnd, "lattice": R.lattice(9), "duplicates": dup, "fewer-than-k": few, "one": few[:1], "none": few[:0]}


@pytest.mark.parametrize("name", list(cases()))
@pytest.mark.parametrize("k", [1, 8, 32])
def test_twin_equals_plain_python_for_bodies(name, k):
    pos = cases()[name]
    idx, d2 = R.neighbours(pos, k)
    idx_py, d2_py = R.neighbours_py(pos, k)
    assert idx.shape == (len(pos), k) and idx.dtype == np.int64 and d2.dtype == np.float64
    assert np.array_equal(idx, idx_py) and np.array_equal(d2, d2_py)
    if len(pos) <= k:                                             # padded: n - 1 neighbours, then -1 / +inf
        assert (idx[:, max(len(pos) - 1, 0):] == -1).all() and np.isinf(d2[:, max(len(pos) - 1, 0):]).all()
    assert not (idx == np.arange(len(pos))[:, None]).any()        # nobody is its own neighbour


@pytest.mark.parametrize("name", list(cases()))
def test_twin_equals_plain_python_for_points(name):
    pos = cases()[name]
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.normal(size=(20, 2)), pos[:10], [[1e6, -1e6]]])     # on bodies too: d2 = 0 counts, nobody left out
    for k in (1, 6):
        idx, d2 = R.neighbours(pos, k, pts)
        idx_py, d2_py = R.neighbours_py(pos, k, pts)
        assert np.array_equal(idx, idx_py) and np.array_equal(d2, d2_py)
    if len(pos) >= 10:
        assert (R.neighbours(pos, 1, pts)[1][20:30, 0] == 0.0).all()
    # a subset of the queries gives the same rows
    rows = np.array([5, 0, 17])
    assert np.array_equal(R.neighbours(pos, 6, pts, rows)[0], R.neighbours(pos, 6, pts)[0][rows])


@pytest.mark.parametrize("name", list(cases()))
def test_count_twin_equals_plain_python(name):
    pos = cases()[name]
    pts = np.concatenate([np.random.default_rng(8).normal(size=(10, 2)), pos[:5]])
    for radius in (0.0, 0.3, 1.0, 2.0, 1e3):
        assert np.array_equal(R.count_within(pos, radius), R.count_within_py(pos, radius))
        assert np.array_equal(R.count_within(pos, radius, pts), R.count_within_py(pos, radius, pts))
    if name == "duplicates":
        assert R.count_within(pos, 0.0)[3] == 25                  # the others at its place, not itself
    if name == "lattice":                                         # inclusive at equality, exclusive just below
        i = int(np.nonzero((pos == [4.0, 4.0]).all(axis=1))[0][0])
        assert R.count_within(pos, 2.0)[i] == 12 and R.count_within(pos, np.nextafter(2.0, 0.0))[i] == 8


def test_ties_fall_to_the_smaller_caller_index():
    pos = R.lattice(9)
    idx, d2 = R.neighbours(pos, 8)
    i = int(np.nonzero((pos == [4.0, 4.0]).all(axis=1))[0][0])
    assert list(d2[i]) == [1.0] * 4 + [2.0] * 4
    assert list(idx[i, :4]) == sorted(idx[i, :4]) and list(idx[i, 4:]) == sorted(idx[i, 4:])


def test_local_density_and_centre():
    rng = np.random.default_rng(4)
    pos = rng.normal(size=(80, 2))
    pos[10:17] = pos[2]                                           # 8 coincident: d2 of the 6th is 0 there
    m = 10.0 ** rng.uniform(-3, 3, size=80)
    idx, d2 = R.neighbours(pos, 6)
    sigma, r_k = E.local_density_from(idx, d2, m)
    want_s, want_r = R.local_density(idx, d2, m)
    assert np.array_equal(sigma, want_s, equal_nan=True) and np.array_equal(r_k, want_r)
    assert np.isinf(sigma[2]) and np.isinf(sigma[10:17]).all() and np.isfinite(np.delete(sigma, [2] + list(range(10, 17)))).all()
    assert np.array_equal(G.density_centre_from(sigma, pos), R.density_centre(sigma, pos))
    # fewer than k neighbours: NaN, and no centre
    idx3, d23 = R.neighbours(pos[:4], 6)
    s3, r3 = G.local_density_from(idx3, d23, m[:4])
    assert np.isnan(s3).all() and np.isinf(r3).all()
    assert np.array_equal(s3, R.local_density(idx3, d23, m[:4])[0], equal_nan=True)
    assert np.isnan(G.density_centre_from(s3, pos[:4])).all() and np.isnan(R.density_centre(s3, pos[:4])).all()
    with pytest.raises(ValueError):
        G.local_density_from(idx[:, :1], d2[:, :1], m)


# ---- resources ----------------------------------------------------------------------------------------------------------------
def test_every_neighbour_kernel_meets_the_resource_conditions():
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+nb_[a-z]+_kernel\S*")
    names = sorted(ks)
    # bounds and keys and gather for both state types, setup, leaf, level, the two searches for bodies and for points
    assert len(ks) >= 13, names
    for stem, count in (("nb_bounds_kernel", 2), ("nb_keys_kernel", 2), ("nb_gather_kernel", 2), ("nb_setup_kernel", 1),
                        ("nb_leaf_kernel", 1), ("nb_level_kernel", 1), ("nb_knn_kernel", 2), ("nb_count_kernel", 2)):
        assert sum(stem in k for k in ks) == count, (stem, names)
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


def test_the_traversals_load_boxes_and_leaf_bodies_through_the_scalar_unit():
    """What is left of vector loads in a search kernel is the lane's own query and its seeds (a point: its order, key and
    the binary search too); boxes, level offsets and leaf bodies come at wave-uniform addresses."""
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+nb_(?:knn|count)_kernel\S*")
    assert len(ks) == 4
    for name in ks:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        loads = body.count("global_load") + body.count("flat_load") + body.count("buffer_load")
        print(name, loads, body.count("s_load_dwordx4"))
        assert loads <= (6 if "nb_knn" in name else 3), (name, loads)
        assert body.count("s_load_dwordx4") >= 3, name            # two for an NbBox, one for a leaf body


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    for sym in ("bh_neighbours", "bh_count_within", "bh_neighbours_times"):
        assert sym in _lib.SIGNATURES and hasattr(_lib.load(), sym)
    for meth in ("neighbours", "count_within", "local_density", "density_centre"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    assert E.NEIGHBOURS_MAX_K == 32 == R.MAX_K
    assert "BH_NEIGHBOURS_MAX_K 32" in open(KM.ROOT + "/include/bhgpu.h").read()
