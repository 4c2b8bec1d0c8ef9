"""Neighbour lists without a GPU.

  * the numpy twin tests/neighbour_lists_ref.py (what tests/test_gpu_neighbour_lists.py compares the device with) is held to an
    independent plain-Python version, to the twins of count_within, neighbours and groups, and its fixtures are shown to have
    empty rows, rows of a few entries and of more than 32, and rows whose order the tie-break decides;
  * BhNeighbourLists built from the twin's arrays: row, counts, nearest, pairs and the ValueError cases;
  * every kernel of csrc/bh_neighbour_lists.hpp meets the resource conditions: no scratch, no spills, no dynamic stack, at most
    64 VGPRs (hipcc cross-compiles), and the fill kernel reads boxes and leaf bodies through the scalar unit;
  * header, binding and Python names are there, and the fp32 walk's translation unit knows nothing of them."""
import functools
import re

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
import groups_ref as GR
import kernel_meta as KM
import neighbour_lists_ref as L
import neighbours_ref as R


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def uniform513():
    pos = R.uniform(513)[1]
    pos.setflags(write=False)
    return pos, L.r8_of(pos)


def coincident():
    rng = np.random.default_rng(2)
    pos = rng.normal(size=(60, 2))
    pos[20:40] = pos[3]                                           # 21 bodies at one place
    return pos


# ---- the twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "coincident", "none", "one", "two"])
def test_twin_equals_plain_python(name):
    few = np.random.default_rng(3).normal(size=(2, 2))
    pos = {"uniform": R.uniform(150)[1], "coincident": coincident(), "none": few[:0], "one": few[:1], "two": few}[name]
    scale = 0.1 if name == "uniform" else 1.0
    pts = np.concatenate([np.random.default_rng(8).normal(size=(10, 2)) * scale, pos[:5], [[1e6, -1e6]]])
    for radius in (0.0, 0.3 * scale, 1.0 * scale, 1e3):
        assert same(L.lists(pos, radius), L.lists_py(pos, radius)), radius
        assert same(L.lists(pos, radius, pts), L.lists_py(pos, radius, pts)), radius
        off, idx, d2 = L.lists(pos, radius, pts)
        # a point that lies on a body lists that body first, at d2 = 0
        for k in range(min(len(pos), 5)):
            assert d2[off[10 + k]] == 0.0 and k in idx[off[10 + k]:off[10 + k + 1]][d2[off[10 + k]:off[10 + k + 1]] == 0.0]
    per = np.random.default_rng(9).uniform(0.0, 1.0 * scale, size=len(pos))
    per[::3] = 0.0
    assert same(L.lists(pos, per), L.lists_py(pos, per))
    if name == "coincident":                                      # the 20 others at its place, in index order, not itself
        off, idx, d2 = L.lists(pos, 0.0)
        assert list(idx[off[3]:off[4]]) == list(range(20, 40)) and list(idx[off[25]:off[26]]) == [3] + [j for j in range(20, 40) if j != 25]
    # a subset of the queries gives the same rows
    if len(pos) > 40:
        rows = np.array([5, 0, 17, 40])
        off, idx, d2 = L.lists(pos, per)
        soff, sidx, sd2 = L.lists(pos, per, rows=rows)
        for k, r in enumerate(rows):
            assert np.array_equal(sidx[soff[k]:soff[k + 1]], idx[off[r]:off[r + 1]])


@pytest.mark.parametrize("fixture", ["uniform", "lattice"])
def test_twin_agrees_with_the_other_twins(fixture):
    pos, radius = (uniform513()[0], uniform513()[1] * 2.0) if fixture == "uniform" else (R.lattice(24), 2.0)
    n = len(pos)
    pts = np.concatenate([pos[:9], np.random.default_rng(4).uniform(pos.min(), pos.max(), size=(30, 2))])
    off, idx, d2 = L.lists(pos, radius)
    assert np.array_equal(np.diff(off), R.count_within(pos, radius))
    assert np.array_equal(np.diff(L.lists(pos, radius, pts)[0]), R.count_within(pos, radius, pts))
    # one radius: the relation is symmetric
    who = np.repeat(np.arange(n), np.diff(off))
    assert set(zip(who.tolist(), idx.tolist())) == set(zip(idx.tolist(), who.tolist()))
    # the first min(k, len) entries of a row are the k nearest neighbours that lie within the radius
    r2 = float(radius) * float(radius)
    for k in (1, 8, 32):
        kidx, kd2 = R.neighbours(pos, k)
        for r in range(n):
            keep = kd2[r] <= r2
            m = min(k, off[r + 1] - off[r])
            assert keep.sum() == m
            assert np.array_equal(idx[off[r]:off[r] + m], kidx[r][keep]) and np.array_equal(d2[off[r]:off[r] + m], kd2[r][keep])
    # the components of the pairs are the friends-of-friends groups at that length
    lo, hi, pd2 = L.pairs(off, idx, d2)
    assert (lo < hi).all() and len(lo) * 2 == len(idx)
    assert np.array_equal(L.components(n, lo, hi), GR.groups(pos, radius)[0])


def test_the_fixtures_are_not_trivial():
    pos, r8 = uniform513()
    assert abs(r8 - 0.0138) < 0.0005
    off, idx, d2 = L.lists(pos, r8)
    lens = np.diff(off)
    assert off[-1] == 3862 and lens.max() == 15 and (lens == 0).sum() == 2
    lens = np.diff(L.lists(pos, 4.0 * r8)[0])
    print("uniform(513) at 4 r8: rows > 32:", (lens > 32).sum(), "longest", lens.max())
    assert (lens > 32).sum() >= 500
    lat = R.lattice(24)
    lens = np.diff(L.lists(lat, 2.0)[0])
    assert lens.min() >= 5 and lens.max() <= 12
    off, idx, d2 = L.lists(lat, 5.0)
    lens = np.diff(off)
    distinct = max(len(np.unique(d2[off[r]:off[r + 1]])) for r in range(len(lat)))
    print("lattice(24) at 5: rows of", lens.min(), "to", lens.max(), "entries, at most", distinct, "distinct d2")
    assert lens.min() >= 25 and lens.max() <= 80 and distinct <= 14


# ---- the Python object ----------------------------------------------------------------------------------------------------------
def test_the_object_built_from_the_twin():
    pos, r8 = uniform513()
    off, idx, d2 = L.lists(pos, r8)
    nl = G.neighbour_lists_from(off, idx, d2, r8, True)
    assert isinstance(nl, G.BhNeighbourLists) and len(nl) == 513 and nl.radius == r8
    assert np.array_equal(nl.counts, np.diff(off)) and nl.counts.dtype == np.int64
    for r in (0, 17, 512):
        ri, rd = nl.row(r)
        assert np.array_equal(ri, idx[off[r]:off[r + 1]]) and np.array_equal(rd, d2[off[r]:off[r + 1]])
        assert ri.base is not None and rd.base is not None          # views
    ni, nd = nl.nearest()
    k1 = R.neighbours(pos, 1)
    empty = np.diff(off) == 0
    assert empty.sum() == 2 and (ni[empty] == -1).all() and np.isinf(nd[empty]).all()
    assert np.array_equal(ni[~empty], k1[0][~empty, 0]) and np.array_equal(nd[~empty], k1[1][~empty, 0])
    lo, hi, pd2 = nl.pairs()
    assert same((lo, hi, pd2), L.pairs(off, idx, d2))
    assert (lo < hi).all() and len(lo) == 3862 // 2 and len(set(zip(lo.tolist(), hi.tolist()))) == len(lo)
    key = lo * 513 + hi
    assert (np.diff(key) > 0).all()                                  # ascending in (lo, hi), every pair once
    # per-query radii and points: the relation is one-sided, there are no pairs
    per = np.full(513, r8)
    with pytest.raises(ValueError):
        G.neighbour_lists_from(off, idx, d2, per, True).pairs()
    poff, pidx, pd2 = L.lists(pos, r8, pos[:7])
    with pytest.raises(ValueError):
        G.neighbour_lists_from(poff, pidx, pd2, r8, False).pairs()
    with pytest.raises(ValueError):
        G.neighbour_lists_from(off, idx[:-1], d2, r8, True)
    with pytest.raises(ValueError):
        G.neighbour_lists_from(off, idx, d2, per[:5], True)
    # nobody at all
    none = G.neighbour_lists_from([0], [], [], 1.0, True)
    assert len(none) == 0 and len(none.pairs()[0]) == 0 and len(none.nearest()[0]) == 0


# ---- resources ----------------------------------------------------------------------------------------------------------------
def nbl_kernels():
    text = KM.assembly("bh_engine.hip")[0]
    return text, KM.kernels(text, r"_ZN2bh\d+nbl_[a-z_]+_kernel\S*")


def test_every_neighbour_list_kernel_meets_the_resource_conditions():
    text, ks = nbl_kernels()
    names = sorted(ks)
    for stem, count in (("nbl_count_kernel", 2), ("nbl_fill_kernel", 2), ("nbl_sort_kernel", 2), ("nbl_scan_totals_kernel", 1),
                        ("nbl_scan_bases_kernel", 1), ("nbl_scan_apply_kernel", 1)):
        assert sum(stem in k for k in ks) == count, (stem, names)
    assert len(ks) == 9, names
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


def test_the_fill_and_count_kernels_read_the_index_through_the_scalar_unit():
    """Boxes, level offsets and leaf bodies come at wave-uniform addresses, as in the other kernels on nb_walk; what is left of
    vector loads is the lane's own query, radius, row length and cursor."""
    text, ks = nbl_kernels()
    walkers = [k for k in ks if "nbl_fill" in k or "nbl_count" in k]
    assert len(walkers) == 4
    for name in walkers:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        print(name, body.count("global_load"), body.count("s_load_dwordx4"))
        assert body.count("flat_load") == 0 and body.count("buffer_load") == 0, name
        assert body.count("global_load") <= 6, name
        assert body.count("s_load_dwordx4") >= 3, name            # two for an NbBox, one for a leaf body


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    lib = _lib.load()
    for sym, arity in (("bh_neighbour_lists", 11), ("bh_neighbour_lists_times", 5), ("bh_neighbour_lists_evals", 3)):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        assert len(_lib.SIGNATURES[sym][1]) == arity
    for meth in ("neighbours_within", "neighbour_lists_times"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    assert "BhNeighbourLists" in G.__all__ and "neighbour_lists_from" in G.__all__
    header = open(KM.ROOT + "/include/bhgpu.h").read()
    assert "#define BHGPU_ABI_VERSION 4 " in header
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int bh_neighbour_lists(bh_ctx *ctx, const double *points, int64_t n_points, const double *radii, int64_t n_radii, "
            "int64_t max_entries, int64_t *offsets , int64_t *idx, double *d2, int64_t *n_entries, uint64_t stats[4]);") in flat
    assert ("int bh_neighbour_lists_times(bh_ctx *ctx, double *build_ms, double *count_ms, double *fill_ms, double *sort_ms);"
            in header)


def test_the_fp32_walk_unit_does_not_know_the_lists():
    for name in ("bh_walk_fast.hip", "bh_walk_fast.h"):
        text = open(KM.ROOT + "/gpu-nbody-simulation_amd/csrc/" + name).read()
        assert "nbl_" not in text and "neighbour_lists" not in text and "NblState" not in text, name
