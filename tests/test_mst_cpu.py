"""Minimum spanning trees and the mass segregation ratio without a GPU.

  * the numpy twin tests/mst_ref.py (what tests/test_gpu_mst.py compares the device with) is held to an independent plain-Python
    Kruskal -- float arithmetic, every pair, `sorted` on (d2, lo, hi) tuples -- on a uniform state, a lattice on which every d2 is
    tied, coincident bodies and n = 0, 1, 2;
  * the tree is the friends-of-friends clustering at every linking length: labels_at(b) of the twin's tree and
    BhSpanningTree.groups_at(b) equal tests/groups_ref.py's labels, the number of groups is n minus the edges with d2 <= b^2;
  * mass_segregation_from: about 1 without segregation, above 1 with the massive bodies at the centre;
  * every kernel of csrc/bh_mst.hpp meets the resource conditions: no scratch, no spills, no dynamic stack, <= 64 VGPRs;
  * the nearest kernel reads boxes, node components and leaf bodies through the scalar unit;
  * header, binding and Python names are there."""
import math
import re

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
import groups_ref as R
import kernel_meta as KM
import mst_ref as M
import neighbours_ref as NR

LENGTHS = (0.0, 0.05, 0.25, float(np.nextafter(0.25, 0.0)), 0.3, 5.0)


def cases():
    rng = np.random.default_rng(3)
    uni = rng.uniform(size=(200, 2))
    dup = rng.normal(size=(120, 2))
    dup[30:70] = dup[5]                                           # 41 bodies at one place
    lat = NR.lattice(10) * 0.25                                   # spacing 0.25: every d2 is exact, every edge of the tree tied
    return {"uniform": uni, "lattice": lat, "coincident": dup, "none": uni[:0], "one": uni[:1], "two": uni[:2]}


@pytest.mark.parametrize("name", list(cases()))
def test_twin_equals_kruskal_in_plain_python(name):
    pos = cases()[name]
    n = len(pos)
    lo, hi, d2 = M.tree(pos)
    klo, khi, kd2 = M.kruskal_py(pos)
    assert lo.dtype == np.int64 and hi.dtype == np.int64 and lo.shape == hi.shape == d2.shape == (max(n - 1, 0),)
    assert np.array_equal(lo, klo) and np.array_equal(hi, khi) and np.array_equal(d2, kd2)
    assert (lo < hi).all()
    keys = list(zip(d2.tolist(), lo.tolist(), hi.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)   # strictly ascending in the edge order
    if name == "lattice":
        assert (d2 == 0.0625).all()
    if name == "coincident":
        # the zero-length edges are the star on the lowest index of the 41 coincident bodies
        zero = d2 == 0.0
        assert zero.sum() == 40 and (lo[zero] == 5).all() and list(hi[zero]) == list(range(30, 70)) and zero[:40].all()


@pytest.mark.parametrize("name", ["uniform", "lattice", "coincident", "one", "none"])
def test_the_tree_holds_the_groups_of_every_linking_length(name):
    pos = cases()[name]
    n = len(pos)
    lo, hi, d2 = M.tree(pos)
    t = G.spanning_tree_from(lo, hi, d2, n)
    assert t.n == n and np.array_equal(t.length, np.sqrt(d2)) and t.total_length == math.fsum(np.sqrt(d2).tolist())
    counts = t.n_groups_at(LENGTHS)
    assert counts.shape == (len(LENGTHS),)
    for k, b in enumerate(LENGTHS):
        label, n_groups, _ = R.groups(pos, b)
        got, got_groups = M.labels_at(n, lo, hi, d2, b)
        assert np.array_equal(got, label) and got_groups == n_groups, (name, b)
        assert n_groups == n - int((d2 <= b * b).sum()) == counts[k] == t.n_groups_at(b), (name, b)
        at = t.groups_at(b)
        assert at.dtype == np.int64 and np.array_equal(at, label), (name, b)
    if name == "lattice":
        assert list(counts) == [100, 100, 1, 100, 1, 1]
    with pytest.raises(ValueError):
        t.groups_at(-1.0)
    with pytest.raises(ValueError):
        t.n_groups_at([0.1, float("nan")])


def test_subset_trees_of_the_twin_are_trees_of_the_rows_alone():
    rng = np.random.default_rng(8)
    pos = rng.normal(size=(60, 2))
    members = np.stack([rng.choice(60, 7, replace=False) for _ in range(5)])
    lo, hi, d2 = M.subset_trees(pos, members)
    for r in range(5):
        row = np.sort(members[r])
        klo, khi, kd2 = M.kruskal_py(pos[row])
        order = np.lexsort((row[khi], row[klo], kd2))            # (Kruskal's order is by place in the row: re-sort by caller index)
        assert np.array_equal(lo[r], row[klo][order]) and np.array_equal(hi[r], row[khi][order]) and np.array_equal(d2[r], kd2[order])


def test_mass_segregation_is_about_one_without_and_above_one_with_segregation():
    rng = np.random.default_rng(12)
    n, k, R_ = 400, 12, 60
    pos = rng.normal(size=(n, 2))
    mass = rng.uniform(0.5, 2.0, size=n)
    ratio, sigma, l_massive, l_random, members = M.mass_segregation(pos, mass, k, R_, seed=4)
    got = G.mass_segregation_from(M.subset_trees(pos, members)[2], members)
    assert (got.ratio, got.sigma, got.l_massive) == (ratio, sigma, l_massive) and np.array_equal(got.l_random, l_random)
    assert got.n_massive == k and got.members.shape == (R_ + 1, k) and sigma > 0.0
    assert list(members[0]) == sorted(range(n), key=lambda i: (-mass[i], i))[:k]
    assert np.array_equal(members[3], np.random.default_rng([4, 2]).choice(n, k, replace=False))
    print("no segregation:", ratio, sigma)
    assert abs(ratio - 1.0) <= 3.0 * sigma
    # the k largest masses go to the k bodies nearest the centre
    seg = mass.copy()
    inner = np.argsort(np.hypot(pos[:, 0], pos[:, 1]))[:k]
    seg[inner] = 10.0 + np.arange(k)
    ratio, sigma, _, _, members = M.mass_segregation(pos, seg, k, R_, seed=4)
    print("segregated:", ratio, sigma)
    assert set(members[0]) == set(inner) and ratio - 3.0 * sigma > 1.0
    # ties go to the smaller index
    assert list(M.segregation_sets(np.ones(30), 4, 1, 0)[0]) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        G.mass_segregation_from(np.zeros((1, 3)), np.zeros((1, 4), dtype=np.int64))


# ---- resources ------------------------------------------------------------------------------------------------------------------
KERNELS = (("mst_init_kernel", 1), ("mst_nodecomp_kernel", 1), ("mst_seed_kernel", 1), ("mst_nearest_kernel", 1), ("mst_pick_kernel", 1),
           ("mst_hook_kernel", 1), ("mst_flatten_kernel", 1), ("mst_iota_kernel", 1), ("mst_gather_kernel", 1), ("mst_subset_kernel", 2))


def test_every_spanning_tree_kernel_meets_the_resource_conditions():
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+mst_[a-z]+_kernel\S*")
    names = sorted(ks)
    for stem, count in KERNELS:
        assert sum(stem in k for k in ks) == count, (stem, names)
    assert len(ks) == sum(c for _, c in KERNELS) == 11, names
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


def test_the_nearest_kernel_loads_boxes_and_leaf_bodies_through_the_scalar_unit():
    """The count of test_groups_cpu.py for the link kernel.  What is left of vector loads: the lane's own body (position,
    component, caller index), its seed (d2 and pair) and its component's smallest seed.  Boxes, level offsets, node components and
    the leaf bodies with their comp / sidx come at wave-uniform addresses (an NbBox as two 16-byte loads or one of 32, a leaf
    body as one of 16)."""
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+mst_nearest_kernel\S*")
    assert len(ks) == 1
    for name in ks:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert body.count("flat_load") == 0 and body.count("buffer_load") == 0
        loads = re.findall(r"global_load_\w+ .*", body)
        print(name, len(loads), body.count("s_load_dwordx4"), body.count("s_load_dwordx8"), body.count("s_load_dword "))
        assert len(loads) <= 6, loads
        assert body.count("s_load_dwordx4") + 2 * body.count("s_load_dwordx8") >= 3, name
        assert body.count("s_load_dword ") >= 3, name              # (the level offset, the node's component, a leaf body's two words)


def test_the_walk_unit_does_not_see_the_spanning_trees():
    src = open(KM.CSRC + "/bh_walk_fast.hip").read() + open(KM.CSRC + "/bh_walk_fast.h").read()
    assert "bh_mst" not in src


# ---- the interface --------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    for sym in ("bh_spanning_tree", "bh_spanning_tree_subsets", "bh_spanning_tree_times"):
        assert sym in _lib.SIGNATURES and hasattr(_lib.load(), sym)
    assert [len(_lib.SIGNATURES[s][1]) for s in ("bh_spanning_tree", "bh_spanning_tree_subsets", "bh_spanning_tree_times")] == [5, 7, 4]
    for meth in ("spanning_tree", "spanning_tree_times", "subset_spanning_trees", "mass_segregation"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    for name in ("BhSpanningTree", "BhMassSegregation", "mass_segregation_from"):
        assert name in G.__all__ and hasattr(G, name)
    assert callable(G.BhSpanningTree.groups_at) and callable(G.BhSpanningTree.n_groups_at)
    head = open(KM.ROOT + "/include/bhgpu.h").read()
    assert "BHGPU_ABI_VERSION 4 " in head and "int bh_spanning_tree(" in head and "int bh_spanning_tree_subsets(" in head
    assert "#define BH_MST_SUBSET_MAX 512" in head
    from gpu_nbody_simulation_amd import engine
    assert engine.MST_SUBSET_MAX == 512
