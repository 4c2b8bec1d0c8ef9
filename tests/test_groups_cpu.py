"""Friends-of-friends groups without a GPU.

  * the numpy twin tests/groups_ref.py (what tests/test_gpu_groups.py compares the device with) is held to an independent
    plain-Python version -- float arithmetic, a breadth-first search from every unvisited body -- on a uniform state, a lattice
    at and just below its spacing, and coincident bodies;
  * the twin's fixed-point catalogue is held to exact rational sums within half a unit per contribution;
  * every kernel of csrc/bh_groups.hpp meets the resource conditions: no scratch, no spills, no dynamic stack;
  * the link kernel reads boxes and leaf bodies through the scalar unit;
  * header, binding and Python names are there."""
import fractions
import re

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
import kernel_meta as KM
import groups_ref as R
import neighbours_ref as NR


def cases():
    rng = np.random.default_rng(3)
    uni = rng.uniform(size=(200, 2))
    dup = rng.normal(size=(120, 2))
    dup[30:70] = dup[5]                                           # 41 bodies at one place
    lat = NR.lattice(12) * 0.25                                   # spacing 0.25: every d2 is exact
    return {"uniform": (uni, 0.05), "uniform-wide": (uni, 0.2), "lattice-at": (lat, 0.25),
            "lattice-below": (lat, float(np.nextafter(0.25, 0.0))), "coincident": (dup, 0.0), "coincident-wide": (dup, 0.3),
            "one": (uni[:1], 0.1), "none": (uni[:0], 0.1)}


@pytest.mark.parametrize("name", list(cases()))
def test_twin_equals_breadth_first_search_in_plain_python(name):
    pos, b = cases()[name]
    label, n_groups, n_pairs = R.groups(pos, b)
    label_py, n_groups_py = R.groups_py(pos, b)
    assert label.dtype == np.int64 and label.shape == (len(pos),)
    assert np.array_equal(label, label_py) and n_groups == n_groups_py
    assert (label <= np.arange(len(pos))).all() and (label[label] == label).all()
    if name == "lattice-at":
        assert n_groups == 1 and n_pairs == 2 * 12 * 11
    if name == "lattice-below":
        assert n_groups == 144 and n_pairs == 0
    if name == "coincident":
        assert n_groups == 120 - 40 and n_pairs == 41 * 40 // 2 and (label[30:70] == 5).all()


def test_fixed_point_catalogue_against_exact_rational_sums():
    rng = np.random.default_rng(9)
    n = 180
    pos = rng.normal(size=(n, 2)) * 3.0
    vel = rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    mass = 10.0 ** rng.uniform(-6, 2, size=n)
    label, n_groups, _ = R.groups(pos, 0.45)
    for min_members in (1, 2, 5):
        ids, counts, sums, e = R.catalogue(pos, vel, mass, label, min_members)
        want = sorted(((int((label == g).sum()), int(g)) for g in np.unique(label) if (label == g).sum() >= min_members),
                      key=lambda t: (-t[0], t[1]))
        assert [(int(c), int(g)) for c, g in zip(counts, ids)] == want
        if min_members == 1:
            assert len(ids) == n_groups and counts.sum() == n
        q = R.moments(pos, vel, mass)
        F = fractions.Fraction
        for g, c, row in zip(ids, counts, sums):
            members = np.nonzero(label == g)[0]
            for p in range(5):
                exact = sum((F(float(q[i, p])) for i in members), F(0)) * F(2) ** int(e[p])
                assert abs(F(int(row[p])) - exact) <= F(len(members), 2), (g, p)
        # no plane can overflow: |sum| <= n * 2^(62 - L) <= 2^62
        assert (np.abs(sums) <= 2 ** 62).all()
    # the exponents: max |q_p| * 2^e_p * 2^L in [2^61, 2^62)
    L = (n - 1).bit_length()
    for p in range(5):
        top = np.abs(q[:, p]).max() * 2.0 ** (int(e[p]) + L)
        assert 2.0 ** 61 <= top < 2.0 ** 62


def test_spiral_fixture_is_what_it_says():
    b = 0.125
    pos, place = R.spiral(2000, b)
    along = pos[np.argsort(place)]
    chord = np.hypot(*(along[1:] - along[:-1]).T)
    assert chord.max() <= 0.9 * b and chord.min() >= 0.89 * b
    # nobody but the two neighbours along the arm within 3 b ... of a sample of bodies
    for k in (0, 1, 700, 1999):
        d = np.hypot(*(along - along[k]).T)
        near = np.nonzero(d < 3.0 * b)[0]
        assert set(near) <= set(range(k - 3, k + 4)), (k, near)
    label, n_groups, n_pairs = R.groups(pos, b)
    assert n_groups == 1 and (label == 0).all() and n_pairs == 1999
    pos, place = R.spiral(2000, b, gap=1200)
    label, n_groups, _ = R.groups(pos, b)
    assert n_groups == 2 and len(pos) == 1999
    assert np.array_equal(label == label[np.argmin(place)], place < 1200)


# ---- resources ------------------------------------------------------------------------------------------------------------------
def test_every_groups_kernel_meets_the_resource_conditions():
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+grp_[a-z]+_kernel\S*")
    names = sorted(ks)
    for stem, count in (("grp_init_kernel", 1), ("grp_link_kernel", 1), ("grp_flatten_kernel", 1), ("grp_label_kernel", 1),
                        ("grp_compact_kernel", 1), ("grp_max_kernel", 2), ("grp_sum_kernel", 2)):
        assert sum(stem in k for k in ks) == count, (stem, names)
    assert len(ks) == 9, names
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


def test_the_link_kernel_loads_boxes_and_leaf_bodies_through_the_scalar_unit():
    """The count of test_neighbours_cpu.py for the search kernels: what is left of vector loads is the lane's own body -- and
    here the words of parent[], every one of them an agent-scope (sc1) load of one dword; boxes, level offsets and leaf bodies
    come at wave-uniform addresses (an NbBox as two 16-byte loads or one of 32, a leaf body as one of 16)."""
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+grp_link_kernel\S*")
    assert len(ks) == 1
    for name in ks:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert body.count("flat_load") == 0 and body.count("buffer_load") == 0
        loads = re.findall(r"global_load_\w+ .*", body)
        parent = [l for l in loads if l.startswith("global_load_dword ") and l.rstrip().endswith("sc1")]
        print(name, len(loads), len(parent), body.count("s_load_dwordx4"), body.count("s_load_dwordx8"))
        assert len(loads) - len(parent) <= 3, loads
        assert parent, loads
        assert body.count("s_load_dwordx4") + 2 * body.count("s_load_dwordx8") >= 3, name
        # every write to parent[] is an atomic: no vector store in the kernel at all (the counters are atomics too)
        assert body.count("global_store") == 0 and body.count("flat_store") == 0, name


def test_the_walk_unit_does_not_see_the_groups():
    src = open(KM.CSRC + "/bh_walk_fast.hip").read() + open(KM.CSRC + "/bh_walk_fast.h").read()
    assert "bh_groups" not in src and "bh_neighbours" not in src


# ---- the interface --------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    for sym in ("bh_groups", "bh_groups_catalogue", "bh_groups_times"):
        assert sym in _lib.SIGNATURES and hasattr(_lib.load(), sym)
    for meth in ("groups", "groups_times"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    assert "BhGroups" in G.__all__ and callable(G.BhGroups.members)
    head = open(KM.ROOT + "/include/bhgpu.h").read()
    assert "BHGPU_ABI_VERSION 4 " in head and "int bh_groups(" in head
