"""Bound pairs without a GPU.

  * the numpy twin tests/binaries_ref.py (what tests/test_gpu_binaries.py compares the device with) is held to an independent
    plain-Python double loop -- float arithmetic, math.sqrt, every pair, `sorted` on (eps, j) tuples -- on a uniform state, a state
    with coincident bodies and n = 0, 1, 2;
  * kepler_pair gives back the a, e and period it was made with, at every phase;
  * the planted pairs of cluster() that are well isolated are all found;
  * every kernel of csrc/bh_binaries.hpp meets the resource conditions: no scratch, no spills, no dynamic stack, <= 64 VGPRs;
  * the search kernel reads boxes, mass bounds and leaf bodies through the scalar unit;
  * header, binding and Python names are there."""
import math
import re

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
import binaries_ref as B
import kernel_meta as KM


def cases():
    rng = np.random.default_rng(17)
    n = 150
    uni = (rng.uniform(size=(n, 2)), rng.normal(size=(n, 2)) * 0.3, rng.uniform(0.5, 1.5, size=n) / n)
    dup_pos = rng.normal(size=(90, 2))
    dup_pos[20:40] = dup_pos[3]                                   # 21 bodies at one place
    dup = (dup_pos, rng.normal(size=(90, 2)) * 0.2, rng.uniform(0.5, 1.5, size=90) / 30)
    cut = lambda s, k: tuple(a[:k] for a in s)
    return {"uniform": uni, "coincident": dup, "none": cut(uni, 0), "one": cut(uni, 1), "two": cut(uni, 2)}


@pytest.mark.parametrize("R", [0.2, float("inf")])
@pytest.mark.parametrize("name", list(cases()))
def test_twin_equals_the_double_loop_in_plain_python(name, R):
    pos, vel, mass = cases()[name]
    n = len(pos)
    partner, eps, lo, hi, rec = B.catalogue(pos, vel, mass, 1.0, R)
    ppy, epy = B.partners_py(pos, vel, mass, 1.0, R)
    assert partner.dtype == np.int64 and partner.shape == eps.shape == (n,) and rec.shape == (len(lo), 11)
    assert np.array_equal(partner, ppy) and np.array_equal(eps, epy)
    lpy, hpy = B.mutual_py(ppy)
    assert np.array_equal(lo, lpy) and np.array_equal(hi, hpy) and (lo < hi).all() and (np.diff(lo) > 0).all()
    assert ((partner == -1) == np.isinf(eps)).all() and (eps[partner >= 0] < 0.0).all()
    if name == "uniform":
        assert (partner >= 0).sum() > n // 2 and len(lo) > 10     # (the case is not empty)
        assert np.array_equal(rec[:, 1], eps[lo]) and np.array_equal(rec[:, 1], eps[hi])          # eps_ij and eps_ji: the same bits
        assert (rec[:, 5] > 0.0).all() and (rec[:, 2] > 0.0).all() and (rec[:, 3] < 1.0).all()
    if name == "coincident":
        same = np.arange(20, 40)
        assert not np.isin(partner[same], np.concatenate([same, [3]])).any() and partner[3] not in same
    if n < 2:
        assert len(lo) == 0 and (partner == -1).all()


def test_elements_in_plain_python_floats():
    """the eleven columns of a record against the formulas of include/bhgpu.h written out with Python floats"""
    pos, vel, mass = cases()["uniform"]
    _, _, lo, hi, rec = B.catalogue(pos, vel, mass, 1.0, 0.2)
    P, V, M_ = pos.tolist(), vel.tolist(), mass.tolist()
    for k, (i, j) in enumerate(zip(lo.tolist(), hi.tolist())):
        dx, dy = P[j][0] - P[i][0], P[j][1] - P[i][1]
        d2 = dx * dx + dy * dy
        ux, uy = V[j][0] - V[i][0], V[j][1] - V[i][1]
        v2 = ux * ux + uy * uy
        M = M_[i] + M_[j]
        mu = 1.0 * M
        r = math.sqrt(d2)
        eps = 0.5 * v2 - mu / r
        a = mu / (-2.0 * eps)
        h = dx * uy - dy * ux
        e = math.sqrt(max(1.0 + ((2.0 * eps) * (h * h)) / (mu * mu), 0.0))
        want = [r, eps, a, e, 6.283185307179586 * math.sqrt(((a * a) * a) / mu), -(((M_[i] * M_[j]) / M) * eps), M,
                (M_[i] * P[i][0] + M_[j] * P[j][0]) / M, (M_[i] * P[i][1] + M_[j] * P[j][1]) / M,
                (M_[i] * V[i][0] + M_[j] * V[j][0]) / M, (M_[i] * V[i][1] + M_[j] * V[j][1]) / M]
        assert rec[k].tolist() == want, (k, i, j)


KEPLER = [(1.0, 1.0, 1.0, 0.1), (3.0, 0.5, 2.5, 0.7), (1e-3, 2e-3, 1e-4, 0.3), (1.0, 1e-6, 7.0, 0.5)]
# At phase 0 the twin's a and period are within 2.5e-15 (relative) of the closed form and e within 5.2e-16 on these four orbits
# (eps is a difference of two terms up to 2 / (1 - e) times larger: a few units of 1.1e-16 each, times that factor); 1e-13 leaves
# a factor of forty.
KEPLER_TOL = 1e-13


@pytest.mark.parametrize("m1,m2,a,e", KEPLER)
def test_kepler_pair_returns_its_elements_at_every_phase(m1, m2, a, e):
    T = B.kepler_period(m1, m2, a)
    for phase in (0.0, 0.7, 2.0, math.pi, 4.5, 6.0):
        mass, pos, vel = B.kepler_pair(m1, m2, a, e, phase)
        partner, eps, lo, hi, rec = B.catalogue(pos, vel, mass, 1.0, float("inf"))
        assert list(partner) == [1, 0] and list(lo) == [0] and list(hi) == [1]
        r, en, ga, ge, gT, bind, M = rec[0, :7]
        print(phase, abs(ga / a - 1.0), abs(ge - e), abs(gT / T - 1.0))
        assert abs(ga / a - 1.0) <= KEPLER_TOL and abs(ge - e) <= KEPLER_TOL and abs(gT / T - 1.0) <= KEPLER_TOL
        assert a * (1.0 - e) * (1.0 - 1e-12) <= r <= a * (1.0 + e) * (1.0 + 1e-12)
        assert M == m1 + m2 and bind > 0.0 and abs(bind / (m1 * m2 / (2.0 * a)) - 1.0) <= KEPLER_TOL
        assert np.abs(rec[0, 7:]).max() <= 1e-15 * max(a, math.sqrt(M / a))          # the centre of mass rests at the origin
    # other units: G scales eps, and a, e stay
    mass, pos, vel = B.kepler_pair(m1, m2, a, e, 1.0, G=6.67e-11)
    rec = B.catalogue(pos, vel, mass, 6.67e-11, float("inf"))[4]
    assert abs(rec[0, 2] / a - 1.0) <= KEPLER_TOL and abs(rec[0, 3] - e) <= KEPLER_TOL


CLUSTER_SEED = 2


def test_isolated_planted_pairs_of_the_cluster_are_found():
    mass, pos, vel, planted = B.cluster(2000, 100, CLUSTER_SEED)
    assert planted.shape == (100, 4) and len(np.unique(planted[:, :2])) == 200
    _, _, lo, hi, rec = B.catalogue(pos, vel, mass, 1.0, 0.05)
    found = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(lo, hi))}
    isolated = 0
    for i, j, a, e in planted:
        i, j = int(i), int(j)
        near = np.inf
        for b in (i, j):
            d = np.hypot(pos[:, 0] - pos[b, 0], pos[:, 1] - pos[b, 1])
            d[[i, j]] = np.inf
            near = min(near, float(d.min()))
        if a * (1.0 + e) < 0.1 * near:                            # the apocentre against the nearest third body
            isolated += 1
            k = found.get((min(i, j), max(i, j)))
            assert k is not None, (i, j, a, e, near)
            assert abs(rec[k, 2] / a - 1.0) <= 1e-6 and abs(rec[k, 3] - e) <= 1e-6       # (the cluster's positions are near 1: 1e-16 / a)
    print("isolated", isolated, "of 100; catalogue", len(lo))
    assert isolated >= 90


# ---- resources ------------------------------------------------------------------------------------------------------------------
KERNELS = (("bin_gather_kernel", 2), ("bin_nodemass_kernel", 1), ("bin_search_kernel", 1), ("bin_pairs_kernel", 1))


def test_every_binaries_kernel_meets_the_resource_conditions():
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+bin_[a-z]+_kernel\S*")
    names = sorted(ks)
    for stem, count in KERNELS:
        assert sum(stem in k for k in ks) == count, (stem, names)
    assert len(ks) == sum(c for _, c in KERNELS) == 5, names
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)


def test_the_search_kernel_loads_boxes_mass_bounds_and_leaf_bodies_through_the_scalar_unit():
    """The count of test_mst_cpu.py for the nearest kernel.  What is left of vector loads: the lane's own body (position,
    velocity, mass, caller index) and its seeds (position, velocity, mass, caller index).  Boxes, level offsets, mass bounds and
    the leaf bodies with their velocity, mass and caller index come at wave-uniform addresses (an NbBox as two 16-byte loads or
    one of 32, a leaf body's position and velocity as one of 16 each, a mass bound or a mass as one of 8)."""
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+bin_search_kernel\S*")
    assert len(ks) == 1
    for name in ks:
        body = text[text.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert body.count("flat_load") == 0 and body.count("buffer_load") == 0
        loads = re.findall(r"global_load_\w+ .*", body)
        print(name, len(loads), body.count("s_load_dwordx4"), body.count("s_load_dwordx8"), body.count("s_load_dwordx2"),
              body.count("s_load_dword "))
        assert len(loads) <= 8, loads
        assert body.count("s_load_dwordx4") + 2 * body.count("s_load_dwordx8") >= 4, name      # a box, a leaf body's position and velocity
        assert body.count("s_load_dwordx2") >= 2, name             # the node's mass bound, a leaf body's mass
        assert body.count("s_load_dword ") >= 2, name              # the level offset, a leaf body's caller index


def test_the_walk_unit_does_not_see_the_binaries():
    src = open(KM.CSRC + "/bh_walk_fast.hip").read() + open(KM.CSRC + "/bh_walk_fast.h").read()
    assert "bh_binaries" not in src


# ---- the interface --------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    names = ("bh_binaries", "bh_binaries_catalogue", "bh_binaries_times")
    for sym in names:
        assert sym in _lib.SIGNATURES and hasattr(_lib.load(), sym)
    assert [len(_lib.SIGNATURES[s][1]) for s in names] == [6, 5, 4]
    for meth in ("binaries", "binaries_times"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    assert "BhBinaries" in G.__all__ and hasattr(G, "BhBinaries")
    head = open(KM.ROOT + "/include/bhgpu.h").read()
    assert "BHGPU_ABI_VERSION 4 " in head and _lib.ABI_VERSION == 4
    assert "int bh_binaries(bh_ctx *ctx, double max_separation, int64_t *partner, double *eps, int64_t *n_pairs, uint64_t stats[4]);" in head
    assert "int bh_binaries_catalogue(bh_ctx *ctx, int64_t max_records, int64_t *lo, int64_t *hi, double *records" in head
    assert "int bh_binaries_times(bh_ctx *ctx, double *build_ms, double *search_ms, double *catalogue_ms);" in head
    engine_unit = open(KM.CSRC + "/bh_engine.hip").read()
    assert engine_unit.index('#include "bh_neighbours.hpp"') < engine_unit.index('#include "bh_binaries.hpp"')


def test_bhbinaries_of_the_twin():
    mass, pos, vel, _ = B.cluster(300, 20, 5)
    partner, eps, lo, hi, rec = B.catalogue(pos, vel, mass, 1.0, 0.05)
    b = G.binaries_from_records(partner, eps, lo, hi, rec, 0.05, mean_kinetic=2.0)
    assert b.n == 300 and len(b.lo) == len(lo) >= 20 and b.fraction == 2.0 * len(lo) / 300
    assert b.total_binding_energy == math.fsum(rec[:, 5].tolist())
    assert np.array_equal(b.hardness(), rec[:, 5] / 2.0) and np.array_equal(b.hardness(0.5), rec[:, 5] / 0.5)
    assert np.array_equal(b.separation, rec[:, 0]) and np.array_equal(b.energy, rec[:, 1]) and np.array_equal(b.period, rec[:, 4])
    assert np.array_equal(b.mass, rec[:, 6]) and np.array_equal(b.com, rec[:, 7:9]) and np.array_equal(b.velocity, rec[:, 9:11])
    w = b.within(3e-4)
    keep = rec[:, 2] <= 3e-4
    assert 20 <= keep.sum() < len(lo) and np.array_equal(w.lo, lo[keep]) and np.array_equal(w.com, rec[keep, 7:9])
    assert w.n == 300 and np.array_equal(w.partner, partner) and w.fraction == 2.0 * keep.sum() / 300
    with pytest.raises(ValueError):
        G.binaries_from_records(partner, eps, lo, hi, rec, 0.05).hardness()
