"""Pair counts without a GPU.

  * the numpy twin tests/pairs_ref.py (what tests/test_gpu_pairs.py compares the device with) is held to an independent
    plain-Python version on a few dozen bodies: random, a lattice full of ties on an inclusive edge, coincident bodies,
    edges[0] = 0;
  * correlation_from is the Davis-Peebles formula, NaN where dr = 0;
  * pair_ring_schedule counts every unordered pair of ranks once and its sends meet its receives;
  * header, binding and Python names are there;
  * both pair_count_kernel instantiations meet the resource conditions (hipcc cross-compiles)."""
import dataclasses
import re

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import _lib
from gpu_nbody_simulation_amd import distributed as D
from gpu_nbody_simulation_amd import engine as E
import kernel_meta as KM
import neighbours_ref as NR
import pairs_ref as R


def cases():
    rng = np.random.default_rng(12)
    dup = rng.normal(size=(40, 2))
    dup[10:30] = dup[3]                                           # 21 bodies at one place
    return {"random": rng.normal(size=(48, 2)), "lattice": NR.lattice(6), "duplicates": dup, "two": rng.normal(size=(2, 2)),
            "one": rng.normal(size=(1, 2)), "none": np.zeros((0, 2))}


EDGES = {"ties": [1.0, 2.0, 3.0, 5.0], "from-zero": [0.0, 0.5, 1.0, 1.5, 4.0], "one-bin": [0.25, 2.5],
         "beyond": [1e3, 2e3, 3e3], "fine": list(np.geomspace(0.05, 8.0, 34))}


@pytest.mark.parametrize("name", list(cases()))
@pytest.mark.parametrize("edges", list(EDGES))
def test_twin_equals_plain_python(name, edges):
    pos, ed = cases()[name], EDGES[edges]
    n = len(pos)
    auto = R.pair_counts(pos, ed)
    assert auto.dtype == np.int64 and auto.shape == (len(ed) + 1,)
    assert np.array_equal(auto, R.pair_counts_py(pos, ed)) and auto.sum() == n * (n - 1) // 2
    pts = np.concatenate([np.random.default_rng(13).normal(size=(9, 2)), pos[:4], [[1e6, -1e6]]])   # on bodies too
    cross = R.pair_counts(pos, ed, pts)
    assert np.array_equal(cross, R.pair_counts_py(pos, ed, pts)) and cross.sum() == len(pts) * n
    # the bodies as points: every ordered pair, and every body on itself
    own = R.pair_counts(pos, ed, pos)
    assert np.array_equal(own[1:], 2 * auto[1:]) and own[0] == 2 * auto[0] + n


def test_ties_coincident_bodies_and_a_zero_edge():
    lat = NR.lattice(6)                                           # integer coordinates 0 .. 5 in shuffled order
    got = R.pair_counts(lat, EDGES["ties"])
    d2 = ((lat[:, None, :] - lat[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(len(lat), 1)]
    assert got[0] == (d2 <= 1).sum() and got[1] == ((d2 > 1) & (d2 <= 4)).sum() and got[3] == ((d2 > 9) & (d2 <= 25)).sum()
    assert (d2 == 25).sum() > 0 and got[4] == (d2 > 25).sum()     # d2 = 25 lies on the inclusive edge 5: not beyond
    dup = np.tile([[0.3, -0.7]], (10, 1))
    assert list(R.pair_counts(dup, [0.0, 1.0])) == [45, 0, 0]     # d2 = 0 is "below" even with edges[0] = 0
    assert list(R.pair_counts(dup, [0.0, 1.0], dup[:2])) == [20, 0, 0]


def test_correlation_from_is_davis_peebles():
    dd, dr = np.array([10, 0, 7, 3]), np.array([40, 5, 0, 12])
    xi = G.correlation_from(dd, dr, 21, 50)
    want = [(50 / 20) * (2 * 10 / 40) - 1, (50 / 20) * 0.0 - 1, np.nan, (50 / 20) * (2 * 3 / 12) - 1]
    assert np.array_equal(xi, np.array(want), equal_nan=True) and np.isnan(xi[2])
    assert np.isnan(G.correlation_from([0], [0], 5, 5)[0])
    with pytest.raises(ValueError):
        G.correlation_from([1, 2], [1], 5, 5)
    with pytest.raises(ValueError):
        G.correlation_from([1], [1], 1, 5)


def test_pair_counts_from_fields():
    raw = np.array([3, 1, 0, 4, 2], dtype=np.int64)
    pc = E.pair_counts_from(raw, [0.5, 1.0, 2.0, 4.0], 5, None, 17)
    assert [f.name for f in dataclasses.fields(G.BhPairCounts)] == ["edges", "counts", "below", "beyond", "total", "n_bodies",
                                                                   "n_points", "evals", "cumulative"]
    assert list(pc.counts) == [1, 0, 4] and (pc.below, pc.beyond, pc.total, pc.n_bodies, pc.n_points, pc.evals) == (3, 2, 10, 5, None, 17)
    assert list(pc.cumulative) == [3, 4, 4, 8] and pc.cumulative.dtype == np.int64 and pc.counts.dtype == np.int64
    assert E.pair_counts_from(raw, [0.5, 1.0, 2.0, 4.0], 5, 2).n_points == 2
    with pytest.raises(ValueError):
        E.pair_counts_from(raw, [0.5, 1.0], 5)


@pytest.mark.parametrize("world", range(1, 10))
def test_ring_schedule_counts_every_rank_pair_once(world):
    rounds = D.pair_ring_schedule(world)
    assert len(rounds) == world // 2
    seen = {}
    for k, rnd in enumerate(rounds, start=1):
        assert len(rnd) == world
        for r, (to, frm, counts) in enumerate(rnd):
            assert to == (r + k) % world and frm == (r - k) % world and to != r
            assert rnd[to][1] == r and rnd[frm][0] == r           # what r sends, `to` expects; what r expects, `frm` sends
            if counts:
                pair = frozenset((r, frm))
                seen[pair] = seen.get(pair, 0) + 1
    want = {frozenset((a, b)) for a in range(world) for b in range(a)}
    assert set(seen) == want and all(v == 1 for v in seen.values())
    with pytest.raises(ValueError):
        D.pair_ring_schedule(0)


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_symbols_and_names():
    lib = _lib.load()
    for sym in ("bh_pair_counts", "bh_pair_counts_times"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    for meth in ("pair_counts", "pair_counts_times", "correlation"):
        assert callable(getattr(G.BarnesHutEngine, meth))
    assert callable(D.LetStepper.pair_counts) and callable(D.pair_ring_schedule)
    for name in ("BhPairCounts", "correlation_from"):
        assert name in G.__all__ and hasattr(G, name)
    assert E.PAIR_MAX_BINS == 1024 == R.MAX_BINS
    header = open(KM.ROOT + "/include/bhgpu.h").read()
    assert "BH_PAIR_MAX_BINS 1024" in header
    assert re.search(r"allowed in LET mode and with world > 1", header)
    assert _lib.ABI_VERSION == 4 and lib.bh_abi_version() == 4    # added functions only


# ---- resources ----------------------------------------------------------------------------------------------------------------
def test_both_pair_kernels_meet_the_resource_conditions():
    text = KM.assembly("bh_engine.hip")[0]
    ks = KM.kernels(text, r"_ZN2bh\d+pair_[a-z]+_kernel\S*")
    assert len(ks) == 2 and sum("pair_count_kernel" in k for k in ks) == 2, sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["scratch"] == 0 and r["dynamic_stack"] == "false", (name, r)
        assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
