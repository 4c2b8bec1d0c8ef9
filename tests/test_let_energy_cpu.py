"""CPU checks of the distributed step's diagnostics (bh_let_potential, bh_let_get_potential, bh_let_energy;
distributed.LetStepper.potential / energy): the interface, the tests' own forest reference
(tests/forest_potential_ref.py), the host glue of LetStepper over gloo with a numpy stand-in engine, and the resources
of the forest potential kernel."""
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import bh_oracle as O  # noqa: E402
from gpu_nbody_simulation_amd import _lib  # noqa: E402
from gpu_nbody_simulation_amd.distributed import partition_orb  # noqa: E402
import forest_potential_ref as FP  # noqa: E402
import kernel_meta as KM  # noqa: E402
from potential_ref import potential_walk  # noqa: E402

HEADER = os.path.join(ROOT, "include", "bhgpu.h")
NEW = ("bh_let_potential", "bh_let_get_potential", "bh_let_energy", "bh_let_bounds_quiet", "bh_let_build_quiet")
FIELDS = ("kinetic", "potential", "total", "px", "py", "angular_momentum", "comx", "comy", "mass", "n_bodies")


def test_the_entry_points_are_declared_exported_and_bound():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 4 and lib.bh_abi_version() == 4          # added functions only
    from gpu_nbody_simulation_amd.distributed import LetStepper
    from gpu_nbody_simulation_amd.engine import BarnesHutEngine
    assert callable(LetStepper.potential) and callable(LetStepper.energy)
    assert callable(BarnesHutEngine.let_potential) and callable(BarnesHutEngine.let_energy_sums)


# ---- the forest reference -------------------------------------------------------------------------------------------
def _bodies(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.5, n), rng.uniform(-1.0, 1.0, (n, 2))


def round_robin(p, w):
    return [np.arange(r, len(p), w) for r in range(w)]


def with_an_empty_rank(p, w):
    parts = partition_orb(p, w - 1)
    return parts[:1] + [np.zeros(0, dtype=np.int64)] + parts[1:]


def test_reference_with_one_rank_is_the_single_tree_walk():
    m, p = _bodies(3000, 3)
    for theta in (0.5, 0.9):
        phi, cnt = FP.forest_potential(m, p, [np.arange(len(m))], theta=theta, G=1.0)
        ref, rc = potential_walk(O.build_tree(p, m, 0), p, theta=theta, G=1.0, compat=False)
        assert np.array_equal(phi, ref) and np.array_equal(cnt, rc)


@pytest.mark.parametrize("partition", [partition_orb, round_robin, with_an_empty_rank], ids=["orb", "round_robin", "empty_rank"])
def test_reference_equals_the_direct_sum_when_every_cell_is_opened(partition):
    """theta 1e-6: every body meets every other as a single-body leaf, of its own tree or of a peer's."""
    n, G = 512, 1.0
    m, p = _bodies(n, 7)
    parts = partition(p, 3)
    assert sorted(np.concatenate(parts).tolist()) == list(range(n))
    if partition is with_an_empty_rank:
        assert min(len(ix) for ix in parts) == 0
    phi, cnt = FP.forest_potential(m, p, parts, theta=1e-6, G=G)
    assert np.array_equal(cnt, np.full(n, n - 1))
    for i in range(n):
        d = np.sqrt(((p - p[i]) ** 2).sum(axis=1)) + 1e-15
        ref = -G * math.fsum(np.delete(m / d, i))
        assert abs(phi[i] - ref) <= 1e-12 * abs(ref), (i, phi[i], ref)


def test_reference_counts_are_the_forest_oracles():
    """The potential reference takes the nodes the forest force oracle takes (tests/forest_ref.forest_diag, uncapped)."""
    import forest_ref as FR
    m, p = _bodies(2500, 11)
    parts = partition_orb(p, 3)
    _, cnt = FP.forest_potential(m, p, parts, theta=0.5)
    d = FR.forest_diag(m, p, parts, 0.5, cap_depth=0)
    assert np.array_equal(cnt, d.counts.astype(np.int64))


# ---- LetStepper.energy() / potential() over gloo ---------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs(n, seed=7):
    rng = np.random.default_rng(seed)
    return ((10.0 ** rng.uniform(-2, 1, n)).astype(np.float32), rng.uniform(-0.1, 0.1, (n, 2)).astype(np.float32),
            rng.uniform(-1e-2, 1e-2, (n, 2)).astype(np.float32))


def _partition(p, world, empty):
    if not empty:
        return partition_orb(p, world)
    parts = partition_orb(p, world - 1)
    return parts[:1] + [np.zeros(0, dtype=np.int64)] + parts[1:]


def _stand_in():
    from dist_standin import LetStandInEngine

    class LetEnergyStandIn(LetStandInEngine):
        """LetStandInEngine with the diagnostics surface in numpy: the potential is the direct sum over the own bodies
        and the bodies the peers' blocks carry, the eight sums are plain fp64 numpy sums of the rank's state."""
        quiet_calls = 0

        def let_bounds(self, quiet=False):
            type(self).quiet_calls += int(quiet)
            super().let_bounds()

        def let_build(self, quiet=False):
            type(self).quiet_calls += int(quiet)
            super().let_build()

        def let_potential(self, with_counts=False):
            nb = self.let_cap * self.QUAD_BYTES
            recv = self.recv.numpy()
            ps, ms = [self.pos], [self.mass]
            for r in range(self.world):
                if r == self.rank:
                    continue
                blk = recv[r * nb:(r + 1) * nb]
                sender, dest, cnt = blk[:12].view(np.int32)
                assert (sender, dest) == (r, self.rank)
                rec = blk[12:12 + 12 * cnt].view(np.float32).reshape(cnt, 3)
                ps.append(rec[:, :2])
                ms.append(rec[:, 2])
            p, m = np.concatenate(ps).astype(np.float64), np.concatenate(ms).astype(np.float64)
            self.phi = FP.direct_potential(m, p, G=self.G)[:self.n]
            cnt = np.full(self.n, len(m) - 1, dtype=np.uint32)
            return (self.phi, cnt) if with_counts else self.phi

        def let_energy_sums(self):
            phi = self.let_potential()
            m, p, v = self.mass.astype(np.float64), self.pos.astype(np.float64), self.vel.astype(np.float64)
            t = [m, m * p[:, 0], m * p[:, 1], m * v[:, 0], m * v[:, 1], m * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0]),
                 m * (v[:, 0] ** 2 + v[:, 1] ** 2), m * phi]
            return np.array([x.sum() for x in t])

    return LetEnergyStandIn


def _energy_worker(rank, world, port, n, empty, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_nbody_simulation_amd.distributed import LetStepper
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m, p, v = _inputs(n)
    mine = _partition(p, world, empty)[rank]
    cls = _stand_in()
    eng = cls(G=1.0, dt=1e-3)
    eng.upload(p[mine], v[mine], m[mine])
    st = LetStepper(eng, rank, world, let_cap=64, device=torch.device("cpu"), ids=mine)
    st.step()
    e = st.energy()
    assert cls.quiet_calls == 2                              # the diagnostic's bounds and build were the quiet ones
    phi, cnt = st.potential(with_counts=True)
    e2 = st.energy()
    pos, vel = eng.download()
    row = [e.kinetic, e.potential, e.total, *e.momentum, e.angular_momentum, *e.com, e.mass, float(e.n_bodies)]
    row2 = [e2.kinetic, e2.potential, e2.total, *e2.momentum, e2.angular_momentum, *e2.com, e2.mass, float(e2.n_bodies)]
    np.savez(os.path.join(out_dir, f"energy{rank}.npz"), row=np.array(row), row2=np.array(row2), pos=pos, vel=vel,
             mass=eng.masses(), phi=phi, cnt=cnt, ids=st.ids)
    # an outgrown let_cap makes the diagnostic raise, on every rank together
    eng.overflow_override = True
    raised = False
    try:
        st.energy()
    except RuntimeError:
        raised = True
    assert raised
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n,empty", [(2, 300, False), (3, 200, False), (3, 200, True)])
def test_let_stepper_energy_is_the_fsum_of_the_gathered_state_on_every_rank(tmp_path, world, n, empty):
    mp.spawn(_energy_worker, args=(world, _free_port(), n, empty, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(tmp_path / f"energy{k}.npz") for k in range(world)]
    if empty:
        assert min(len(x["ids"]) for x in r) == 0
    for x in r[1:]:                                           # every rank: the same bits, and again on the second call
        assert np.array_equal(x["row"], r[0]["row"])
    for x in r:
        assert np.array_equal(x["row2"], x["row"])
    ids = np.concatenate([x["ids"] for x in r])
    assert sorted(ids.tolist()) == list(range(n))
    m = np.concatenate([x["mass"] for x in r])
    p, v = np.concatenate([x["pos"] for x in r]), np.concatenate([x["vel"] for x in r])
    phi = np.concatenate([x["phi"] for x in r])
    assert all((x["cnt"] == n - 1).all() for x in r)
    # the stand-in's potential is the direct sum over everything that reached the rank: the whole system
    order = np.argsort(ids)
    ref_phi = FP.direct_potential(m[order], p[order], G=1.0)
    assert np.allclose(phi[order], ref_phi, rtol=1e-12, atol=0)
    terms = [m, m * p[:, 0], m * p[:, 1], m * v[:, 0], m * v[:, 1], m * (p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0]),
             m * (v[:, 0] ** 2 + v[:, 1] ** 2), m * phi]
    S = [math.fsum(t) for t in terms]
    A = [math.fsum(np.abs(t)) for t in terms]
    e = dict(zip(FIELDS, r[0]["row"]))
    bound = lambda k: 1e-13 * A[k]
    assert abs(e["mass"] - S[0]) <= bound(0)
    assert abs(e["px"] - S[3]) <= bound(3) and abs(e["py"] - S[4]) <= bound(4)
    assert abs(e["angular_momentum"] - S[5]) <= bound(5)
    assert abs(e["kinetic"] - 0.5 * S[6]) <= 0.5 * bound(6)
    assert abs(e["potential"] - 0.5 * S[7]) <= 0.5 * bound(7)
    assert e["total"] == e["kinetic"] + e["potential"]
    assert abs(e["comx"] - S[1] / S[0]) <= (bound(1) + abs(S[1] / S[0]) * bound(0)) / S[0] + 1e-16 * abs(S[1] / S[0])
    assert abs(e["comy"] - S[2] / S[0]) <= (bound(2) + abs(S[2] / S[0]) * bound(0)) / S[0] + 1e-16 * abs(S[2] / S[0])
    assert int(e["n_bodies"]) == n


def test_world_one_energy_needs_no_process_group():
    from gpu_nbody_simulation_amd.distributed import LetStepper
    m, p, v = _inputs(64)
    eng = _stand_in()(G=1.0)
    eng.upload(p, v, m)
    st = LetStepper(eng, 0, 1, let_cap=64, device=torch.device("cpu"))
    e = st.energy()
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    assert e.n_bodies == 64 and abs(e.mass - math.fsum(m64)) <= 1e-13 * e.mass
    assert abs(e.kinetic - 0.5 * math.fsum(m64 * (v64 ** 2).sum(axis=1))) <= 1e-13 * e.kinetic
    assert e.potential < 0.0


# ---- kernel resources ----------------------------------------------------------------------------------------------
def test_forest_potential_kernel_compiles_for_gfx950_without_scratch_or_spills():
    """The standard tests/test_field_cpu.py holds the side walks to: no scratch, no dynamic stack, no spills, <= 64
    VGPRs and <= 80 SGPRs (8 waves per SIMD)."""
    text = KM.assembly("bh_engine.hip")[0]
    seen = KM.kernels(text, r"_ZN2bh27forest_potential_f32_kernel\S+")
    assert len(seen) == 1, sorted(seen)
    for name, k in seen.items():
        assert k["scratch"] == 0 and k["dynamic_stack"] == "false" and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= 64 and k["sgpr"] <= 80, (name, k)
