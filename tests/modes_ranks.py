"""One rank of the distributed azimuthal modes, a process of its own: a helper of tests/test_gpu_modes.py, not a test file.

    python modes_ranks.py RANK WORLD PORT OUT_DIR

WORLD processes share the one GPU, so the collectives go over gloo (world 1: no process group at all).  Every rank takes its
share of the bodies of modes_ref.fixture (fp32 values), steps twice, re-balances once (bodies migrate), and then takes the modes
of the whole system with distributed.LetStepper; it writes the results and ITS bodies to OUT_DIR/rankR.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd.distributed import LetStepper, partition_orb  # noqa: E402
import modes_ref as MR  # noqa: E402

N, NB, M = 4097, 33, 5


def bodies():
    pos, vel, mass = MR.fixture(N, NB, hand=False, decades=1.0)
    return MR.state_of(pos, vel, mass, precision_is_f32=True)


def main(rank, world, port, out_dir):
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    pos, vel, mass = bodies()
    mine = np.asarray(partition_orb(pos, world)[rank], dtype=np.int64)
    cfg = G.BhConfig(capacity=N + 4096, dt=1e-3, max_depth=21, precision=G.Precision.F32, reference_compat=False)
    edges = MR.fixture_edges(NB)
    with G.BarnesHutEngine(cfg) as eng:
        eng.upload(pos[mine], vel[mine], mass[mine])
        st = LetStepper(eng, rank, world, let_cap=1 << 13, device=dev, ids=mine)
        st.autotune()
        st.step()
        st.step()
        st.check()
        st.rebalance()
        out = {}
        md = st.azimuthal_modes(edges, M, MR.CENTRE, MR.CENTRE_VEL, rates=True, raw=True)
        out["planes"], out["e"], out["amplitude"], out["speed"] = md.planes, md.exponents, md.amplitude, md.pattern_speed
        plain = st.azimuthal_modes(edges, 2, MR.CENTRE, raw=True)
        out["plain_planes"], out["plain_e"] = plain.planes, plain.exponents
        com = st.azimuthal_modes(edges, centre="com", raw=True)
        out["com"], out["com_planes"], out["com_m"] = np.array(com.centre), com.planes, com.m_max
        # the ranks must agree on the arguments: a different edge, harmonic count or rates flag on one rank raises on every rank
        raised = 0
        for call in (lambda: st.azimuthal_modes(edges + 0.001 * rank, M, MR.CENTRE), lambda: st.azimuthal_modes(edges, M + rank, MR.CENTRE),
                     lambda: st.azimuthal_modes(edges, M, MR.CENTRE, rates=bool(rank))):
            try:
                call()
            except ValueError:
                raised += 1
        try:
            st.azimuthal_modes(edges, M, "density")
        except ValueError:
            raised += 1
        out["raised"] = raised
        p, v = eng.download()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=p, vel=v, mass=eng.masses(), ids=st.ids, **out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
