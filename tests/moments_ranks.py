"""One rank of the distributed moment map, a process of its own: a helper of tests/test_gpu_moments.py, not a test file.

    python moments_ranks.py RANK WORLD PORT OUT_DIR

WORLD processes share the one GPU, so the collectives go over gloo (world 1: no process group at all).  Every rank takes its
share of the clump bodies of moments_ref.fixture (fp32 values), steps twice, re-balances once (bodies migrate), and then maps
the whole system with distributed.LetStepper.moment_map, both schemes; it writes the maps and ITS bodies to OUT_DIR/rankR.npz."""
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
import moments_ref as M  # noqa: E402

N, NX, NY = 4097, 64, 64
BOX = (-0.5, 2.5, -1.5, 0.5)             # inside the clumps' extent: bodies on every side of it


def bodies():
    pos, vel, mass = M.fixture(N, hand=False)
    return M.state_of(pos, vel, mass, precision_is_f32=True)


def main(rank, world, port, out_dir):
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    pos, vel, mass = bodies()
    mine = np.asarray(partition_orb(pos, world)[rank], dtype=np.int64)
    cfg = G.BhConfig(capacity=N + 4096, dt=1e-3, max_depth=21, precision=G.Precision.F32, reference_compat=False)
    with G.BarnesHutEngine(cfg) as eng:
        eng.upload(pos[mine], vel[mine], mass[mine])
        st = LetStepper(eng, rank, world, let_cap=1 << 13, device=dev, ids=mine)
        st.autotune()
        st.step()
        st.step()
        st.check()
        st.rebalance()
        out = {}
        for scheme in ("ngp", "cic"):
            mm = st.moment_map(BOX, NX, NY, scheme, raw=True)
            out[scheme + "_planes"], out[scheme + "_e"], out[scheme + "_n"] = mm.planes, mm.exponents, mm.n_deposited
            out[scheme + "_sigma"] = mm.sigma
        # the ranks must agree on the arguments: a different grid on one rank raises on every rank
        raised = False
        try:
            st.moment_map(BOX, NX + rank, NY, "cic")
        except ValueError:
            raised = True
        out["raised"] = raised
        p, v = eng.download()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=p, vel=v, mass=eng.masses(), ids=st.ids, **out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
