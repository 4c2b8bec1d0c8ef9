"""One GPU rehearsing the distributed step: W contexts act as W ranks, and the collectives (all_gather of the bounds,
all_to_all of the LET blocks, the all_reduce and all_to_all of a re-balance) are device copies between them -- a helper of
tests/test_gpu_let.py and the tests/test_gpu_let_*.py modules, not a test file.  The device code is the real one."""
import numpy as np
import torch

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd.distributed import (ORB_BINS, OrbCuts, choose_cut, padded_root_box, partition_orb,
                                                  wrap_device)

# the 80-byte record of a sibling quad (csrc/bh_nodes.hpp: QuadF)
QUAD_DTYPE = np.dtype([("xy", "<f4", (8,)), ("m", "<f4", (4,)), ("thr", "<f4", (4,)), ("child", "<i4", (4,))])
assert QUAD_DTYPE.itemsize == 80


class EmulatedRanks:
    def __init__(self, mass, pos, vel, world, let_cap, partition=partition_orb, headroom=1.0, **cfg):
        self.world = world
        self.parts = partition(pos, world)
        dev = torch.device("cuda", 0)
        self.engs, self.bufs = [], []
        cfg.setdefault("precision", G.Precision.F32)
        # every context sized for ITS OWN bodies, as bench.py does: the contexts' quad arrays then differ
        # in size, and only the agreed forest_base makes a sender's links land in the receiver's blocks
        for ix in self.parts:
            e = G.BarnesHutEngine(G.BhConfig(capacity=max(int(headroom * len(ix)), 1), **cfg))
            e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for the contexts and the "collectives"
            e.upload(pos[ix], vel[ix], mass[ix])
            e.set_ids(ix)
            self.engs.append(e)
        self.forest_base = max(e.let_local_quads() for e in self.engs)
        self.dev = dev
        self.configure(let_cap)

    def configure(self, let_cap):
        if let_cap is None:                   # room for any rank's whole tree: no LET can overflow
            let_cap = self.forest_base
        self.let_cap, self.bufs = let_cap, []
        dev, world = self.dev, self.world
        for r, e in enumerate(self.engs):
            e.let_configure(r, world, let_cap, self.forest_base)
            lb, ab, sd, rv, nb, k = e.let_pointers()
            self.bufs.append((wrap_device(lb, 4 * k, "<f8", dev), wrap_device(ab, 4 * k * world, "<f8", dev),
                              wrap_device(sd, world * nb, "|u1", dev), wrap_device(rv, world * nb, "|u1", dev), nb))

    def rebalance(self, tol=0.01):
        """LetStepper.rebalance() with the three collectives replaced by device copies / sums between the
        contexts of this one GPU: the device code (histogram, classify, group, pack, unpack) is the real one.
        Returns (cuts, summed histograms per level)."""
        W, dev = self.world, self.dev
        for e in self.engs:
            e.let_bounds()
        torch.cuda.synchronize()
        b = torch.cat([x[0] for x in self.bufs]).cpu().numpy().reshape(-1, 4)
        b = b[np.isfinite(b).all(1) & (b[:, 0] <= b[:, 1])]
        cuts = OrbCuts(W, padded_root_box(b[:, 0].min(), b[:, 1].max(), b[:, 2].min(), b[:, 3].max()))
        hists = []
        for level in range(cuts.depth()):
            regs = cuts.regions(level)
            for k, _, _, rb in regs:
                cuts.axis[k] = int((rb[3] - rb[2]) > (rb[1] - rb[0]))
            tot = None
            for e in self.engs:
                ptr, nw = e.orb_histogram(cuts, level)
                h = wrap_device(ptr, nw, "<i8", dev).clone()
                tot = h if tot is None else tot + h                      # "all_reduce"
            hh = tot.cpu().numpy().reshape(-1, ORB_BINS)
            hists.append(hh)
            for k, _, nr, rb in regs:
                cuts.value[k] = choose_cut(hh[k], rb, cuts.box, int(cuts.axis[k]), (nr // 2) / nr, tol)
        counts = [e.migrate_pack(cuts) for e in self.engs]               # counts[src][dst]
        ptrs = [e.migrate_pointers() for e in self.engs]
        send = [wrap_device(p[0], p[2] * 6, "<f8", dev) for p in ptrs]
        recv = [wrap_device(p[1], p[2] * 6, "<f8", dev) for p in ptrs]
        for dst in range(W):                                             # "all_to_all_single" with splits
            o = 0
            for src in range(W):
                c = counts[src][dst]
                so = sum(counts[src][:dst])
                assert o + c <= ptrs[dst][2], "capacity"
                recv[dst][6 * o: 6 * (o + c)].copy_(send[src][6 * so: 6 * (so + c)])
                o += c
            self.engs[dst].migrate_unpack(o)
        torch.cuda.synchronize()
        self.cuts = cuts
        return cuts, hists

    def ids(self):
        return [e.ids() for e in self.engs]

    def step(self, integrate=True, two_launches=False, bounds=True):
        """bounds=False: the caller has run let_bounds() on every rank already (and looked at the boxes)."""
        for e in self.engs:
            if bounds:
                e.let_bounds()
            e.sync()
        allb = torch.cat([b[0] for b in self.bufs])                 # "all_gather"
        for b in self.bufs:
            b[1].copy_(allb)
        torch.cuda.synchronize()
        for e in self.engs:
            e.let_build()
            e.sync()
        for r in range(self.world):                                  # "all_to_all"
            nb = self.bufs[r][4]
            for q in range(self.world):
                if q != r:
                    self.bufs[q][3][r * nb:(r + 1) * nb].copy_(self.bufs[r][2][q * nb:(q + 1) * nb])
        torch.cuda.synchronize()
        for e in self.engs:
            if two_launches:
                e.let_walk_local()
                e.let_walk_remote(integrate)
            else:
                e.let_walk() if integrate else e.let_forces()
            e.sync()

    def gather(self, what):
        n = sum(e.n for e in self.engs)
        out = np.zeros((n, 2))
        for e in self.engs:
            out[e.ids()] = what(e)                                       # ids = the caller's global indices
        return out

    def close(self):
        for e in self.engs:
            e.close()

    def gather1(self, what, dtype=np.int64):
        """gather() for one value per body."""
        out = np.zeros(sum(e.n for e in self.engs), dtype=dtype)
        for e in self.engs:
            out[e.ids()] = what(e)
        return out

    # -- what the device holds, read back (tests/test_gpu_let_blocks.py, tests/test_gpu_let_boxes.py) --------------------
    def _quads(self, r, first, count):
        """`count` quad records of rank r's forest array from record `first` (0 = its own root quad)."""
        rv = self.engs[r].let_pointers()[3]
        t = wrap_device(rv - 80 * self.forest_base + 80 * first, 80 * count, "|u1", self.dev)
        torch.cuda.synchronize()
        return t.cpu().numpy().view(QUAD_DTYPE).copy()

    def local_quads(self, r):
        """Rank r's own tree: quads 0 .. n_internal."""
        return self._quads(r, 0, self.engs[r].stats().n_internal + 1)

    def send_block(self, r, q):
        """The let_cap records rank r packed for peer q."""
        nb = self.bufs[r][4]
        torch.cuda.synchronize()
        return self.bufs[r][2][q * nb:(q + 1) * nb].cpu().numpy().view(QUAD_DTYPE).copy()

    def recv_block(self, q, r):
        """The let_cap records rank q holds of sender r."""
        nb = self.bufs[q][4]
        torch.cuda.synchronize()
        return self.bufs[q][3][r * nb:(r + 1) * nb].cpu().numpy().view(QUAD_DTYPE).copy()

    def lbounds(self, r):
        """[8, 4] {xmin, xmax, ymin, ymax}: rank r's boxes as its last let_bounds() left them."""
        torch.cuda.synchronize()
        return self.bufs[r][0].cpu().numpy().reshape(-1, 4).copy()

    def all_bounds(self, r):
        """[world, 8, 4]: every rank's boxes as rank r received them."""
        torch.cuda.synchronize()
        return self.bufs[r][1].cpu().numpy().reshape(self.world, -1, 4).copy()


def expected_split(n_rank, flags=0, n_threads=0, world=2):
    """Waves per 64-body group that launch_walk_f32 (csrc/bh_engine.hip) picks for a rank of n_rank bodies in LET mode:
    8 up to 512 groups, 4 up to 3,072, then the one-wave loop; one wave with FLAG_WALK_NO_SPLIT, the LDS stack, n_threads
    passes, or more than 56 trees."""
    from gpu_nbody_simulation_amd.engine import FLAG_LDS_STACK, FLAG_WALK_NO_SPLIT
    if (flags & (FLAG_WALK_NO_SPLIT | FLAG_LDS_STACK)) or n_threads > 0 or world > 56:
        return 1
    groups = -(-n_rank // 64)
    return 8 if groups <= 512 else 4 if groups <= 3072 else 1


def rel(a, ref):
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)
