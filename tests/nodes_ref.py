"""Twin of the fp32 / mixed node records (nodes_fast_kernel, csrc/bh_tree.hpp) and the bound they are held to.

Plain numpy, no GPU.  `Twin(pos, mass, max_depth)` takes the caller-order bodies AS THE DEVICE HOLDS THEM (float32 values
widened to fp64 for Precision.F32, the fp64 values for Precision.MIXED), builds the oracle's tree, and identifies every cell
of it with its body set: the bodies are sent down the canonical tree with DetermineChild's comparisons on the
nodes' stored boxes, so body -> leaf is the reference's, and a cell's bodies are one contiguous range of the bodies sorted by
the pre-order index of their leaf (`order`, `lo`, `hi`).  The twin checks itself: a one-body leaf's `particle` names that
body, an empty leaf has no mass, several bodies share a leaf only at the depth cap.

REFERENCE VALUES: this module's own sums, not the oracle's fp64 mass / comx / comy.  The terms (m, m x, m y) are formed and
added in np.longdouble: the bodies of a leaf one after the other, then the four children of a cell, level by level.  With
u_ref = np.finfo(np.longdouble).eps (2^-63 on x86-64) a cell's sum carries at most (levels below it + bodies of its largest
leaf + 2) u_ref relative to its sum of |term|; that is added to the bound as `ref_units` (about one unit of 2^-53 for a
2,049-body depth-cap cell, nothing for ordinary cells).  (tests/test_nodes_ref_cpu.py also holds the oracle's own fp64 values to
these sums.)

WHAT THE DEVICE COMPUTES.  A cell of one body takes the body's sorted fp32 copies: compared with ==.  A cell of two or more
bodies [lo, hi) takes  mm = P[hi] - P[lo]  for each of the three terms, P the fp64 exclusive prefix sums over the whole sorted
array, then  m = (float)mm,  cx = (float)((P_b[hi] - P_b[lo]) * rcp(mm)).  A record whose fp32 mass is not > 1e-15f is stored
as (0, 0, 0) without children (project.cu:617).

H, THE LONGEST CHAIN OF fp64 ADDITIONS BETWEEN A TERM AND A STORED PREFIX SUM, counted from the code (an addition to a
zero-initialised accumulator counts as one).  W = 6: wave_inclusive_sum's DPP steps.  B = 4: block_exclusive_sum adds the four
wave totals in a row (`tot`; `base` takes at most three of them and then `+ prev`, also four).  S <= 8 rows of 256 per tile
(ITEMS).
    same row as the target            W + B (base, + prev) + 1 (dcarry + dex)                          = 11
    earlier row of the same tile      W + B (dtot) + (S - 1) (dcarry += dtot, once per row) + 1          = 18
    tile total (prep_kernel)          S (tsum += t) + W + B                                              = 18
    earlier tile, FOLD                18 + 8 (db += over <= 8 tiles per thread) + W + B (block total)
                                         + (S - 1) + 1                                                   = 44
    earlier tile, scan_top2           18 + max(W + B + 1 (same chunk of 256 tiles: ex, carry + ex),
                                               W + B + (C - 1) (carry += tot) + 1) + (S - 1) + 1         = 36 + C
with C = the number of 256-tile chunks scan_top2 loops over.  FOLD is taken while there are at most 8 * 256 tiles, and the
smallest tile is 512 keys, so  H(n) = 44  while n + 1 <= 2,048 * 512, and  max(44, 36 + ceil(ceil((n + 1) / 512) / 256))
beyond (an upper bound for every BH_BUILD_ITEMS).

THE BOUND (u = 2^-53, v = 2^-24; A_m = sum m, A_x = sum |m x|, A_y = sum |m y| over ALL bodies, which bound every partial sum of
absolute terms).  A stored prefix sum is  sum t_j (1 + th_j), |th_j| <= H u / (1 - H u), so the difference of two of them is off
by at most 2 H u A, its own rounding adds u A at most, and one more unit covers the second-order terms:  K = 2 H + 2 (+ ref_units).
F32 forms the terms from fp32 copies (24 + 24 bits: exact products); MIXED rounds m x and m y once in prep_kernel: one more
unit on the two moments, none on the mass.  For a cell of two or more bodies with exact mass M and centre X:
    e_M = K u A_m                               |mm - M| <= e_M
    e_B = (K + mixed) u A_x                     |bb - M X| <= e_B
    e_X = (e_B + |X| e_M) / (M - e_M) + 8 u |X|     (bb / mm against M X / M; v_rcp_f64 + two Newton steps + the multiply: 8 u)
    |m_dev - M|  <= e_M + v (M + e_M)           (the fp32 cast)
    |cx_dev - X| <= e_X + v (|X| + e_X)         and the same for y
When M <= e_M the cell is lighter than the prefix sums resolve: the centre has no bound (the mass still has), and it is
counted in `unresolved`.  These are the issue's constants; the only additions are the second-order terms e_M and e_X inside the
cast and M - e_M in the quotient, which matter only for such light cells.

PRUNING.  The twin prunes as the kernel does: one-body and empty records by the fp32 value itself; a larger cell is pruned when
(float)(M + e_M) is not > 1e-15f and kept when (float)(M - e_M) is.  In between -- a cell lighter than e_M -- the kernel's own
decision is rounding noise of the prefix sums, so the twin follows the export (a childless (0, 0, 0) record: pruned) and counts
the cell in `undecided`.  Everything below a pruned cell is absent from the export and from the comparison.
"""
import numpy as np

from oracle import bh_oracle as O

U53, U24 = 2.0 ** -53, 2.0 ** -24
CUT = np.float32(1e-15)
LD = np.longdouble
U_REF = float(np.finfo(LD).eps)

POPULATIONS = (2, 3, 7, 8, 9, 10, 16, 17, 255, 256, 257, 700, 800, 1023, 1024, 1025, 1032, 1100, 2047, 2049)
N_UNIFORM = 6000
CLUSTER_SEED = 1                                        # (checked on the CPU: tests/test_nodes_ref_cpu.py)
# cell counts of exactly 256 and 257 (a full and a ragged last workgroup of the node kernel), found with the oracle on the
# CPU: (n, seed) of uniform_case below, max_depth 21
CELLS_256 = (321, 17)
CELLS_257 = (316, 15)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def prefix_chain(n):
    """H(n): see the module docstring."""
    if n + 1 <= 2048 * 512:
        return 44
    tiles = -(-(n + 1) // 512)
    return max(44, 36 + -(-tiles // 256))


def cluster_case(w, straddle=False, seed=CLUSTER_SEED):
    """(pos, mass) in fp64: 6,000 uniform bodies in [-1, 1]^2, the four box corners (the root box is [-1.2, 1.2]^2), and one
    cluster per population, uniform in a square of half-width w about a random centre inside its own depth-11 cell (the
    depth-cap cell of max_depth 12; side 2.4 / 2,048 = 1.17e-3): clear of the cell's edges by a quarter of its side, or, with
    `straddle`, within 3 % of its side of the cell's corner, so that the cluster spills over four cells.  Masses uniform in [0.1, 0.5]."""
    rng = np.random.default_rng(seed)
    side = 2.4 / 2048
    cells = rng.choice(np.arange(300, 1748), size=(len(POPULATIONS), 2), replace=False)   # distinct rows AND columns, |centre| < 0.85
    frac = rng.uniform(-0.03, 0.03, (len(POPULATIONS), 2)) if straddle else rng.uniform(0.25, 0.75, (len(POPULATIONS), 2))
    centres = -1.2 + (cells + frac) * side
    parts = [rng.uniform(-1, 1, (N_UNIFORM, 2)), np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]])]
    for c, k in zip(centres, POPULATIONS):
        parts.append(c + rng.uniform(-w, w, (k, 2)))
    pos = np.concatenate(parts)
    mass = rng.uniform(0.1, 0.5, len(pos))
    return pos, mass


def off_grid(pos, seed=1):
    """Positions off the fp32 grid (as tests/test_gpu_mixed.py does), the four corner bodies left where they are."""
    q = pos * (1.0 + 3e-9 * np.random.default_rng(seed).standard_normal(pos.shape))
    corner = (np.abs(pos) == 1.0).all(axis=1)
    q[corner] = pos[corner]
    assert not np.array_equal(q, f32(q))
    return q


def uniform_case(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, 2)), rng.uniform(0.1, 0.5, n)


class Twin:
    def __init__(self, pos, mass, max_depth):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        self.pos, self.mass, self.max_depth, self.n = pos, mass, max_depth, len(mass)
        self.ref, self.depth = O.canonical_tree(O.build_tree(pos, mass, max_depth))
        ref, depth = self.ref, self.depth
        N = len(ref)
        self.has = ref["child"][:, 0] != -1
        assert np.array_equal(self.has, (ref["child"] != -1).all(axis=1))          # four children or none
        # children and subtree sizes, bottom-up: the nodes of depth d + 1 in pre-order are the children, four by four, of the
        # subdivided nodes of depth d in pre-order
        dmax = int(depth.max())
        by_depth = np.argsort(depth, kind="stable")
        cuts = np.concatenate([[0], np.cumsum(np.bincount(depth, minlength=dmax + 1))])
        at = [by_depth[cuts[d]:cuts[d + 1]] for d in range(dmax + 1)]
        self.kids = np.full((N, 4), -1, dtype=np.int64)
        size = np.ones(N, dtype=np.int64)
        self._levels = []
        for d in range(dmax - 1, -1, -1):
            par = at[d][self.has[at[d]]]
            ch = at[d + 1].reshape(-1, 4)
            assert len(ch) == len(par) and np.array_equal(ch[:, 0], par + 1)
            self.kids[par] = ch
            size[par] = 1 + size[ch].sum(axis=1)
            self._levels.append((par, ch))
        assert not self.has[at[dmax]].any() and size[0] == N
        self.size = size
        # body -> leaf by DetermineChild (project.cu:348-356) on the nodes' own boxes (finite bodies: its four tests are
        # (x >= mx) + 2 (y >= my))
        assert np.isfinite(pos).all()
        midx, midy = (ref["xmin"] + ref["xmax"]) / 2, (ref["ymin"] + ref["ymax"]) / 2
        leaf = np.zeros(self.n, dtype=np.int64)
        act = np.arange(self.n) if (N > 1) else np.arange(0)
        x, y = pos[:, 0].copy(), pos[:, 1].copy()
        while act.size:
            k = leaf[act]
            c = (x[act] >= midx[k]).astype(np.int64) + 2 * (y[act] >= midy[k])
            k = self.kids[k, c]
            leaf[act] = k
            act = act[self.has[k]]
        self.order = np.argsort(leaf, kind="stable")                                 # DFS leaf order, body order inside a leaf
        sl = leaf[self.order]
        idx = np.arange(N)
        self.lo = np.searchsorted(sl, idx, side="left")
        self.hi = np.searchsorted(sl, idx + size, side="left")
        self.cnt = self.hi - self.lo
        cnt = self.cnt
        assert cnt[0] == self.n and (cnt[self.has] >= 2).all()
        leaves = ~self.has
        assert (depth[leaves & (cnt > 1)] == max_depth - 1).all()                     # several bodies: depth-cap leaves only
        assert (ref["mass"][leaves & (cnt == 0)] == 0).all()
        one = cnt == 1
        self.body = np.where(one, self.order[np.minimum(self.lo, max(self.n - 1, 0))], -1) if self.n else np.full(N, -1)
        p = ref["particle"][one]
        assert np.array_equal(np.where(p >= 0, p, -p - 2), self.body[one])
        assert (ref["particle"][~one] == -1).all()
        # exact sums
        t = np.stack([mass.astype(LD), mass.astype(LD) * pos[:, 0].astype(LD), mass.astype(LD) * pos[:, 1].astype(LD)], axis=1)[self.order]
        S = np.zeros((N, 3), dtype=LD)
        full = np.flatnonzero(leaves & (cnt > 0))
        if full.size:
            S[full] = np.add.reduceat(t, self.lo[full], axis=0)
        for par, ch in self._levels:
            S[par] = S[ch[:, 0]] + S[ch[:, 1]] + S[ch[:, 2]] + S[ch[:, 3]]
        self.S = S
        self.M = S[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.X = np.where(cnt > 0, S[:, 1] / S[:, 0], 0)
            self.Y = np.where(cnt > 0, S[:, 2] / S[:, 0], 0)
        self.A = np.array([float(np.abs(t[:, k]).sum()) for k in range(3)]) if self.n else np.zeros(3)
        pmax = int(cnt[leaves].max()) if N else 0
        self.ref_units = (dmax + pmax + 3) * U_REF / U53
        self.H = prefix_chain(self.n)

    # ---- the bound -------------------------------------------------------------------------------------
    def bounds(self, k, mixed, H=None):
        """(bound_m, bound_x, bound_y, e_M) for the nodes k (meaningful where cnt >= 2); inf where there is no bound."""
        K = 2 * (self.H if H is None else H) + 2 + self.ref_units
        M = self.M[k].astype(np.float64)
        e_M = K * U53 * self.A[0]
        out = [e_M + U24 * (M + e_M)]
        with np.errstate(divide="ignore", invalid="ignore"):
            for C, A in ((self.X, self.A[1]), (self.Y, self.A[2])):
                c = np.abs(C[k].astype(np.float64))
                e_B = (K + (1 if mixed else 0)) * U53 * A
                e_C = np.where(M > e_M, (e_B + c * e_M) / (M - e_M) + 8 * U53 * c, np.inf)
                out.append(e_C + U24 * (c + e_C))
        return out[0], out[1], out[2], e_M

    def judge(self, k, m, cx, cy, mixed, H=None):
        """Per node k with device values (m, cx, cy): ratios error / bound for the three fields.  One-body and empty cells have no
        bound: their ratio is 0 where the value is == the expected one and inf where it is not.  (No pruning here.)"""
        k = np.asarray(k)
        m, cx, cy = (np.asarray(a, dtype=np.float64) for a in (m, cx, cy))
        cnt = self.cnt[k]
        bm, bx, by, _ = self.bounds(k, mixed, H)
        with np.errstate(invalid="ignore", divide="ignore"):
            rm = np.abs((m.astype(LD) - self.M[k]).astype(np.float64)) / bm
            rx = np.where(np.isinf(bx), 0.0, np.abs((cx.astype(LD) - self.X[k]).astype(np.float64)) / bx)
            ry = np.where(np.isinf(by), 0.0, np.abs((cy.astype(LD) - self.Y[k]).astype(np.float64)) / by)
        b = np.maximum(self.body[k], 0)
        em = np.where(cnt == 1, f32(self.mass[b]) if self.n else 0.0, 0.0)
        ex = np.where(cnt == 1, f32(self.pos[b, 0]) if self.n else 0.0, 0.0)
        ey = np.where(cnt == 1, f32(self.pos[b, 1]) if self.n else 0.0, 0.0)
        dead = (cnt == 1) & ~(em.astype(np.float32) > CUT)                             # project.cu:617 on a one-body record
        em, ex, ey = np.where(dead, 0.0, em), np.where(dead, 0.0, ex), np.where(dead, 0.0, ey)
        small = cnt <= 1
        rm = np.where(small, np.where(m == em, 0.0, np.inf), rm)
        rx = np.where(small, np.where(cx == ex, 0.0, np.inf), rx)
        ry = np.where(small, np.where(cy == ey, 0.0, np.inf), ry)
        return rm, rx, ry

    # ---- the device path in numpy ------------------------------------------------------------------------
    def terms(self):
        """fp64 terms (m, m x, m y) in DFS leaf order, as prep_kernel forms them."""
        o = self.order
        return np.stack([self.mass[o], self.mass[o] * self.pos[o, 0], self.mass[o] * self.pos[o, 1]], axis=1)

    def prefix(self):
        """Exclusive fp64 prefix sums (n + 1 rows), by sequential cumsum: H = n for this emulation."""
        P = np.zeros((self.n + 1, 3))
        np.cumsum(self.terms(), axis=0, out=P[1:])
        return P

    def records(self, P, k, lo=None, hi=None):
        """(m, cx, cy) the node kernel stores for the cells k given the prefix sums P and the cells' body ranges (before pruning)."""
        k = np.asarray(k)
        lo = self.lo[k] if lo is None else np.asarray(lo)
        hi = self.hi[k] if hi is None else np.asarray(hi)
        c = hi - lo
        first = self.order[np.clip(lo, 0, max(self.n - 1, 0))] if self.n else np.zeros_like(lo)
        d = P[hi] - P[lo]
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(c == 1, f32(self.mass[first]), np.where(c > 1, f32(d[:, 0]), 0.0))
            cx = np.where(c == 1, f32(self.pos[first, 0]), np.where(c > 1, f32(d[:, 1] / d[:, 0]), 0.0))
            cy = np.where(c == 1, f32(self.pos[first, 1]), np.where(c > 1, f32(d[:, 2] / d[:, 0]), 0.0))
        return m, cx, cy

    def emulate_export(self, P=None):
        """(nodes, depth) as BarnesHutEngine.export_tree() would show them if the prefix sums were P."""
        P = self.prefix() if P is None else P
        N = len(self.ref)
        m, cx, cy = self.records(P, np.arange(N))
        dead = ~(m.astype(np.float32) > CUT)
        gone = np.zeros(N, dtype=bool)
        for k in np.flatnonzero(dead & self.has):
            gone[k + 1:k + self.size[k]] = True
        out = self.ref.copy()
        out["mass"], out["comx"], out["comy"] = np.where(dead, 0, m), np.where(dead, 0, cx), np.where(dead, 0, cy)
        out["child"][dead] = -1.0
        out["particle"] = np.where(self.cnt == 1, self.ref["particle"], -1.0)
        return out[~gone], self.depth[~gone]

    # ---- the comparison ---------------------------------------------------------------------------------------
    def check(self, nodes, depth, mixed, H=None):
        """Every exported node against the twin; returns {"mass", "comx", "comy": largest error / bound, "unresolved": cells
        lighter than e_M, "undecided": cells whose pruning the bound cannot decide, "nodes"}.  AssertionError otherwise."""
        ref, N = self.ref, len(self.ref)
        allk = np.arange(N)
        _, _, _, e_M = self.bounds(allk, mixed, H)
        M = self.M.astype(np.float64)
        big = self.cnt >= 2
        sure_dead = big & ~((M + e_M).astype(np.float32) > CUT)
        sure_live = big & ((M - e_M).astype(np.float32) > CUT)
        undecided = big & ~sure_dead & ~sure_live
        # which reference nodes the export shows: below a pruned cell nothing
        gone = np.zeros(N, dtype=bool)
        pruned = sure_dead.copy()
        for k in np.flatnonzero(self.has & ~sure_live):
            if gone[k]:
                continue
            j = k - int(gone[:k].sum())
            if undecided[k]:
                assert j < len(nodes), "export shorter than the twin"
                pruned[k] = bool((nodes["child"][j] == -1).all() and nodes["mass"][j] == 0 and nodes["comx"][j] == 0 and nodes["comy"][j] == 0)
            if pruned[k]:
                gone[k + 1:k + self.size[k]] = True
        vis = allk[~gone]
        assert len(nodes) == len(vis), (len(nodes), len(vis))
        for k in np.flatnonzero(undecided[vis] & ~self.has[vis]):                     # depth-cap leaves: either record
            v = vis[k]
            pruned[v] = bool(nodes["mass"][k] == 0 and nodes["comx"][k] == 0 and nodes["comy"][k] == 0)
        assert np.array_equal(depth, self.depth[vis])
        for f in ("xmin", "xmax", "ymin", "ymax"):
            assert np.array_equal(nodes[f], ref[f][vis]), f
        has_dev = nodes["child"][:, 0] != -1
        assert np.array_equal(has_dev, (nodes["child"] != -1).all(axis=1))
        assert np.array_equal(has_dev, self.has[vis] & ~pruned[vis]), "has-child flags"
        one = self.cnt[vis] == 1
        assert np.array_equal(nodes["particle"][one], ref["particle"][vis][one]), "particle of one-body leaves"
        assert (nodes["particle"][~one] == -1).all(), "particle of cells that hold no or several bodies"
        rm, rx, ry = self.judge(vis, nodes["mass"], nodes["comx"], nodes["comy"], mixed, H)
        pv = pruned[vis]
        zero = (nodes["mass"] == 0) & (nodes["comx"] == 0) & (nodes["comy"] == 0)
        assert zero[pv].all(), "a pruned record is (0, 0, 0)"
        rm, rx, ry = np.where(pv, 0.0, rm), np.where(pv, 0.0, rx), np.where(pv, 0.0, ry)
        res = {"mass": float(rm.max()), "comx": float(rx.max()), "comy": float(ry.max()),
               "unresolved": int((big[vis] & ~(M[vis] > e_M)).sum()), "undecided": int(undecided[vis].sum()), "nodes": len(vis)}
        for name, r, dev, exact in (("mass", rm, nodes["mass"], self.M), ("comx", rx, nodes["comx"], self.X), ("comy", ry, nodes["comy"], self.Y)):
            w = int(np.argmax(r))
            assert r[w] <= 1.0, (f"{name}: error / bound = {r[w]:.4g} at exported node {w} (depth {depth[w]}, {self.cnt[vis[w]]} bodies, "
                                 f"sorted range [{self.lo[vis[w]]}, {self.hi[vis[w]]})): device {dev[w]!r}, exact {float(exact[vis[w]])!r}; "
                                 f"H = {self.H if H is None else H}, largest ratios {res}")
        return res
