// bh_mst.hpp -- the Euclidean minimum spanning tree of the current state and of small subsets of it (bh_spanning_tree,
// bh_spanning_tree_subsets).  The reference has no such output.  Included by bh_engine.hip after bh_groups.hpp, so it is compiled
// with -ffp-contract=off: nothing below is fused.
//
// Definition.  d2(i, j) is the d2 of bh_count_within and bh_groups: dx = x_j - x_i, dy = y_j - y_i, d2 = dx * dx + dy * dy in fp64
// (an fp32 state is widened first, which is exact), symmetric in (i, j) bit for bit.  The edges of the complete graph are ordered
// by the triple (d2, lo, hi), lo < hi the CALLER indices of the two ends: a strict total order, so the minimum spanning tree is
// unique -- with coincident bodies and on a lattice too.  In the code an edge is the pair of words (bits of d2, lo << 24 | hi):
// a non-negative double orders as its bit pattern, and the indices fit because the index holds at most 2^24 bodies.
//
// Whole state: Boruvka's algorithm on the index of bh_neighbours.hpp as nb_build leaves it (spos, sidx, boxes, off, levels).
// State over SORTED positions s: parent[] as in bh_groups.hpp (parent[s] <= s, a root is the lowest position of its tree, every
// write an atomic, agent-scope relaxed loads while unions run), comp[s] = the root of s, flattened after every round.  A round:
//   mst_nodecomp_kernel  level by level, bottom-up: nodecomp[node] = the component all bodies under the node share, else
//                        kMstMixed.  A lane never opens a subtree that lies wholly inside its own component: late rounds, when
//                        few large components are left, open the nodes along the borders only.
//   mst_seed_kernel      every lane looks at the sorted positions s +- kMstSeed for bodies of other components: its seed, the
//                        smallest such edge, goes to cand[], and its d2 to seedmin[comp] with a 64-bit atomicMin.  Every
//                        component has a seed (where its run of sorted positions ends, another begins).
//   mst_nearest_kernel   nb_walk (bh_neighbours.hpp), one lane per sorted body; the node components and the leaf bodies'
//                        comp / sidx are read at the walker's wave-uniform addresses, in the constant address space too.
//                        The lane finds its smallest edge, in the edge order, to a body of another
//                        component: `best`, which starts from the lane's seed (the traversal skips the seeds' positions).  A
//                        node is dropped when its component is the lane's, or when lb > bound = min(best.d2, the smallest seed
//                        of the lane's component) -- STRICTLY: at equality an edge with smaller indices can still win (as in
//                        nb_knn_kernel; lb is nb_bound's, so the computed d2 of every body of the node is >= lb).  The
//                        component's smallest seed is the d2 of a real edge that leaves the component, so the component's
//                        final edge is not longer: no lane loses that edge, or any edge of its d2, to the bound.  It is what
//                        keeps the late rounds cheap: a lane deep inside a large component has no near foreign body, and
//                        without the bound it would open every mixed node until it met one.  At the end the lanes send
//                        the bits of best.d2 to mind2[comp] with a 64-bit atomicMin (the lanes of a wave that share a component
//                        send one minimum) and keep (d2, pair) in cand[].
//                        The scalar cache is not coherent with stores of the running kernel: everything this kernel reads
//                        through the scalar unit -- boxes, off, nodecomp, spos, comp, sidx -- was written by an EARLIER launch.
//                        mind2[] is written by this launch and not read by it.
//   mst_pick_kernel      the 128-bit minimum without a 128-bit atomic: the lanes whose d2 equals their component's minimum
//                        send their pair to minpair[comp] with a second 64-bit atomicMin.
//   mst_hook_kernel      one thread per component with a chosen edge calls grp_union on its two ends and appends the edge to
//                        the output iff THAT CALL hooked.  Under a strict total order the chosen edges form a forest (a cycle
//                        would need an edge that is not the smallest leaving either of the components it joins), except that
//                        two components may choose the same edge.  A union hooks exactly when its ends were in two trees at
//                        the instant of the CAS, and the ends of an edge of a forest are in one tree only when that very edge
//                        has been added: so every distinct chosen edge is appended once, the second copy of a mutual choice
//                        finds one tree and appends nothing, and the call ends with n - 1 edges.
//   mst_flatten_kernel   comp[s] = the root of s (pointer chasing from the old comp[s], which is an ancestor), the number of
//                        roots of the round, and mind2 / minpair reset for the next.  A launch of its own: the kernel boundary
//                        is the only hand-off relied on.
// Each round at least halves the number of components (every component chooses an edge); the host loops until one is left,
// reads one 8-byte word per round and gives up with an error beyond kMstMaxRounds -- it never spins.
// The final order: the n - 1 records are sorted by the bits of d2 with the stable LSD passes of bh_sort.hpp (eight, the edge's
// place in the append order as the payload: mst_iota_kernel), mst_gather_kernel puts the pairs in that order, and the host sorts
// the runs of equal d2 by pair -- on a lattice that is all of them, on a state in general position none.
//
// Pruning on the component's RUNNING minimum as well (mind2[comp], re-read during the traversal) gives the same edges by the
// same argument; it was measured and lost and is not in the code.
//
// Counters (MstCounters; stats of bh_spanning_tree): rounds, distances computed, nodes skipped as own-component and edges are
// all the same in every run -- every decision rests on boxes, positions, comp[], the lane's own best and seedmin[], which an
// earlier launch completed; the races of the atomics decide nothing but the order in which the edges are appended.
//
// Subsets (mst_subset_kernel): many small dense problems, one wavefront (one workgroup) per subset.  Prim's algorithm with the
// set's positions, best keys (d2, pair) and caller indices in LDS, item t belongs to lane t % 64 for good: a lane reads and
// writes the keys of its own items only, and whether an item is in the tree is a bit in a register of its lane.  k - 1
// selections, each a wave-wide arg-min over (d2, pair) by shuffles; the update against the body just added is fused into the
// next selection's scan.  Every loop is bounded by k.  The start (item 0) cannot matter: the tree is unique.
#pragma once

#include "bh_groups.hpp"

namespace bh {

constexpr int kMstMaxRounds = 25;                 // 2^24 bodies need 24; the host stops with an error beyond
constexpr int kMstSeed = 4;                       // sorted neighbours on either side that seed a lane's best
constexpr int kMstSubsetMax = 512;                // = BH_MST_SUBSET_MAX: 36 bytes of LDS per item, 18 KiB per workgroup
constexpr int kMstItems = kMstSubsetMax / kWave;  // items of a subset per lane at most
constexpr uint32_t kMstMixed = ~0u;               // a node whose bodies lie in more than one component
constexpr unsigned long long kMstNone = ~0ull;    // no edge (above the bits of +inf; a pair of real indices is below 2^48)

// counters of a call on the device
struct MstCounters {
    unsigned long long evals, skips, edges;
    unsigned long long roots[kMstMaxRounds + 1];  // components left after round r
};

__device__ __forceinline__ unsigned long long mst_pair(uint32_t a, uint32_t b)
{
    const uint32_t lo = (a < b) ? a : b, hi = (a < b) ? b : a;
    return ((unsigned long long)lo << 24) | (unsigned long long)hi;
}

// (d, p) before (bd, bp) in the edge order
__device__ __forceinline__ bool mst_before(double d, unsigned long long p, double bd, unsigned long long bp)
{
    return d < bd || (d == bd && p < bp);
}

__device__ __forceinline__ unsigned long long mst_wave_min(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = (o < v) ? o : v;
    }
    return v;
}

// every body a component of its own; inv[caller index] = sorted position
__global__ __launch_bounds__(kBlock) void mst_init_kernel(const uint32_t *__restrict__ sidx, int32_t n, uint32_t *__restrict__ parent,
                                                          uint32_t *__restrict__ comp, uint32_t *__restrict__ inv,
                                                          unsigned long long *__restrict__ seedmin,
                                                          unsigned long long *__restrict__ mind2, unsigned long long *__restrict__ minpair)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    parent[s] = (uint32_t)s;
    comp[s] = (uint32_t)s;
    inv[sidx[s]] = (uint32_t)s;
    seedmin[s] = kMstNone;
    mind2[s] = kMstNone;
    minpair[s] = kMstNone;
}

// one level of node components (`count` nodes): level 0 from comp[] of the leaf's bodies, a level above from the `below` nodes
// of `down`
__global__ __launch_bounds__(kBlock) void mst_nodecomp_kernel(const uint32_t *__restrict__ comp, const uint32_t *__restrict__ down,
                                                              int32_t level, int32_t below, int32_t n, int32_t count,
                                                              uint32_t *__restrict__ up)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    uint32_t c;
    if (level == 0) {
        const int64_t first = i * kNbLeaf;
        const int64_t last = (first + kNbLeaf < n) ? first + kNbLeaf : (int64_t)n;
        c = comp[first];
        for (int64_t j = first + 1; j < last; ++j) c = (comp[j] == c) ? c : kMstMixed;
    } else {
        c = down[4 * i];
        for (int k = 1; k < 4; ++k) {
            if (4 * i + k >= below) break;
            c = (down[4 * i + k] == c) ? c : kMstMixed;
        }
    }
    up[i] = c;
}

// sends the lanes' d2 (kMstNone: none) to mind2[mine]: the bodies lie in curve order, so the lanes of a wave have few components
// -- up to kGrpRounds times the lanes that share the component of the first lane left send one minimum; the other lanes send
// their own
__device__ __forceinline__ void mst_send(unsigned long long *__restrict__ mind2, uint32_t mine, unsigned long long bits)
{
    const int lane = lane_id();
    const bool have = bits != kMstNone;
    unsigned long long todo = __ballot(have);
    for (int round = 0; round < kGrpRounds && todo != 0ull; ++round) {
        const int first = __builtin_ctzll(todo);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, first);
        const bool same = have && mine == c0;
        todo &= ~__ballot(same);
        const unsigned long long low = mst_wave_min(same ? bits : kMstNone);
        if (lane == first) atomicMin(mind2 + c0, low);
    }
    if (((todo >> lane) & 1ull) != 0ull) atomicMin(mind2 + mine, bits);
}

// the seeds: the smallest edge of the body at sorted position s to a body of another component among the sorted positions
// s +- kMstSeed, into cand_d2[s] (kMstNone: none) and cand_pair[s]; seedmin[comp[s]] lowered to it
__global__ __launch_bounds__(kBlock) void mst_seed_kernel(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                                          const uint32_t *__restrict__ comp, int32_t n,
                                                          unsigned long long *__restrict__ seedmin,
                                                          unsigned long long *__restrict__ cand_d2,
                                                          unsigned long long *__restrict__ cand_pair, MstCounters *__restrict__ ctr)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < n;
    const int32_t s = valid ? (int32_t)r : 0;
    uint32_t mine = kMstMixed, evals = 0;
    double bd = (double)INFINITY;
    unsigned long long bp = kMstNone;
    if (valid) {
        const double2 q = spos[s];
        const uint32_t id = sidx[s];
        mine = comp[s];
        const int32_t j0 = (s - kMstSeed > 0) ? s - kMstSeed : 0, j1 = (s + kMstSeed < n - 1) ? s + kMstSeed : n - 1;
        for (int32_t j = j0; j <= j1; ++j) {
            if (comp[j] == mine) continue;
            const double2 p = spos[j];
            const double dx = p.x - q.x, dy = p.y - q.y;
            const double d = dx * dx + dy * dy;
            const unsigned long long pr = mst_pair(id, sidx[j]);
            ++evals;
            if (mst_before(d, pr, bd, bp)) { bd = d; bp = pr; }
        }
    }
    const unsigned long long bits = (valid && bp != kMstNone) ? (unsigned long long)__double_as_longlong(bd) : kMstNone;
    if (valid) { cand_d2[s] = bits; cand_pair[s] = bp; }
    mst_send(seedmin, mine, bits);
    const unsigned long long e = grp_wave_sum(evals);
    if (lane_id() == 0 && e) atomicAdd(&ctr->evals, e);
}

// the smallest edge of the body at sorted position s to a body of another component: cand_d2[s] (kMstNone: none), cand_pair[s],
// which hold the seeds' on entry; mind2[comp[s]] lowered to it.  seedmin[]: the components' smallest seeds, as the seed kernel
// left them -- this launch does not write them, so every lane of a component starts from the same bound in every run
__global__ __launch_bounds__(kBlock) void mst_nearest_kernel(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                                             const uint32_t *__restrict__ comp, const uint32_t *__restrict__ nodecomp,
                                                             const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                                             int32_t levels, int32_t n,
                                                             const unsigned long long *__restrict__ seedmin,
                                                             unsigned long long *__restrict__ mind2,
                                                             unsigned long long *__restrict__ cand_d2,
                                                             unsigned long long *__restrict__ cand_pair, MstCounters *__restrict__ ctr)
{
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < n;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const uint32_t BH64_CONSTANT *ccomp = (const uint32_t BH64_CONSTANT *)comp;
    const uint32_t BH64_CONSTANT *cidx = (const uint32_t BH64_CONSTANT *)sidx;
    const uint32_t BH64_CONSTANT *cnode = (const uint32_t BH64_CONSTANT *)nodecomp;
#pragma clang diagnostic pop

    const int32_t s = valid ? (int32_t)r : 0;
    double2 q{0.0, 0.0};
    uint32_t mine = kMstMixed, id = 0u;                  // the lane's component and caller index
    if (valid) { q = spos[s]; mine = comp[s]; id = sidx[s]; }
    double bd = (double)INFINITY;                        // best: (bd, bp); bp == kMstNone: no edge yet
    unsigned long long bp = kMstNone;
    double bound = (double)INFINITY;                     // min(bd, the component's smallest seed)
    if (valid) {
        const unsigned long long u = cand_d2[s], floor = seedmin[mine];
        bp = cand_pair[s];
        if (bp != kMstNone) bd = __longlong_as_double((long long)u);
        if (floor != kMstNone) bound = __longlong_as_double((long long)floor);
    }
    uint32_t evals = 0, skips = 0;
    const int32_t slo = s - kMstSeed, shi = s + kMstSeed;
    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool took, const NbNode &nd) {
                const uint32_t nc = cnode[nd.at];
                double unused;
                const double lb = nb_bound<false>(nd.box, q, unused);
                const bool own = took && nc == mine;
                skips += own ? 1u : 0u;
                return took && !own && !(lb > bound);
            },
            [&](const bool in, const int32_t j, const double px, const double py) {
                const uint32_t cj = ccomp[j], ij = cidx[j];
                const double dx = px - q.x, dy = py - q.y;
                if (in && cj != mine && (j < slo || j > shi)) {
                    const double d = dx * dx + dy * dy;
                    const unsigned long long pr = mst_pair(id, ij);
                    ++evals;
                    if (mst_before(d, pr, bd, bp)) { bd = d; bp = pr; }
                }
            },
            [&] { bound = (bd < bound) ? bd : bound; });

    const bool have = valid && bp != kMstNone;
    const unsigned long long bits = have ? (unsigned long long)__double_as_longlong(bd) : kMstNone;
    if (valid) { cand_d2[s] = bits; cand_pair[s] = bp; }
    mst_send(mind2, mine, bits);
    const unsigned long long e = grp_wave_sum(evals), k = grp_wave_sum(skips);
    if (lane == 0) {
        if (e) atomicAdd(&ctr->evals, e);
        if (k) atomicAdd(&ctr->skips, k);
    }
}

// the lanes whose candidate has the component's smallest d2 send its pair
__global__ __launch_bounds__(kBlock) void mst_pick_kernel(const uint32_t *__restrict__ comp, const unsigned long long *__restrict__ mind2,
                                                          const unsigned long long *__restrict__ cand_d2,
                                                          const unsigned long long *__restrict__ cand_pair, int32_t n,
                                                          unsigned long long *__restrict__ minpair)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const unsigned long long d = cand_d2[s];
    const uint32_t c = comp[s];
    if (d != kMstNone && d == mind2[c]) atomicMin(minpair + c, cand_pair[s]);
}

// every component with a chosen edge unites its two ends; the edge is appended iff this call hooked (room for n edges)
__global__ __launch_bounds__(kBlock) void mst_hook_kernel(const uint32_t *__restrict__ comp, const uint32_t *__restrict__ inv,
                                                          const unsigned long long *__restrict__ mind2,
                                                          const unsigned long long *__restrict__ minpair, int32_t n,
                                                          uint32_t *__restrict__ parent, unsigned long long *__restrict__ edge_pair,
                                                          unsigned long long *__restrict__ edge_d2, MstCounters *__restrict__ ctr)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n || comp[s] != (uint32_t)s) return;
    const unsigned long long pr = minpair[s];
    if (pr == kMstNone) return;
    const uint32_t lo = (uint32_t)(pr >> 24), hi = (uint32_t)(pr & 0xffffffull);
    if (lo >= (uint32_t)n || hi >= (uint32_t)n) return;
    uint32_t hooks = 0;
    grp_union(parent, inv[lo], inv[hi], hooks);
    if (hooks == 0) return;
    const unsigned long long k = atomicAdd(&ctr->edges, 1ull);
    if (k < (unsigned long long)n) { edge_pair[k] = pr; edge_d2[k] = mind2[s]; }
}

// comp[s] = the root of s; *roots += the roots; the per-component words reset
__global__ __launch_bounds__(kBlock) void mst_flatten_kernel(const uint32_t *__restrict__ parent, int32_t n, uint32_t *__restrict__ comp,
                                                             unsigned long long *__restrict__ seedmin,
                                                             unsigned long long *__restrict__ mind2,
                                                             unsigned long long *__restrict__ minpair,
                                                             unsigned long long *__restrict__ roots)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool is_root = false;
    if (s < n) {
        uint32_t x = comp[s];
        for (;;) { const uint32_t p = parent[x]; if (p == x) break; x = p; }
        comp[s] = x;
        is_root = x == (uint32_t)s;
        seedmin[s] = kMstNone;
        mind2[s] = kMstNone;
        minpair[s] = kMstNone;
    }
    const unsigned long long votes = __ballot(is_root);
    if (lane_id() == 0 && votes) atomicAdd(roots, (unsigned long long)__popcll(votes));
}

// order[k] = k: the payload of the final sort's first pass
__global__ __launch_bounds__(kBlock) void mst_iota_kernel(int32_t count, uint32_t *__restrict__ order)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < count) order[k] = (uint32_t)k;
}

// out[k] = pair[order[k]]: the pairs in the sorted order of their d2
__global__ __launch_bounds__(kBlock) void mst_gather_kernel(const uint32_t *__restrict__ order, const unsigned long long *__restrict__ pair,
                                                            int32_t count, unsigned long long *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const uint32_t o = order[k];
    out[k] = (o < (uint32_t)count) ? pair[o] : kMstNone;
}

// The spanning tree of set blockIdx.x: the k bodies members[set * k ..] (caller indices; slot_of: caller index -> slot of pos,
// nullptr: identity), k - 1 edges (pair, d2) in the order Prim's algorithm adds them from item 0.  *bad |= 1 when a member's
// position is not finite.  Dynamic LDS: 36 * k bytes.
template <typename Real2>
__global__ __launch_bounds__(kWave) void mst_subset_kernel(const Real2 *__restrict__ pos, const uint32_t *__restrict__ slot_of,
                                                           const int64_t *__restrict__ members, int32_t k,
                                                           unsigned long long *__restrict__ out_pair, double *__restrict__ out_d2,
                                                           uint32_t *__restrict__ bad)
{
    extern __shared__ double mst_lds[];
    double *X = mst_lds, *Y = X + k, *D = Y + k;
    unsigned long long *P = reinterpret_cast<unsigned long long *>(D + k);
    uint32_t *ID = reinterpret_cast<uint32_t *>(P + k);
    const int lane = lane_id();
    const int64_t set = blockIdx.x;
    const int64_t *row = members + set * k;

    bool notfinite = false;
#pragma unroll
    for (int i = 0; i < kMstItems; ++i) {
        const int t = lane + i * kWave;
        if (t < k) {
            const int64_t m = row[t];
            const Real2 p = pos[slot_of ? (int64_t)slot_of[m] : m];
            const double x = (double)p.x, y = (double)p.y;
            notfinite |= !(map_finite(x) && map_finite(y));
            X[t] = x; Y[t] = y; ID[t] = (uint32_t)m;
            D[t] = (double)INFINITY; P[t] = kMstNone;
        }
    }
    if (__ballot(notfinite) != 0ull && lane == 0) atomicOr(bad, 1u);
    __syncthreads();                                       // (one wavefront: X, Y and ID are read across lanes from here on)

    uint32_t intree = (lane == 0) ? 1u : 0u;              // bit i: item lane + 64 i is in the tree
    int cur = 0;
    for (int step = 0; step + 1 < k; ++step) {
        const double cx = X[cur], cy = Y[cur];
        const uint32_t cid = ID[cur];
        double bd = (double)INFINITY;
        unsigned long long bp = kMstNone;
        int bt = -1;
#pragma unroll
        for (int i = 0; i < kMstItems; ++i) {
            const int t = lane + i * kWave;
            if (t < k && ((intree >> i) & 1u) == 0u) {
                const double dx = X[t] - cx, dy = Y[t] - cy;
                const double d = dx * dx + dy * dy;
                const unsigned long long pr = mst_pair(cid, ID[t]);
                double kd = D[t];
                unsigned long long kp = P[t];
                if (mst_before(d, pr, kd, kp)) { kd = d; kp = pr; D[t] = d; P[t] = pr; }
                if (mst_before(kd, kp, bd, bp)) { bd = kd; bp = kp; bt = t; }
            }
        }
#pragma unroll
        for (int w = 1; w < kWave; w <<= 1) {
            const double od = __shfl_xor(bd, w, kWave);
            const unsigned long long op = __shfl_xor(bp, w, kWave);
            const int ot = __shfl_xor(bt, w, kWave);
            if (mst_before(od, op, bd, bp)) { bd = od; bp = op; bt = ot; }
        }
        if (bt < 0) break;                                 // (a position that is not finite: flagged above; wave-uniform)
        if (lane == 0) {
            out_pair[set * (k - 1) + step] = bp;
            out_d2[set * (k - 1) + step] = bd;
        }
        cur = bt;
        if ((cur & (kWave - 1)) == lane) intree |= 1u << (cur >> 6);
    }
}

}  // namespace bh
