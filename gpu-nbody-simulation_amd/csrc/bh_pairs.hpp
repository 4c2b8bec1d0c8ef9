// bh_pairs.hpp -- pair-separation counts of the current state (bh_pair_counts): how many pairs of bodies, or of points and
// bodies, lie at each separation.  The reference has no such output.  Included by bh_engine.hip, so it is compiled with
// -ffp-contract=off: nothing below is fused.
//
// Distance: the d2 of bh_count_within (bh_neighbours.hpp): dx = x_j - q.x, dy = y_j - q.y, d2 = dx * dx + dy * dy in fp64, an
// fp32 state widened first.  It is symmetric in (i, j) bit for bit (negation is exact).
// Bins: nb + 2 of them on the squared edges e2[0 .. nb]: bin(d2) = the number of edges with e2[k] < d2 -- 0: d2 <= e2[0];
// k + 1: e2[k] < d2 <= e2[k + 1]; nb + 1: d2 > e2[nb].  The upper edge is inclusive, as in bh_count_within and bh_groups.
//
// Structure and traversal: the index of nb_build and nb_walk (bh_neighbours.hpp), one lane per query in sorted order.
//
// Why taking a node whole is exact.  Every body of a node has a computed d2 with lb <= d2 <= ub, lb and ub the two bounds of
// nb_bound<true> (the argument stands with nb_walk).  bin() is non-decreasing in d2.  So with bin(lb) == bin(ub) every body of the
// node falls in that bin, and the node's body count is added to it without opening the node.  Otherwise the node is opened;
// a leaf's bodies are binned one by one, searching upward from bin(lb), never past bin(ub).  Nodes wholly below e2[0] or wholly
// beyond e2[nb] are taken whole into the two outer counters like any other.
//
// Auto mode counts every unordered pair once, by its later member: the query at sorted position s counts the sorted positions
// < s only.  A node over the positions [first, last) holds m = clamp(s - first, 0, last - first) of them; a lane with m == 0
// drops out of the node; a leaf loop evaluates j < s only.  No self-exclusion is needed, and half the distances are.
// Late positions are the heaviest, so workgroup b takes the rows of group gridDim.x - 1 - b: the heaviest are dispatched first.
//
// Storage: dynamic LDS holds the nb + 1 squared edges, the workgroup's int64 histogram of nb + 2 bins and one evals word
// ((2 nb + 4) * 8 bytes: 16 KiB at 1,024 bins).  The histogram is filled with LDS integer atomics -- per leaf and bin, not per
// distance, where a leaf spans at most two bins; the two outer bins of whole nodes are kept in registers -- and its non-zero
// entries are flushed to memory once with ordinary vector atomics.  Integer sums are the same bits in any order.
#pragma once

#include "bh_neighbours.hpp"

namespace bh {

constexpr int kPairMaxBins = 1024;             // = BH_PAIR_MAX_BINS

// the number of edges e2[k], k in [0, nb], with e2[k] < d2, known to lie in [lo, hi]
__device__ __forceinline__ int pair_bin(const double *e2, int lo, int hi, double d2)
{
    while (lo < hi) {                                          // (at most 11 rounds)
        const int mid = (lo + hi) >> 1;
        if (e2[mid] < d2) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Rows [0, nq) of this launch: row r is the body at sorted position s0 + r (POINTS false: it counts the positions before its
// own) or the point points[order[r]] (POINTS true: it counts every body).  hist[nb + 2] += the bins, *evals += the d2 computed.
// Dynamic LDS: (2 * nb + 4) * 8 bytes.
template <bool POINTS>
__global__ __launch_bounds__(kBlock) void pair_count_kernel(const double2 *__restrict__ spos, const NbBox *__restrict__ boxes,
                                                            const int32_t *__restrict__ off, int32_t levels, int32_t n,
                                                            const double2 *__restrict__ points, const uint32_t *__restrict__ order,
                                                            int64_t s0, int64_t nq, const double *__restrict__ e2_mem, int32_t nb,
                                                            unsigned long long *__restrict__ hist, unsigned long long *__restrict__ evals)
{
    extern __shared__ unsigned long long pair_lds[];
    double *e2 = reinterpret_cast<double *>(pair_lds);         // nb + 1 squared edges
    unsigned long long *h = pair_lds + (nb + 1);               // nb + 2 bins, then the evals word
    for (int k = threadIdx.x; k <= nb; k += kBlock) e2[k] = e2_mem[k];
    for (int k = threadIdx.x; k < nb + 3; k += kBlock) h[k] = 0ull;
    __syncthreads();

#ifdef BHGPU_PAIR_FORWARD                                       // A/B builds only: workgroup b takes group b
    const int64_t group = blockIdx.x;
#else
    const int64_t group = gridDim.x - 1 - blockIdx.x;
#endif
    const int64_t r = group * kBlock + threadIdx.x;
    const bool valid = r < nq;

    double2 q{0.0, 0.0};
    int64_t s = n;                                             // bodies before the query: a point counts them all
    if (valid) {
        if (POINTS) q = points[order[r]];
        else { s = s0 + r; q = spos[s]; }
    }
    const double e2_first = e2[0], e2_last = e2[nb];
    uint32_t below = 0, beyond = 0, ev = 0;                    // (a lane meets fewer than 2^24 bodies)
    int kl = 0, ku = 0;                                        // of the node last visited: bin(lb), bin(ub) ...
    double edge = 0.0;                                         // ... e2[kl] of an opened leaf ...
    uint32_t c0 = 0, c1 = 0;                                   // ... and what it adds to the bins kl and kl + 1
    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool mine, const NbNode &nd) {
                double ub;
                const double lb = nb_bound<true>(nd.box, q, ub);
                // m of the node's bodies lie before the query
                const int64_t upto = (s < nd.last) ? s : nd.last;
                const uint32_t m = (upto > nd.first) ? (uint32_t)(upto - nd.first) : 0u;
                bool rest = false;
                kl = ku = 0;
                if (mine && m != 0u) {
                    if (ub <= e2_first) below += m;
                    else if (lb > e2_last) beyond += m;
                    else {
                        kl = pair_bin(e2, 0, nb + 1, lb);
                        ku = pair_bin(e2, kl, nb + 1, ub);
                        if (kl == ku) atomicAdd(&h[kl], (unsigned long long)m);
                        else rest = true;
                    }
                }
                if (nd.level == 0) edge = rest ? e2[kl] : 0.0;
                return rest;
            },
            [&](const bool rest, const int32_t j, const double px, const double py) {
                const double dx = px - q.x, dy = py - q.y;
                const double d2 = dx * dx + dy * dy;
                if (rest && j < s) {
                    ++ev;
                    if (!(edge < d2)) ++c0;
                    else if (ku == kl + 1 || !(e2[kl + 1] < d2)) ++c1;
                    else atomicAdd(&h[pair_bin(e2, kl + 2, ku, d2)], 1ull);
                }
            },
            [&] {
                if (c0) atomicAdd(&h[kl], (unsigned long long)c0);
                if (c1) atomicAdd(&h[kl + 1], (unsigned long long)c1);
                c0 = c1 = 0;
            });
    if (below) atomicAdd(&h[0], (unsigned long long)below);
    if (beyond) atomicAdd(&h[nb + 1], (unsigned long long)beyond);
    if (ev) atomicAdd(&h[nb + 2], (unsigned long long)ev);
    __syncthreads();
    for (int k = threadIdx.x; k < nb + 2; k += kBlock) {
        const unsigned long long v = h[k];
        if (v) atomicAdd(&hist[k], v);
    }
    if (threadIdx.x == 0 && h[nb + 2]) atomicAdd(evals, h[nb + 2]);
}

}  // namespace bh
