// bh_binaries.hpp -- bound pairs of the current state and their Keplerian elements (bh_binaries, bh_binaries_catalogue).  The
// reference has no such output.  Included by bh_engine.hip after bh_neighbours.hpp (and bh_groups.hpp, whose wave sum it uses), so
// it is compiled with -ffp-contract=off: nothing below is fused, and fp64 sqrt and division are the correctly rounded ones.
//
// Definition.  For bodies i != j, in fp64 (an fp32 state is widened first, which is exact), G the context's:
//   dx = x_j - x_i, dy = y_j - y_i, d2 = dx * dx + dy * dy                      (the d2 of bh_count_within)
//   ux = vx_j - vx_i, uy = vy_j - vy_i, v2 = ux * ux + uy * uy
//   M = m_i + m_j,  eps_ij = 0.5 * v2 - (G * M) / sqrt(d2)                      (two-body energy per unit reduced mass)
// eps_ij and eps_ji are the same bits: the differences change sign only, and + commutes.  The engine's Plummer softening does
// not enter: the elements are Keplerian.
//   candidates of i   all j != i with 0 < d2 <= R2 = R * R and eps_ij < 0 (the upper edge inclusive as in bh_count_within;
//                     coincident bodies are never candidates of each other; a NaN velocity or mass makes every comparison
//                     false, so such a body is nobody's candidate and has none)
//   partner p(i)      the candidate first in the strict total order (eps_ij, caller index j); none: -1 with eps = +inf
//   binary            lo < hi (caller indices) with p(lo) == hi and p(hi) == lo
//
// Structure: the index of bh_neighbours.hpp as nb_build leaves it (spos, sidx, slot, boxes, off, levels), and beside it, built by
// this call alone (the other queries' build keeps its launches):
//   bin_gather_kernel    svel[s], smass[s]: velocity and mass of the s-th sorted body, through the slot permutation of
//                        nb_gather_kernel
//   bin_nodemass_kernel  nodemass[], laid out like boxes[] (as nodecomp[] of bh_mst.hpp): the largest mass under every node,
//                        leaves first, then level by level.  The maximum is m > mx ? m : mx from -inf: a NaN mass never becomes a
//                        node's bound (it would open or close nodes it says nothing about); a node of NaN masses only keeps -inf.
//
// bin_search_kernel: a visitor on nb_walk, one lane per body in sorted order, 256-thread workgroups.  The lane carries
// (best_eps, best_id), from (0, none), and accepts body j when
//   0 < d2 && d2 <= R2 && eps < 0 && (eps < best_eps || (eps == best_eps && id_j < best_id)).
// It DROPS a node only when one of these holds -- drop conditions, so that a NaN bound opens the node:
//   lb > R2         lb is nb_bound's: every body of the node has d2 >= lb as computed (the argument stands with nb_walk)
//   B >= 0
//   B > best_eps    strictly: at equality a body with a smaller caller index can still enter
// with B = 0.5 * kv - (G * (m_i + nodemass)) / sqrt(lb) and kv = 0.
//
// Why pruning on B is exact.  Rounded +, *, / and sqrt are monotone (x <= y gives op(x) <= op(y) in each argument, the sign
// of the other fixed).  Let j be a body of the node that is a candidate, so eps_ij < 0, which needs G * M_ij > 0 (else
// eps_ij = 0.5 * v2 - (something <= 0) >= 0).  m_j <= nodemass gives M_ij = m_i + m_j <= m_i + nodemass as computed; G > 0 gives
// G * M_ij <= G * (m_i + nodemass), both > 0; d2 >= lb gives sqrt(d2) >= sqrt(lb) >= 0; a positive numerator that grows over a
// denominator that shrinks gives (G * M_ij) / sqrt(d2) <= (G * (m_i + nodemass)) / sqrt(lb) = Q; and v2 >= 0 gives
// 0.5 * v2 >= 0 = 0.5 * kv, so eps_ij = 0.5 * v2 - (G * M_ij) / sqrt(d2) >= 0 - Q = B, every step as computed.  Hence: B >= 0
// leaves no candidate in the node; B > best_eps leaves none that would replace the lane's best, whatever its index.  A body
// that is no candidate is never accepted, so a bound that does not hold for it costs nothing.  lb == 0 makes Q = +inf (B = -inf)
// or 0 / 0 (NaN): neither satisfies a drop condition, the node is opened.  A NaN m_i makes B NaN everywhere: the lane opens all
// that lb <= R2 leaves it and accepts nobody.  So neither kNbLeaf, the keys nor the order of the traversal can change a partner:
// they decide only how many energies are computed.
//
// Seeding.  Before the traversal the lane looks at the sorted positions s +- kNbLeaf (itself has d2 = 0 and is no candidate),
// and the traversal skips those positions, as nb_knn_kernel does: best_eps is then that of a near body before the first box is
// tested.  The seed width is a choice that was not measured.
//
// The scalar cache is not coherent with stores of the running kernel: everything the search reads through the scalar unit --
// boxes, off, nodemass, spos, svel, smass, sidx -- was written by an EARLIER launch.
//
// bin_pairs_kernel: one lane per sorted body; where the lane's partner names the lane back and the lane has the smaller caller
// index, it appends one record (lo, hi, the eleven elements below) at the next free place (one atomic per wave).  The order of
// the places is that of the atomics; the host puts the records in ascending lo, which is the order of the catalogue (a body is
// lo of at most one pair: no ties).  With i = lo, j = hi:
//   mu = G * M;  r = sqrt(d2);  eps as above
//   a = mu / (-2.0 * eps)
//   h = dx * uy - dy * ux
//   e = sqrt(max(1.0 + ((2.0 * eps) * (h * h)) / (mu * mu), 0.0))                (max(x, 0) is x > 0 ? x : 0)
//   period = 6.283185307179586 * sqrt(((a * a) * a) / mu)
//   binding = -(((m_i * m_j) / M) * eps)
//   com = ((m_i * x_i + m_j * x_j) / M, same in y);  velocity likewise
// A record: r, eps, a, e, period, binding, M, com x, com y, velocity x, velocity y.
//
// Counters (BinCounters; stats of bh_binaries): energies computed in all and by the busiest lane, nodes opened, pairs -- the same
// in every run: every decision rests on arrays an earlier launch completed and on the lane's own best.
#pragma once

#include "bh_groups.hpp"

namespace bh {

constexpr int kBinRecord = 11;                    // doubles of a catalogue record
constexpr uint32_t kBinNone = ~0u;                // no partner yet (above every caller index)

struct BinCounters { unsigned long long evals, max_evals, opened, pairs; };

__device__ __forceinline__ uint32_t bin_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_xor(v, d, kWave);
        v = (o > v) ? o : v;
    }
    return v;
}

// eps_ij of the header from the differences and the two masses
__device__ __forceinline__ double bin_eps(double d2, double ux, double uy, double mi, double mj, double G)
{
    const double v2 = ux * ux + uy * uy;
    const double M = mi + mj;
    return 0.5 * v2 - (G * M) / sqrt(d2);
}

// svel[s], smass[s] = velocity and mass of the body in slot[s], widened
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void bin_gather_kernel(const Real2 *__restrict__ vel, const Real *__restrict__ mass,
                                                            const uint32_t *__restrict__ slot, int64_t n, double2 *__restrict__ svel,
                                                            double *__restrict__ smass)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t b = slot[s];
    const Real2 v = vel[b];
    svel[s] = double2{(double)v.x, (double)v.y};
    smass[s] = (double)mass[b];
}

// one level of mass bounds (`count` nodes): level 0 from smass[] of the leaf's bodies, a level above from the `below` nodes of
// `down`
__global__ __launch_bounds__(kBlock) void bin_nodemass_kernel(const double *__restrict__ smass, const double *__restrict__ down,
                                                              int32_t level, int32_t below, int32_t n, int32_t count,
                                                              double *__restrict__ up)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    double mx = -(double)INFINITY;
    if (level == 0) {
        const int64_t first = i * kNbLeaf;
        const int64_t last = (first + kNbLeaf < n) ? first + kNbLeaf : (int64_t)n;
        for (int64_t j = first; j < last; ++j) { const double m = smass[j]; mx = (m > mx) ? m : mx; }
    } else {
        for (int k = 0; k < 4; ++k) {
            if (4 * i + k >= below) break;
            const double m = down[4 * i + k];
            mx = (m > mx) ? m : mx;
        }
    }
    up[i] = mx;
}

// the partner of the body at sorted position s: partner[sidx[s]] (caller index, -1: none), eps[sidx[s]] (+inf: none), and
// psort[s], the partner's sorted position (-1: none)
__global__ __launch_bounds__(kBlock) void bin_search_kernel(const double2 *__restrict__ spos, const double2 *__restrict__ svel,
                                                            const double *__restrict__ smass, const uint32_t *__restrict__ sidx,
                                                            const double *__restrict__ nodemass, const NbBox *__restrict__ boxes,
                                                            const int32_t *__restrict__ off, int32_t levels, int32_t n, double R2,
                                                            double G, int64_t *__restrict__ partner, double *__restrict__ eps_out,
                                                            int32_t *__restrict__ psort, BinCounters *__restrict__ ctr)
{
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < n;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const double2 BH64_CONSTANT *cvel = (const double2 BH64_CONSTANT *)svel;
    const double BH64_CONSTANT *cmass = (const double BH64_CONSTANT *)smass;
    const uint32_t BH64_CONSTANT *cidx = (const uint32_t BH64_CONSTANT *)sidx;
    const double BH64_CONSTANT *cnode = (const double BH64_CONSTANT *)nodemass;
#pragma clang diagnostic pop

    const int32_t s = valid ? (int32_t)r : 0;
    double2 q{0.0, 0.0}, w{0.0, 0.0};
    double mi = 0.0;
    if (valid) { q = spos[s]; w = svel[s]; mi = smass[s]; }
    double best = 0.0;                                   // (best, bid): the lane's partner so far; bid == kBinNone: none
    uint32_t bid = kBinNone;
    int32_t bj = -1;                                     // its sorted position
    uint32_t evals = 0, opened = 0;

    const int32_t slo = s - kNbLeaf, shi = s + kNbLeaf;  // the seeds: the traversal skips them
    if (valid) {
        const int32_t j1 = (shi < n - 1) ? shi : n - 1;
        for (int32_t j = (slo > 0) ? slo : 0; j <= j1; ++j) {
            const double2 p = spos[j], v = svel[j];
            const double dx = p.x - q.x, dy = p.y - q.y;
            const double d2 = dx * dx + dy * dy;
            if (d2 > 0.0 && d2 <= R2) {
                const double e = bin_eps(d2, v.x - w.x, v.y - w.y, mi, smass[j], G);
                const uint32_t id = sidx[j];
                ++evals;
                if (e < 0.0 && (e < best || (e == best && id < bid))) { best = e; bid = id; bj = j; }
            }
        }
    }

    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool mine, const NbNode &nd) {
                const double nm = cnode[nd.at];
                double unused;
                const double lb = nb_bound<false>(nd.box, q, unused);
                const double B = 0.0 - (G * (mi + nm)) / sqrt(lb);             // (0.5 * kv with kv = 0)
                const bool open = mine && !(lb > R2) && !(B >= 0.0) && !(B > best);
                opened += open ? 1u : 0u;
                return open;
            },
            [&](const bool in, const int32_t j, const double px, const double py) {
                const uint32_t id = cidx[j];
                const double mj = cmass[j];
                const double vx = cvel[j].x, vy = cvel[j].y;
                const double dx = px - q.x, dy = py - q.y;
                const double d2 = dx * dx + dy * dy;
                if (in && (j < slo || j > shi) && d2 > 0.0 && d2 <= R2) {
                    const double e = bin_eps(d2, vx - w.x, vy - w.y, mi, mj, G);
                    ++evals;
                    if (e < 0.0 && (e < best || (e == best && id < bid))) { best = e; bid = id; bj = j; }
                }
            });

    if (valid) {
        const uint32_t me = sidx[s];
        const bool have = bid != kBinNone;
        partner[me] = have ? (int64_t)bid : (int64_t)-1;
        eps_out[me] = have ? best : (double)INFINITY;
        psort[s] = bj;
    }
    const unsigned long long e = grp_wave_sum(evals), o = grp_wave_sum(opened);
    const unsigned long long most = bin_wave_max(evals);
    if (lane == 0) {
        if (e) atomicAdd(&ctr->evals, e);
        if (o) atomicAdd(&ctr->opened, o);
        if (most) atomicMax(&ctr->max_evals, most);
    }
}

// the mutual pairs: where psort[psort[s]] == s and sidx[s] is the smaller caller index, the record of (lo, hi) = (sidx[s],
// sidx[psort[s]]) is appended at the next free place below `room`; the lanes of a wave take their places with one atomic
__global__ __launch_bounds__(kBlock) void bin_pairs_kernel(const double2 *__restrict__ spos, const double2 *__restrict__ svel,
                                                           const double *__restrict__ smass, const uint32_t *__restrict__ sidx,
                                                           const int32_t *__restrict__ psort, int32_t n, double G, int64_t room,
                                                           uint32_t *__restrict__ rec_lo, uint32_t *__restrict__ rec_hi,
                                                           double *__restrict__ rec, BinCounters *__restrict__ ctr)
{
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t t = -1;
    uint32_t lo = 0u, hi = 0u;
    bool have = false;
    if (s < n) {
        t = psort[s];
        if (t >= 0 && t < n && psort[t] == (int32_t)s) {
            lo = sidx[s]; hi = sidx[t];
            have = lo < hi;
        }
    }
    const unsigned long long votes = __ballot(have);
    if (votes == 0ull) return;
    const int leader = __builtin_ctzll(votes);
    unsigned long long base = 0ull;
    if (lane == leader) base = atomicAdd(&ctr->pairs, (unsigned long long)__popcll(votes));
    base = __shfl(base, leader, kWave);
    if (!have) return;
    const unsigned long long k = base + (unsigned long long)__popcll(votes & ((1ull << lane) - 1ull));
    if (k >= (unsigned long long)room) return;
    const double2 pi = spos[s], pj = spos[t], vi = svel[s], vj = svel[t];
    const double mi = smass[s], mj = smass[t];
    const double dx = pj.x - pi.x, dy = pj.y - pi.y, d2 = dx * dx + dy * dy;
    const double ux = vj.x - vi.x, uy = vj.y - vi.y, v2 = ux * ux + uy * uy;
    const double M = mi + mj;
    const double mu = G * M;
    const double r = sqrt(d2);
    const double eps = 0.5 * v2 - mu / r;
    const double a = mu / (-2.0 * eps);
    const double h = dx * uy - dy * ux;
    const double e2 = 1.0 + ((2.0 * eps) * (h * h)) / (mu * mu);
    const double e = sqrt((e2 > 0.0) ? e2 : 0.0);
    const double period = 6.283185307179586 * sqrt(((a * a) * a) / mu);
    const double binding = -(((mi * mj) / M) * eps);
    rec_lo[k] = lo;
    rec_hi[k] = hi;
    double *out = rec + k * kBinRecord;
    out[0] = r; out[1] = eps; out[2] = a; out[3] = e; out[4] = period; out[5] = binding; out[6] = M;
    out[7] = (mi * pi.x + mj * pj.x) / M; out[8] = (mi * pi.y + mj * pj.y) / M;
    out[9] = (mi * vi.x + mj * vj.x) / M; out[10] = (mi * vi.y + mj * vj.y) / M;
}

}  // namespace bh
