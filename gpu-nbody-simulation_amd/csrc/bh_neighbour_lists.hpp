// bh_neighbour_lists.hpp -- fixed-radius neighbour lists of the current state (bh_neighbour_lists): for every query the bodies
// with d2 <= r2, each row ascending in (d2, caller index).  The reference has no such query.  Included by bh_engine.hip after
// bh_neighbours.hpp, so it is compiled with -ffp-contract=off: nothing below is fused.
//
// Distance, queries and self-exclusion: those of bh_count_within (bh_neighbours.hpp); the radius may differ from query to query.
// Structure and traversal: the index of nb_build and nb_walk, one lane per query in the launch's sorted order.
//
// The answer's size is not known before the search, so there are two traversals:
//   count   nbl_count_kernel: nb_count_kernel's visitor with the lane's own r2 -- a node is dropped when lb > r2 and taken whole,
//           unopened, when ub <= r2.  Row lengths in launch order.
//   scan    nbl_scan_*: the exclusive prefix of a launch's row lengths as int64 write cursors (tile totals, their scan by one
//           workgroup, the tiles again with their bases; block_exclusive_sum of bh_prims.hpp).
//   fill    nbl_fill_kernel: prunes on lb <= r2 only and takes no node whole; every body with d2 <= r2 is an entry
//           (d2 bits, caller index).
// Why the two agree.  nb_walk's comment proves lb <= d2 <= ub for every body of a box, as computed.  The count drops a node only
// when lb > r2: none of its bodies has d2 <= r2; it takes a node whole only when ub <= r2: all of them have.  Otherwise both
// passes open the node and test the same d2 <= r2 on the same bodies.  So the count is the number of bodies with d2 <= r2 (self
// left out by index in both), which is what the fill pass meets, whatever either of them opened on the way.  The fill pass still
// guards every store with cursor < row end and reports a refused store or a row that ends short (NblCounters): it never writes
// past a row.
//
// Rows in order.  d2 >= +0 (a sum of two squares, never -0, never NaN for finite positions), so its bit pattern orders as an
// unsigned integer; a caller index is unique in a row, so (d2 bits, index) is a strict total order and every tier gives the
// same bytes:
//   <= kNblSmall entries   kept sorted while they are filled, in the lane's LDS list (NbList of the knn kernel with k = the
//                          row's known length), written out after the traversal;
//   <= BH_LISTS_SORT_LDS   nbl_sort_kernel<false>: one workgroup per row, a bitonic network in LDS over the row padded with
//                          (~0, ~0) to a power of two;
//   longer                 nbl_sort_kernel<true>: the same network on tiles of the row, then merge passes by rank between the
//                          row and its place in a second buffer of global memory: an entry's place in the merged run is its
//                          place in its own run plus the number of entries of the sibling run below it (a binary search; no
//                          ties, so no rule for them).
// A row's bytes depend on its own entries only.
#pragma once

#include "bh_neighbours.hpp"

namespace bh {

#ifndef BH_NBL_SMALL
#define BH_NBL_SMALL 8                  // (measured against 1, 2, 4, 16 and 32 in A/B builds: DESIGN.md section 28)
#endif
constexpr int kNblSmall = BH_NBL_SMALL; // rows up to here are kept in order in the fill pass's LDS lists
static_assert(kNblSmall >= 1 && kNblSmall <= kNbMaxK, "the fill pass's lists are the knn kernel's");
constexpr int kNblMaxLds = 4096;        // most entries the bitonic network holds: 12 bytes each, 48 KiB
constexpr int kNblScanItems = 8;        // row lengths per thread of a scan tile
constexpr int kNblScanTile = kBlock * kNblScanItems;

// what the fill pass leaves beside the entries; refused and cut must be 0
struct NblCounters {
    unsigned long long refused;         // stores at or past a row's end (not made)
    unsigned long long cut;             // rows that ended short of their length
    unsigned long long evals;           // distances computed
    unsigned long long opened;          // nodes opened, summed over the lanes
};

template <> __device__ __forceinline__ uint64_t zero_of<uint64_t>() { return 0; }

// the sum of a value over the wave, in every lane
__device__ __forceinline__ unsigned long long nbl_wave_sum(uint64_t v)
{
    const uint64_t inc = wave_inclusive_sum<uint64_t>(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inc, kWave - 1);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(inc >> 32), kWave - 1);
    return ((unsigned long long)hi << 32) | lo;
}

// the queries of rows [0, nq) of a launch: row r is the body at sorted position s0 + r (POINTS false), or the point
// points[order[r]].  q, self, and the lane's r2: rad2[caller index of the query] (rad2 null: r2_all)
template <bool POINTS>
__device__ __forceinline__ void nbl_query(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                          const double2 *__restrict__ points, const uint32_t *__restrict__ order, int64_t s0, int64_t r,
                                          const double *__restrict__ rad2, double r2_all, double2 &q, int32_t &self, double &r2)
{
    if (POINTS) {
        const uint32_t o = order[r];
        q = points[o];
        self = -1;
        r2 = rad2 ? rad2[o] : r2_all;
    } else {
        self = (int32_t)(s0 + r);
        q = spos[self];
        r2 = rad2 ? rad2[sidx[self]] : r2_all;
    }
}

// counts[r]: the bodies with d2 <= the row's r2 (nb_count_kernel with a per-lane r2)
template <bool POINTS>
__global__ __launch_bounds__(kBlock) void nbl_count_kernel(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                                           const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                                           int32_t levels, int32_t n, const double2 *__restrict__ points,
                                                           const uint32_t *__restrict__ order, int64_t s0, int64_t nq,
                                                           const double *__restrict__ rad2, double r2_all,
                                                           uint32_t *__restrict__ counts)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < nq;
    double2 q{0.0, 0.0};
    int32_t self = -1;
    double r2 = 0.0;
    if (valid) nbl_query<POINTS>(spos, sidx, points, order, s0, r, rad2, r2_all, q, self, r2);
    uint32_t cnt = 0;
    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool mine, const NbNode &nd) {
                double ub;
                const double lb = nb_bound<true>(nd.box, q, ub);
                const bool in = mine && lb <= r2;
                const bool whole = in && ub <= r2;
                if (whole) cnt += (uint32_t)(nd.last - nd.first) - ((self >= nd.first && self < nd.last) ? 1u : 0u);
                return in && !whole;
            },
            [&](const bool rest, const int32_t j, const double px, const double py) {
                const double dx = px - q.x, dy = py - q.y;
                if (rest && j != self && dx * dx + dy * dy <= r2) ++cnt;
            });
    if (valid) counts[r] = cnt;
}

// ---- the scan: cursors[r] = counts[0] + ... + counts[r - 1] over the nq rows of a launch, in 64 bits
__device__ __forceinline__ uint64_t nbl_tile_items(const uint32_t *__restrict__ counts, int64_t nq, int64_t first,
                                                uint32_t (&v)[kNblScanItems])
{
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kNblScanItems; ++k) {
        v[k] = (first + k < nq) ? counts[first + k] : 0u;
        sum += v[k];
    }
    return sum;
}

__global__ __launch_bounds__(kBlock) void nbl_scan_totals_kernel(const uint32_t *__restrict__ counts, int64_t nq,
                                                                 uint64_t *__restrict__ tiles)
{
    __shared__ uint64_t sh[kWavesPerBlock + 1];
    uint32_t v[kNblScanItems];
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kNblScanItems;
    uint64_t total;
    (void)block_exclusive_sum<uint64_t>(nbl_tile_items(counts, nq, first, v), sh, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// one workgroup: tiles[t] becomes the sum of the tiles before t
__global__ __launch_bounds__(kBlock) void nbl_scan_bases_kernel(uint64_t *__restrict__ tiles, int32_t nt)
{
    __shared__ uint64_t sh[kWavesPerBlock + 1];
    uint64_t carry = 0;
    for (int32_t t0 = 0; t0 < nt; t0 += kBlock) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        const uint64_t v = (t < nt) ? tiles[t] : (uint64_t)0;
        uint64_t total;
        const uint64_t ex = block_exclusive_sum<uint64_t>(v, sh, total);
        if (t < nt) tiles[t] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kBlock) void nbl_scan_apply_kernel(const uint32_t *__restrict__ counts, int64_t nq,
                                                                const uint64_t *__restrict__ tiles,
                                                                int64_t *__restrict__ cursors)
{
    __shared__ uint64_t sh[kWavesPerBlock + 1];
    uint32_t v[kNblScanItems];
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kNblScanItems;
    uint64_t total;
    uint64_t at = block_exclusive_sum<uint64_t>(nbl_tile_items(counts, nq, first, v), sh, total) + tiles[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kNblScanItems; ++k) {
        if (first + k < nq) cursors[first + k] = (int64_t)at;
        at += v[k];
    }
}

// ---- the fill pass.  Row r of the launch owns ent[cursors[r] .. cursors[r] + counts[r]).  A row of up to kNblSmall entries is
// collected in the lane's LDS list in order and written out at the end; a longer one is stored as it is met (the sort kernels
// order it).  Dynamic LDS: kl * kWave * 12 bytes, kl >= the longest row of the launch that is no longer than kNblSmall (>= 1).
// evals[r]: the bodies whose d2 the lane computed.
template <bool POINTS>
__global__ __launch_bounds__(kWave) void nbl_fill_kernel(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                                         const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                                         int32_t levels, int32_t n, int32_t kl, const double2 *__restrict__ points,
                                                         const uint32_t *__restrict__ order, int64_t s0, int64_t nq,
                                                         const double *__restrict__ rad2, double r2_all,
                                                         const uint32_t *__restrict__ counts, const int64_t *__restrict__ cursors,
                                                         unsigned long long *__restrict__ ent_d2, uint32_t *__restrict__ ent_idx,
                                                         uint32_t *__restrict__ evals, NblCounters *__restrict__ ctr)
{
    extern __shared__ double nbl_list_lds[];
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * kWave + lane;
    const bool valid = r < nq;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const uint32_t BH64_CONSTANT *cidx = (const uint32_t BH64_CONSTANT *)sidx;
#pragma clang diagnostic pop

    double2 q{0.0, 0.0};
    int32_t self = -1;
    double r2 = 0.0;
    int64_t cur = 0, end = 0;
    if (valid) {
        nbl_query<POINTS>(spos, sidx, points, order, s0, r, rad2, r2_all, q, self, r2);
        cur = cursors[r];
        end = cur + (int64_t)counts[r];
    }
    const int64_t len = end - cur;
    const bool small = len <= (int64_t)kNblSmall;
    NbList list;
    list.D = nbl_list_lds + lane;
    list.I = reinterpret_cast<uint32_t *>(nbl_list_lds + (size_t)kl * kWave) + lane;
    list.k = small ? (int)((len < kl) ? len : kl) : 0;       // (kl covers it; a list never leaves its LDS)
    list.cnt = 0; list.kd2 = (double)INFINITY; list.kid = 0u;

    uint32_t ev = 0, opened = 0, refused = 0;
    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool mine, const NbNode &nd) {
                double unused;
                const double lb = nb_bound<false>(nd.box, q, unused);
                const bool in = mine && lb <= r2;
                opened += in ? 1u : 0u;
                return in;
            },
            [&](const bool rest, const int32_t j, const double px, const double py) {
                const uint32_t id = cidx[j];
                const double dx = px - q.x, dy = py - q.y;
                const double d = dx * dx + dy * dy;
                if (rest && j != self) {
                    ++ev;
                    if (d <= r2) {
                        if (small) {
                            if (list.cnt < list.k) list.insert(d, id); else ++refused;
                        } else if (cur < end) {
                            ent_d2[cur] = (unsigned long long)__double_as_longlong(d);
                            ent_idx[cur] = id;
                            ++cur;
                        } else {
                            ++refused;
                        }
                    }
                }
            });

    if (valid && small) {
        for (int e = 0; e < list.cnt; ++e) {
            ent_d2[cur] = (unsigned long long)__double_as_longlong(list.D[e * kWave]);
            ent_idx[cur] = list.I[e * kWave];
            ++cur;
        }
    }
    if (valid) evals[r] = ev;
    const unsigned long long bad = nbl_wave_sum(refused), cut = nbl_wave_sum((valid && cur != end) ? 1ull : 0ull);
    const unsigned long long evs = nbl_wave_sum(ev), ops = nbl_wave_sum(opened);
    if (lane == 0) {
        if (bad) atomicAdd(&ctr->refused, bad);
        if (cut) atomicAdd(&ctr->cut, cut);
        atomicAdd(&ctr->evals, evs);
        atomicAdd(&ctr->opened, ops);
    }
}

// ---- the row sorts: workgroup b sorts row rows[b] of the launch
__device__ __forceinline__ bool nbl_less(unsigned long long da, uint32_t ia, unsigned long long db, uint32_t ib)
{
    return da < db || (da == db && ia < ib);
}

// the bitonic network over the T (a power of two) entries of D / I in LDS, ascending; every thread of the workgroup
__device__ __forceinline__ void nbl_bitonic(unsigned long long *D, uint32_t *I, int T)
{
    for (int k = 2; k <= T; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = (int)threadIdx.x; i < T; i += (int)blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long di = D[i], dl = D[l];
                    const uint32_t ii = I[i], il = I[l];
                    const bool up = (i & k) == 0;
                    if (nbl_less(dl, il, di, ii) == up) { D[i] = dl; I[i] = il; D[l] = di; I[l] = ii; }
                }
            }
        }
    }
    __syncthreads();
}

// the number of entries of the sorted run [lo, hi) of (d / x) that are below (kd, ki)
__device__ __forceinline__ int64_t nbl_rank(const unsigned long long *d, const uint32_t *x, int64_t lo, int64_t hi,
                                            unsigned long long kd, uint32_t ki)
{
    const int64_t first = lo;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (nbl_less(d[mid], x[mid], kd, ki)) lo = mid + 1; else hi = mid;
    }
    return lo - first;
}

// MERGE false: the row has at most T entries and is padded to its own power of two.  MERGE true: tiles of T, then merge
// passes between ent and alt (the row's own place in both).  T is a power of two; dynamic LDS: T * 12 bytes.  Workgroups of 64,
// 128 or 256 threads: the host gives short rows fewer.
template <bool MERGE>
__global__ __launch_bounds__(kBlock) void nbl_sort_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ counts,
                                                          const int64_t *__restrict__ cursors, int32_t T,
                                                          unsigned long long *ent_d2, uint32_t *ent_idx,
                                                          unsigned long long *alt_d2, uint32_t *alt_idx)
{
    extern __shared__ unsigned long long nbl_sort_lds[];
    unsigned long long *D = nbl_sort_lds;
    uint32_t *I = reinterpret_cast<uint32_t *>(nbl_sort_lds + T);
    const uint32_t row = rows[blockIdx.x];
    const int64_t base = cursors[row], len = (int64_t)counts[row];
    if (!MERGE && len > T) return;                             // (the host never lists such a row here)
    int Tr = T;                                                // the network's size: the tile, or the least power of two for the row
    if (!MERGE) { Tr = 2; while (Tr < len) Tr <<= 1; }
    const int step = (int)blockDim.x;

    for (int64_t t0 = 0; t0 < len; t0 += T) {
        const int64_t m = (len - t0 < T) ? len - t0 : T;
        __syncthreads();
        for (int i = (int)threadIdx.x; i < Tr; i += step) {
            const bool have = i < m;
            D[i] = have ? ent_d2[base + t0 + i] : ~0ull;
            I[i] = have ? ent_idx[base + t0 + i] : ~0u;
        }
        nbl_bitonic(D, I, Tr);
        for (int i = (int)threadIdx.x; i < m; i += step) {
            ent_d2[base + t0 + i] = D[i];
            ent_idx[base + t0 + i] = I[i];
        }
    }
    if (!MERGE) return;

    unsigned long long *sd = ent_d2 + base, *dd = alt_d2 + base;
    uint32_t *si = ent_idx + base, *di = alt_idx + base;
    for (int64_t w = T; w < len; w <<= 1) {
        __syncthreads();                                       // (the run's entries of the pass before are written)
        for (int64_t i = threadIdx.x; i < len; i += step) {
            const int64_t pair = i / (2 * w) * (2 * w), mid = (pair + w < len) ? pair + w : len;
            const int64_t last = (pair + 2 * w < len) ? pair + 2 * w : len;
            const unsigned long long kd = sd[i];
            const uint32_t ki = si[i];
            // (no two entries of a row are equal, so "below" needs no rule for ties)
            const int64_t at = (i < mid) ? pair + (i - pair) + nbl_rank(sd, si, mid, last, kd, ki)
                                         : pair + (i - mid) + nbl_rank(sd, si, pair, mid, kd, ki);
            dd[at] = kd;
            di[at] = ki;
        }
        unsigned long long *td = sd; sd = dd; dd = td;
        uint32_t *ti = si; si = di; di = ti;
    }
    if (sd != ent_d2 + base) {
        __syncthreads();
        for (int64_t i = threadIdx.x; i < len; i += step) { ent_d2[base + i] = sd[i]; ent_idx[base + i] = si[i]; }
    }
}

}  // namespace bh
