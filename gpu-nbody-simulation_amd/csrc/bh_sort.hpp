// bh_sort.hpp -- the sort of (key, body) pairs for the tree build.  Included by the engine translation unit
// only.  Two sorts with the same result, the stable order by key:
//
//   LSD radix sort (first build after an upload, launches above 4M bodies, exact mode): 8-bit digits, three
//   launches per pass --
//     radix_hist      : counts[digit * nblocks + block] = occurrences of digit in tile `block`
//     radix_rowscan   : one workgroup per digit: exclusive prefix along its row, row total aside
//     radix_scatter_w : base(digit, block) = exclusive scan of the 256 row totals (done in-kernel) + row
//                       prefix; stable scatter of the tile, ranks within a wave's round from a per-wave LDS
//                       table of lane masks
//   bucket sort (every later build of up to 4M bodies with packed keys; see "bucket sort" below): ONE such
//   counting pass whose digit is the key's bucket among splitters from the previous build, then
//     bucket_sort_kernel : one workgroup sorts one bucket entirely in LDS.
//
// Element order inside a tile is (wave, round, lane) = tile order and ranks follow lane order, so equal keys
// keep their input order.  (Measured and rejected in rounds 1-2, code removed in round 4: a barrier-per-round scatter and
// a look-back "onesweep" sort -- DESIGN.md section 3, profiles/r02_final; also letting every scatter workgroup derive its own offsets from the count matrix -- it re-reads the
// 256 x nblocks matrix per workgroup, 37 us per pass at N = 1M against 18 + 14 us for scatter + scan then.)
#pragma once

#include "bh_prims.hpp"

namespace bh {

#ifndef BH_SORT_ITEMS
#define BH_SORT_ITEMS 8
#endif
constexpr int kSortItems = BH_SORT_ITEMS;          // keys per thread in the sort kernels
constexpr int kSortTile = kBlock * kSortItems;
constexpr int kRadixBits = 8;

// grid = 256 workgroups (one per digit): counts[d][*] -> exclusive prefix in place, total aside
__global__ __launch_bounds__(kBlock) void radix_rowscan(uint32_t *__restrict__ counts,
                                                         uint32_t *__restrict__ row_total, int nblocks)
{
    __shared__ uint32_t sm[kWavesPerBlock + 1];
    uint32_t *row = counts + (int64_t)blockIdx.x * nblocks;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < nblocks; c0 += kBlock) {
        const int b = c0 + threadIdx.x;
        const uint32_t v = (b < nblocks) ? row[b] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_sum(v, sm, tot);
        if (b < nblocks) row[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) row_total[blockIdx.x] = carry;
}

constexpr int kRadix = 1 << kRadixBits;
static_assert(kRadix == kBlock, "one thread per digit");

// Digit width of the default sort.  10 bits (the 40-bit keys of max_depth 21 in 4 passes instead of 5)
// was measured and lost at every size: build 0.241 vs 0.215 ms at N = 1M, 0.093 vs 0.090 at 65k, 3.29 vs
// 2.80 at 16.7M -- with 1,024 digits a 2,048-key tile has two keys per digit, so the digit-sorted
// write-out degenerates into 16-byte runs and the count matrix is four times larger.
constexpr int kSortBits = 8;
// ITEMS keys per thread: 8 (tiles of 2,048) when there are enough tiles to fill the GPU, 2 (tiles of
// 512) for launches of few bodies, where a workgroup's 8 sequential rounds are pure latency.
// BITS: digit width; counts[digit * nblocks + block].
// ---- bucket sort (launches of up to kBucketMaxN bodies with packed keys) --------------------------------
// The LSD sort costs five passes of dependent short kernels (~9 us per pass at any size below 1M bodies).
// Consecutive builds sort almost the same bodies, so the engine sorts in TWO steps instead:
//   (1) ONE stable counting pass whose "digit" is the bucket of the key among 256 splitters (keys_kernel
//       derives them from the previous build's sorted positions: near-equal buckets), histogram + row scan
//       + scatter as for a radix digit;
//   (2) bucket_sort_kernel: one workgroup per bucket sorts its <= kBucketCap (16,384) keys entirely in LDS (stable
//       8-bit LSD passes over the key bits that differ inside the bucket) and writes plain keys + indices.
// The result is the stable sort by key whatever the splitters are -- they only have to be sorted, which
// keys_kernel guarantees -- so (keys_sorted, perm) is bit-identical to the LSD sort's.  A bucket that does
// not fit (bodies that moved wildly, a root box that jumped and scrambled the curve) is sorted by its
// workgroup through global memory: correct, slow, and gone at the next build.
// 256 buckets up to 1M bodies, 1,024 up to 4M (BITS = 8 / 10 in the counting pass): the average bucket stays
// at most a third of what one workgroup sorts in LDS.
constexpr int kBuckets = 256, kBucketsBig = 1024;
constexpr int kBucketStartOffset = kBucketsBig + 8;        // bsum_sort: [0, nb) bucket totals, [kBucketStartOffset, +nb) bucket starts
constexpr int kDigits = 256;                              // the in-LDS sort's own 8-bit digits
constexpr int kMaxSplitSamples = 2048;                    // sample positions sorted by keys_kernel's splitter workgroup
constexpr uint64_t kKeyMask40 = (1ull << 40) - 1;
// largest j with spl[j] <= key (spl sorted, spl[0] = 0)
template <int NB>
__device__ __forceinline__ uint32_t bucket_of(uint64_t key, const uint64_t *spl)
{
    int b = 0;
#pragma unroll
    for (int s = NB / 2; s >= 1; s >>= 1) b += (spl[b + s] <= key) ? s : 0;
    return (uint32_t)b;
}

// run-time NB (sorted spl, spl[0] = 0, nb a power of two): the same answer as bucket_of<NB>
__device__ __forceinline__ uint32_t bucket_of_n(uint64_t key, const uint64_t *spl, int nb)
{
    int b = 0;
    for (int s = nb >> 1; s >= 1; s >>= 1) b += (spl[b + s] <= key) ? s : 0;
    return (uint32_t)b;
}

// ---- direct input (fp32-tree builds whose state is in the previous sorted order) ---------------------------
// keys_kernel writes the packed keys in state order, and the state is the sorted order of a recent build: the
// array is sorted but for the few bodies that overtook a neighbour since.  The counting pass above moves all of
// it to move those few.  Direct input skips it:
//   * bucket b owns the array range [b * L, (b + 1) * L) of keys[0], L = ceil(n / nb) (the last range is shorter,
//     ranges that start at or beyond n are empty);
//   * range key j is the key, in this build's box, of the body that stands at j * L (0 for j = 0, "infinity" for an
//     empty range).  While the range keys are non-decreasing they are splitters like any others, and
//     bucket_of(key, range keys) == b  <=>  range key b <= key < range key b + 1  (stays_in below -- the ONE test
//     of keys_kernel and of bucket_sort_kernel; with equal range keys the left of the two buckets keeps nothing,
//     exactly as bucket_of routes);
//   * keys_kernel appends every key that does not stay in the bucket of its index (a "crosser") to one of kDirectSubs
//     lists, each behind a counter of its own (atomics on one word cost ~3.5 ns apiece, lists chosen by wave number
//     spread them over 64 words in 64 memory channels), and leaves keys[0] complete either way;
//   * at most T crossers in all, no list overfull, nobody said otherwise (direct_total): radix_hist and radix_scatter_w
//     return at once, and workgroup b of bucket_sort_kernel takes the keys of its range that stay plus the listed keys
//     that bucket_of sends to b, in the order of their body index (which is the order the counting pass would have
//     delivered them in: the result is the same stable sort);
//   * otherwise -- more crossers, a list that ran over, half a wave crossing at once, range keys out of order (the first
//     sample workgroup of keys_kernel looks) -- the counting pass runs as before.  The decision is a function of 65
//     words in device memory, evaluated alike by every wave of the three kernels.
// No kernel waits for another workgroup: every key workgroup forms the two or three range keys it needs itself.
constexpr int64_t kSortDirectMax = 1024;                   // default T (below where the two paths cross, by the spread)
constexpr int kDirectSubs = 64;                            // crosser lists (and counters) of an adaptive build
constexpr int kDirectCounterWords = 64 * (1 + kDirectSubs);   // one build's counters
constexpr uint32_t kDirectStride = 64;                     // words between two counters: 256 bytes, another memory channel
constexpr uint64_t kRangeKeyInf = ~0ull;                   // range key of an empty range: above every 40-bit key
struct SortDirect {
    // the counters of THIS build (zero on entry), kDirectStride words apart: word 0 is set when the counting pass has to
    // run whatever the counts, counter 1 + s belongs to list s; null: no direct input
    uint32_t *count = nullptr;
    uint32_t *count_next = nullptr; // the counters of the next build: keys_kernel clears them
    uint64_t *list = nullptr;       // [nsub][subcap] the packed keys of the crossers, in arrival order
    uint64_t *range_keys = nullptr; // [nb] written by keys_kernel's first sample workgroup
    uint32_t cap = 0;               // T: most crossers in all lists together
    uint32_t subcap = 0;            // room of one list
    uint32_t len = 0;               // L
    int nsub = 1;                   // lists (a power of two, <= 64: one lane each in direct_total)
};
// The decision, taken alike by every wave of every kernel of the build (all lanes call): the number of listed crossers, or
// ~0u when the counting pass has to run -- told so, a list overfull, or more than cap crossers in all.
// (in two halves: a kernel that has other work to start issues the loads first and decides after it, so that the build
// that takes the counting pass does not wait for them)
struct DirectWords { uint32_t v, off; };
__device__ __forceinline__ DirectWords direct_load(const uint32_t *count, int nsub)
{
    const int l = threadIdx.x & 63;
    return DirectWords{(l < nsub) ? count[kDirectStride * (1u + (uint32_t)l)] : 0u, count[0]};
}
__device__ __forceinline__ uint32_t direct_total(DirectWords w, uint32_t cap, uint32_t subcap)
{
    const uint32_t v = w.v, off = w.off;
    uint32_t total = v;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) total += (uint32_t)__shfl_xor((int)total, o);
    const bool bad = off != 0u || __ballot(v > subcap) != 0ull || total > cap;
    return bad ? ~0u : total;
}
__device__ __forceinline__ uint32_t direct_total(const uint32_t *count, int nsub, uint32_t cap, uint32_t subcap)
{
    return direct_total(direct_load(count, nsub), cap, subcap);
}
__device__ __forceinline__ bool stays_in(uint64_t key40, uint64_t lo, uint64_t hi) { return lo <= key40 && key40 < hi; }

// LDS atomics of one wave instruction that hit ONE counter are served lane after lane.  On sorted data -- the
// bucket digit of a tile, the upper bytes of the keys of a bucket -- that is every instruction of the count
// phase.  A full wave whose lanes all hold the same digit therefore adds 64 through one lane, and its ranks
// are the lane numbers (no ballot matching).
// (Used in the bucket pass only -- histogram and scatter, where a tile's keys fall into one or two buckets; in
// the byte passes of bucket_sort_kernel the test cost more on moving bodies than it saved on frozen ones:
// sort 0.051 / 0.083 ms frozen / drifting with it, 0.053 / 0.074 without, N = 1M.)
__device__ __forceinline__ bool wave_same_digit(uint32_t d, bool valid)
{
    return __ballot(valid) == ~0ull && __ballot(d != (uint32_t)__builtin_amdgcn_readfirstlane((int)d)) == 0ull;
}
// (TRY = false where digits are as good as random -- the low key bytes, every pass of the LSD sort on unsorted
// data: there the two extra ballots per key cost more than they save, LSD sort 89 -> 95 us at N = 1M.)
template <bool TRY = true>
__device__ __forceinline__ void wave_count_digit(uint32_t *row, uint32_t d, bool valid)
{
    if (TRY && wave_same_digit(d, valid)) {                     // uniform branch
        if (lane_id() == 0) atomicAdd(&row[d], (uint32_t)kWave);
    } else if (valid) {
        atomicAdd(&row[d], 1u);
    }
}

// BUCKET: the digit is the key's bucket among the splitters (shift unused)
template <int ITEMS, int BITS = kRadixBits, bool BUCKET = false>
__global__ __launch_bounds__(kBlock) void radix_hist(const uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ counts, int64_t n,
                                                      int shift, int nblocks,
                                                      const uint64_t *__restrict__ splitters = nullptr,
                                                      uint16_t *__restrict__ dig16 = nullptr,
                                                      uint32_t *__restrict__ row_total = nullptr,
                                                      const uint32_t *__restrict__ direct_count = nullptr,
                                                      uint32_t direct_cap = 0, uint32_t direct_subcap = 0, int direct_nsub = 1)
{
    DirectWords dw{0u, 1u};
    if (BUCKET && direct_count != nullptr) dw = direct_load(direct_count, direct_nsub);
    constexpr int R = 1 << BITS;
    __shared__ uint32_t h[R];
    __shared__ uint64_t spl[BUCKET ? R : 1];
    // A key value frequent enough to be sampled twice (bodies piled into one depth-cap cell) gets a bucket of
    // its own: the second of two equal splitters becomes value + 1, so [value, value + 1) holds equal keys only
    // -- already in their final order after the stable scatter, whatever their number.
    if (BUCKET)
        for (int d = threadIdx.x; d < R; d += kBlock) {
            const uint64_t v = splitters[d];
            spl[d] = (d > 0 && splitters[d - 1] == v) ? v + 1 : v;
        }
    for (int d = threadIdx.x; d < R; d += kBlock) h[d] = 0;
    __syncthreads();
    if (BUCKET && direct_count != nullptr && direct_total(dw, direct_cap, direct_subcap) != ~0u) return;   // direct input: nothing to count
    const int64_t base = (int64_t)blockIdx.x * (kBlock * ITEMS);
    uint32_t guess = 0;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        const bool valid = i < n;
        const uint64_t k = valid ? keys[i] : 0ull;
        uint32_t d;
        if (BUCKET) {
            // The bodies arrive almost in order: a key 256 places further on lies in the same bucket as the last one, or
            // the next.  Two independent LDS reads confirm that for the whole wave; the search (eight or ten
            // DEPENDENT reads) runs only where a lane's guess fails.
            const uint64_t kk = k & kKeyMask40;
            bool ok = false;
            if (r > 0) ok = spl[guess] <= kk && (guess + 1 == (uint32_t)R || kk < spl[guess + 1]);
            if (r > 0 && __ballot(valid && !ok) == 0ull) d = guess;   // uniform
            else d = bucket_of<R>(kk, spl);
            guess = d;
        } else {
            d = (uint32_t)(k >> shift) & (R - 1);
        }
        if (BUCKET && valid) dig16[i] = (uint16_t)d;            // the scatter reads it back instead of searching again
        wave_count_digit<BUCKET>(h, d, valid);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < R; d += kBlock) {
        const uint32_t v = h[d];
        counts[(int64_t)d * nblocks + blockIdx.x] = v;
        // BUCKET: the bucket totals are summed here (keys_kernel zeroed them) and the scatter adds up the few rows it
        // needs itself -- the keys arrive almost in order, a tile meets one or two buckets -- so this pass has no
        // radix_rowscan launch between its two kernels
        if (BUCKET && row_total != nullptr && v) atomicAdd(&row_total[d], v);
    }
}


// ---- scatter with wave-private ranking --------------------------------------------------------------
// The round-1 scatter (scripts/experiments) synchronised the workgroup three times per round of 256 keys (24 barriers per
// 2,048-key tile), and a workgroup's rounds are sequential: with every tile resident at once the
// kernel's time IS that chain.  Here wave w owns the contiguous keys [w * 64 * ITEMS, (w+1) * 64 * ITEMS)
// of the tile: (1) every wave counts its digits into its own LDS histogram, (2) one barrier, the
// histograms are turned into per-wave start offsets (digit base + tile prefix + earlier waves),
// (3) one barrier, then each wave scatters its rounds on its own (ranks and counts were kept in registers
// from step 1) -- the only shared state left is the wave's own offset row, and LDS operations of one wave are
// ordered.  Element order is
// (wave, round, lane) = tile order, and ranks within a round follow lane order, so the sort stays
// stable and its output is bitwise the same.
// PACK: the body index travels in the key word itself (bits 40..63; the keys of max_depth <= 21 are 40 bits,
// the launch holds <= 2^24 bodies), so a pass reads and writes ONE 8-byte array instead of a key and a
// value array (16 instead of 24 bytes per element, half the memory instructions, 16 KB less LDS per tile).
// PACK == 2: the last pass, which writes the plain key and the index to their own arrays for the tree build.
constexpr int kPackShift = 40;
constexpr uint64_t kPackKeyMask = (1ull << kPackShift) - 1;
// RAW (bucket pass only): `offs` holds the histogram's raw counts and the kernel adds up the rows it needs itself (no
// radix_rowscan launch) -- for bodies that arrive almost in order.  The exact modes never re-order their state, a tile meets
// as many buckets as it has room for, and the pass keeps its row scan (RAW = false: 29 us against 9 at N = 1M).
template <int ITEMS, int BITS = kRadixBits, int PACK = 0, bool BUCKET = false, bool RAW = BUCKET>
__global__ __launch_bounds__(kBlock) void radix_scatter_w(const uint64_t *__restrict__ kin,
                                                           const uint32_t *__restrict__ vin,
                                                           uint64_t *__restrict__ kout,
                                                           uint32_t *__restrict__ vout,
                                                           const uint32_t *__restrict__ offs,
                                                           const uint32_t *__restrict__ row_total, int64_t n,
                                                           int shift, int nblocks,
                                                           const uint16_t *__restrict__ dig16 = nullptr,
                                                           uint32_t *__restrict__ bucket_start = nullptr,
                                                           const uint32_t *__restrict__ direct_count = nullptr,
                                                           uint32_t direct_cap = 0, uint32_t direct_subcap = 0, int direct_nsub = 1)
{
    static_assert(!BUCKET || PACK == 1, "the bucket pass moves packed keys");
    DirectWords dw{0u, 1u};
    if (BUCKET && direct_count != nullptr) dw = direct_load(direct_count, direct_nsub);
    // (4) the tile is first sorted by digit INTO LDS, then written out in that order: the keys a digit
    // has in a tile leave as one contiguous run instead of separate partial-line writes from
    // different rounds
    constexpr int TILE = kBlock * ITEMS;
    constexpr int R = 1 << BITS, DPT = R / kBlock;          // digits per thread (thread t owns DPT*t ..)
    static_assert(R % kBlock == 0, "whole digits per thread");
    __shared__ uint32_t woff[kWavesPerBlock][R];            // counts, then running local offsets, per wave
    __shared__ int32_t gdelta[R];                           // global position - position in the sorted tile
    __shared__ uint64_t skey[TILE];
    __shared__ uint32_t sval[PACK ? 1 : TILE];
    __shared__ uint32_t sm[kWavesPerBlock + 1];
    __shared__ uint16_t sdig[BUCKET ? TILE : 1];            // BUCKET: the bucket of every key of the sorted tile
    // per wave: digit -> mask of the lanes that hold it in the current round (see bucket_sort_lds below: an LDS
    // OR + read + clear per key instead of ~8 vector instructions per digit bit of ballot matching)
    __shared__ uint64_t match[kWavesPerBlock][R];
    constexpr int kRowsTogether = 64;
    __shared__ uint32_t s_np, s_plist[kRowsTogether], s_before[kRowsTogether];
    const int t = threadIdx.x, w = wave_id(), l = lane_id();
    for (int d = t; d < R; d += kBlock)
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; ++k) { woff[k][d] = 0; match[k][d] = 0ull; }
    __syncthreads();
    if (BUCKET && direct_count != nullptr && direct_total(dw, direct_cap, direct_subcap) != ~0u) return;   // direct input: nothing to move

    const int64_t tile_base = (int64_t)blockIdx.x * TILE;
    const int64_t base = tile_base + (int64_t)w * (kWave * ITEMS);
    uint64_t key[ITEMS];
    uint32_t val[PACK ? 1 : ITEMS];
    uint32_t dig[ITEMS], rank[ITEMS], npeer[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int64_t i = base + r * kWave + l;
        const bool valid = i < n;
        key[r] = valid ? kin[i] : ~0ull;
        if (!PACK) val[r] = valid ? vin[i] : 0u;
        dig[r] = BUCKET ? (valid ? (uint32_t)dig16[i] : 0u) : (uint32_t)(key[r] >> shift) & (R - 1);
    }
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const bool valid = base + r * kWave + l < n;
        const uint32_t d = dig[r];
        if (BUCKET && wave_same_digit(d, valid)) {              // (uniform) a full wave inside one bucket: the usual case
            rank[r] = (uint32_t)l;
            npeer[r] = (uint32_t)kWave;
            if (l == 0) woff[w][d] += (uint32_t)kWave;
            continue;
        }
        uint64_t peers = 0;
        if (valid) (void)__hip_atomic_fetch_or(&match[w][d], 1ull << l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_wave_barrier();
        if (valid) peers = match[w][d];
        __builtin_amdgcn_wave_barrier();
        if (valid) match[w][d] = 0ull;
        __builtin_amdgcn_wave_barrier();
        rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
        npeer[r] = (uint32_t)__popcll(peers);
        if (valid && rank[r] == 0) woff[w][d] += npeer[r];      // one lane per digit; this wave's row only
    }
    __syncthreads();
    {
        // exclusive prefixes over the digits, in digit order: thread t holds digits DPT*t .. DPT*t+DPT-1
        uint32_t cnt[DPT], tot[DPT], csum = 0, tsum = 0;
#pragma unroll
        for (int j = 0; j < DPT; ++j) {
            const int d = DPT * t + j;
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < kWavesPerBlock; ++k) c += woff[k][d];
            cnt[j] = c; csum += c;
            tot[j] = row_total[d]; tsum += tot[j];
        }
        uint32_t all;
        uint32_t digit_base = block_exclusive_sum(tsum, sm, all);
        uint32_t lstart = block_exclusive_sum(csum, sm, all);
        if (BUCKET && RAW) {
            // offs holds the histogram's raw counts: the keys of bucket d in the tiles before this one are the sum of row
            // d up to this tile.  The buckets this tile meets -- one or two in steady motion, a dozen when the bodies
            // have drifted for sixteen builds since the state was last put in order -- are listed, and the waves add up
            // their rows, four rows per wave at a time; a tile that meets more than kRowsTogether buckets (disorder) lets
            // every thread add up the rows of its own digits instead.
            if (t == 0) s_np = 0u;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < DPT; ++j)
                if (cnt[j]) { const uint32_t k = atomicAdd(&s_np, 1u); if (k < (uint32_t)kRowsTogether) s_plist[k] = (uint32_t)(DPT * t + j); }
            __syncthreads();
            const uint32_t np = s_np;
            if (np <= 2u) {                                      // steady motion: the whole workgroup on one row, then the other
                for (uint32_t k = 0; k < np; ++k) {
                    const uint32_t *row = offs + (int64_t)s_plist[k] * nblocks;
                    uint32_t part = 0;
                    for (uint32_t b = (uint32_t)t; b < blockIdx.x; b += kBlock) part += row[b];
                    uint32_t total;
                    (void)block_exclusive_sum(part, sm, total);
                    if (t == 0) s_before[k] = total;
                }
                __syncthreads();
            } else if (np <= (uint32_t)kRowsTogether) {
                for (uint32_t k0 = 4u * (uint32_t)w; k0 < np; k0 += 4u * kWavesPerBlock) {   // four rows per wave at a time
                    const uint32_t *row[4];
                    uint32_t part[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 4; ++j) row[j] = offs + (int64_t)s_plist[(k0 + j < np) ? k0 + j : k0] * nblocks;
                    for (uint32_t b = (uint32_t)l; b < blockIdx.x; b += kWave) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) part[j] += row[j][b];                   // (independent loads)
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t inc = wave_inclusive_sum(part[j]);
                        if (l == kWave - 1 && k0 + j < np) s_before[k0 + j] = inc;
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int j = 0; j < DPT; ++j) {
            const int d = DPT * t + j;
            uint32_t before = 0;                                // keys of digit d in the tiles before this one
            if (BUCKET && RAW) {
                if (cnt[j]) {
                    const uint32_t np = s_np;
                    if (np <= (uint32_t)kRowsTogether) {
                        for (uint32_t k = 0; k < np; ++k) before = (s_plist[k] == (uint32_t)d) ? s_before[k] : before;
                    } else {
                        const uint32_t *row = offs + (int64_t)d * nblocks;
#pragma unroll 8
                        for (uint32_t b = 0; b < blockIdx.x; ++b) before += row[b];
                    }
                }
            } else {
                before = offs[(int64_t)d * nblocks + blockIdx.x];
            }
            gdelta[d] = (int32_t)(digit_base + before) - (int32_t)lstart;
            if (BUCKET && blockIdx.x == 0) bucket_start[d] = digit_base;   // where bucket d begins: bucket_sort_kernel reads it
            uint32_t run = lstart;
#pragma unroll
            for (int k = 0; k < kWavesPerBlock; ++k) { const uint32_t c = woff[k][d]; woff[k][d] = run; run += c; }
            digit_base += tot[j];
            lstart += cnt[j];
        }
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const bool valid = base + r * kWave + l < n;
        const uint32_t d = dig[r];
        uint32_t o = 0;
        if (valid) o = woff[w][d];                          // every peer reads the same word ...
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            skey[o + rank[r]] = key[r];
            if (!PACK) sval[o + rank[r]] = val[r];
            if (BUCKET) sdig[o + rank[r]] = (uint16_t)d;
        }
        if (valid && rank[r] == 0) woff[w][d] = o + npeer[r];   // ... before the first peer advances it
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    const int64_t left = n - tile_base;
    const int count = (left < TILE) ? (int)left : TILE;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int lp = r * kBlock + t;
        if (lp < count) {
            const uint64_t k = skey[lp];
            const int64_t dst = (int64_t)lp + gdelta[BUCKET ? (uint32_t)sdig[lp] : (uint32_t)(k >> shift) & (R - 1)];
            if (PACK == 2) {
                kout[dst] = k & kPackKeyMask;
                vout[dst] = (uint32_t)(k >> kPackShift);
            } else {
                kout[dst] = k;
                if (!PACK) vout[dst] = sval[lp];
            }
        }
    }
}

// ---- step (2) of the bucket sort ------------------------------------------------------------------------
// (A root box that moves by a depth-12 cell width per step re-aligns every finer cell, so in a dense core --
// where a bucket is a few such cells -- the re-keyed splitters are only as good as random ones at that scale:
// the largest of 256 buckets was 1.5x the average on the dynamic Plummer workload at N = 1.1M.  The LDS
// buffer therefore holds three times the average bucket of the largest launch.)
constexpr int kBsThreads = 1024, kBsWaves = kBsThreads / kWave;   // 16 waves: 4 per SIMD hide the LDS round trips
constexpr int kBucketItemsMax = 12;
constexpr int kBucketCap = kBucketItemsMax * kBsThreads;      // 12,288 keys (96 KB; + 16 KB offsets + 32 KB match tables)
// (the average bucket is at most a third of what fits: the largest of the buckets of a moving workload was
// measured at 1.5x the average)
constexpr int64_t kBucketMaxN = (int64_t)kBuckets * (kBucketCap / 3);       // 1,048,576 bodies with 256 buckets
constexpr int64_t kBucketMaxNBig = (int64_t)kBucketsBig * (kBucketCap / 3);  // 4,194,304 with 1,024

// exclusive scan of the 256 values held by threads 0..255 of the 1,024-thread workgroup (every thread calls;
// threads 256.. pass 0 and ignore the result)
__device__ __forceinline__ uint32_t bs_scan256(uint32_t v, uint32_t *sm, uint32_t &total)
{
    const int w = wave_id();
    const uint32_t inc = wave_inclusive_sum(v);
    if (w < 4 && lane_id() == kWave - 1) sm[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t q = sm[k]; base += (k < w) ? q : 0u; tot += q; }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// m <= 1,024 * ITEMS keys of one bucket: stable LSD byte passes, keys in registers between passes (wave w owns the
// contiguous keys [w * 64 * ITEMS, ...) as in radix_scatter_w), one LDS buffer.
// Who shares my digit?  Matching by ballots costs ~8 vector instructions per digit bit and the kernel was bound
// by exactly those (8.4 M vector instructions per launch at N = 1M, 2,050 per wave).  Instead every wave
// owns a 256-entry table of 64-bit lane masks in LDS: a lane ORs its lane bit into the entry of its digit, reads
// the entry back -- the mask of its peers -- and clears it (LDS instructions of one wave execute in order).
//
// How many passes?  A workgroup's time is its chain of passes (barriers, the 256-digit scan, the trip through LDS:
// ~4.5 us each, whatever the number of keys -- profiles/r03_final/build_ab.txt), one workgroup per CU, and the kernel
// is as slow as its slowest bucket: the keys of a core bucket of a Plummer sphere span 2^26, those of a halo bucket
// 2^38 -- four passes against five.  So the keys are taken relative to the bucket's smallest (the SPAN counts, not
// the differing bit positions: a bucket astride a quadrant boundary differs in bit 39), and a bucket whose span
// exceeds 24 bits is sorted by the TOP 24 bits of its span in three passes, after which every run of keys equal in
// those bits -- almost always a single key: <= 12,288 keys over 2^24 values -- is put in order by counting inside
// the run.  A run longer than kFixRun (keys piled up on a few values below a wide span) sends the workgroup through
// the full passes instead.  Either way the result is the stable order by key.
constexpr int kFixRun = 8;
//
// Placement (a bucket that is in order but for a few keys; BH_SORT_PLACE=0 turns it off).  With direct input a bucket is a
// range of an array that was sorted a few builds ago: bodies that overtook a neighbour along the curve since stand a place or
// two from where they belong, everybody else stands right.  Such a bucket is finished without a byte pass:
//   * an inversion is a pair j < i (input order) with K_j > K_i; the bucket is placeable with window W = kPlaceWindow iff no
//     inversion has i - j > W.  Then the stable rank of key i is
//         i - #{j in [i - W, i): K_j > K_i} + #{j in (i, i + W]: K_j < K_i},
//     and every key is written straight to kout / vout at that rank, as the run fix-up writes;
//   * the bucket's descents (K_i < K_{i-1}) are found on the way through the kmin / kmax reduction, each wave listing its own
//     -- position, the key before ("peak"), the key itself ("valley") -- in its row of `match`.  More than
//     kPlaceMaxDescents of them: straight to the passes, nothing else was done.  Otherwise every key is compared with the
//     listed ones: the largest key before i is a peak before i or K_{i-1}, the smallest after i a valley after i or K_{i+1},
//     so a key with no larger peak before it and no smaller valley after it stands where it belongs (no descents: all of
//     them), and only the others read their window from `in`;
//   * a peak larger than K_i more than W places before i, a valley smaller than K_i more than W places behind it, or
//     K_{i-W-1} > K_i, is an inversion too far apart: refused;
//   * crowds keep the passes and their re-run (`reruns` keeps its meaning): a bucket whose span exceeds 24 bits is refused
//     when some K_i and K_{i+kFixRun} (input order) are equal in the top 24 bits of the span.
// The decision is a function of the bucket's input alone (tests/sort_place_ref.py is its twin), every thread reads it from
// LDS after a barrier, and a refused bucket goes on into the passes with the keys it holds in registers.  It is taken in two
// steps: what the keys in registers and the list say first (crowd, a peak too far in front), so that a bucket with an
// inversion far apart reads no window; then, only in a bucket that has descents, what the windows say.
// Who is tested at all is decided by bucket_sort_kernel (`placeable`): single-bucket launches and the ranges of a direct build
// in which NO body changed bucket, up to kPlaceItemsMax keys per thread.  A bucket that is tested and refused pays the test and
// then the passes, and the kernel is as slow as its slowest bucket: builds that took the counting pass and builds with
// crossers -- bodies on their way, which also stand far from their place inside ranges -- were measurably slower with the test
// (profiles/sort_place/README.md) and take the passes untested.
//
// The stages, their barriers and what the LDS words hold between them:
//   before barrier 1 (the kmin / kmax barrier): every wave clears its row of match and lists its descents in match[w][0 ..
//     2 * kPlaceMaxDescents); thread 0 clears sm[4], sm[5] and puts this bucket's two counters into sm[6], sm[7] (kept to the end:
//     bs_scan256 uses sm[0..3] only); s_red[2 * kBsWaves + w] = descents of wave w;
//   after barrier 1: too many descents -> passes.  Else stage 1, from registers and the lists (read-only from here): crowd, peak
//     and valley rule; a thread that refuses sets sm[4];
//   barrier 2 (skipped when nothing can refuse: no descent, span <= 24 bits): sm[4] set -> passes.  Else stage 2: every key is
//     written to its rank -- speculatively, the passes overwrite all of it after a refusal -- and a key one place beyond whose
//     window a larger key stands sets sm[5];
//   barrier 3 (only with descents): sm[5] set -> passes, else placed.
//   On the way to the passes every wave zeroes the list entries of its own row again (all reads of them lie before barrier 2).
constexpr int kPlaceWindow = 8;
// (every key is compared with every listed descent, so what a bucket pays before it is refused grows with their number;
// slow motion leaves one or two)
constexpr int kPlaceMaxDescents = 8;
// keys per thread up to which the in-LDS sort has the path: a range of the direct input holds at most 4,096 keys (L <= 4,096 up
// to 4M bodies) and a single-bucket launch as many, so no larger tier ever meets a bucket that may be placed
constexpr int kPlaceItemsMax = 4;
static_assert(2 * kPlaceMaxDescents <= kDigits, "a wave lists its descents in its own row of match");
template <int ITEMS>
__device__ __forceinline__ void bucket_sort_lds(const uint64_t *in, int m, uint64_t *skey,
                                                uint32_t (*woff)[kDigits], uint64_t (*match)[kDigits],
                                                uint32_t *sm, uint64_t *s_red, uint32_t *s_flag,
                                                uint64_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                uint32_t *__restrict__ reruns, uint32_t *__restrict__ paths, bool placeable)
{
    const bool place = ITEMS <= kPlaceItemsMax && placeable;    // (uniform)
    const int t = threadIdx.x, w = wave_id(), l = lane_id();
    const int wbase = w * (kWave * ITEMS);
    // how often this bucket number was placed / went through the passes so far: thread 0 adds one to either at the end, in words
    // nobody else touches (loaded here, with the keys, and kept in sm[6], sm[7]: no atomic and no load at the end of the chain).
    // A plain load and store: right only because the bucket_sort_kernel launches of one context follow each other on one stream.
    uint32_t seen[2] = {0u, 0u};
    if (t == 0) { seen[0] = paths[0]; seen[1] = paths[kBucketsBig]; }
    uint64_t key[ITEMS];
    // placement: every key's predecessor, loaded beside it (the same lines; passing it from lane to lane cost four cross-lane
    // operations per key), and the kFixRun keys behind this wave's last (for the crowd rule)
    uint64_t pred[ITEMS <= kPlaceItemsMax ? ITEMS : 1];
    uint64_t kmin = ~0ull, kmax = 0ull;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int i = wbase + r * kWave + l;
        key[r] = (i < m) ? in[i] : ~0ull;
        if (ITEMS <= kPlaceItemsMax) pred[r] = (place && i > 0 && i < m) ? in[i - 1] : 0ull;
        if (i < m) {
            const uint64_t k = key[r] & kKeyMask40;
            kmin = (k < kmin) ? k : kmin; kmax = (k > kmax) ? k : kmax;
        }
    }
    uint64_t behind = 0ull;
    const bool has_behind = place && l >= kWave - kFixRun && wbase + kWave * ITEMS + l - (kWave - kFixRun) < m;
    if (has_behind) behind = in[wbase + kWave * ITEMS + l - (kWave - kFixRun)];
    // (every wave clears its own row of match: its list of descents below goes there, behind the zeroes)
    for (int k = t; k < kBsWaves * kDigits; k += kBsThreads) (&woff[0][0])[k] = 0;
#pragma unroll
    for (int k = 0; k < kDigits / kWave; ++k) match[w][k * kWave + l] = 0ull;
    if (t == 0) { *s_flag = 0u; sm[4] = 0u; sm[5] = 0u; sm[6] = seen[0]; sm[7] = seen[1]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
        kmin = (a < kmin) ? a : kmin; kmax = (b > kmax) ? b : kmax;
    }
    uint32_t ndesc = 0;                                         // this wave's descents (uniform)
    if (place) {
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int i = wbase + r * kWave + l;
            const uint64_t k = key[r] & kKeyMask40;
            const uint64_t prev = pred[ITEMS <= kPlaceItemsMax ? r : 0] & kKeyMask40;
            const bool desc = i < m && k < prev;
            const uint64_t bal = __ballot(desc);
            if (bal != 0ull) {                                  // (uniform; rare)
                if (ndesc < (uint32_t)kPlaceMaxDescents) {      // (a wave that is over has nothing to list)
                    const uint32_t slot = ndesc + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    if (desc && slot < (uint32_t)kPlaceMaxDescents) {
                        match[w][2 * slot] = prev | ((uint64_t)i << kPackShift);
                        match[w][2 * slot + 1] = k;
                    }
                }
                ndesc += (uint32_t)__popcll(bal);
            }
        }
    }
    if (l == 0) { s_red[w] = kmin; s_red[kBsWaves + w] = kmax; s_red[2 * kBsWaves + w] = ndesc; }
    __syncthreads();
    kmin = ~0ull; kmax = 0ull;
    uint32_t descents = 0;
#pragma unroll
    for (int k = 0; k < kBsWaves; ++k) {
        const uint64_t a = s_red[k], b = s_red[kBsWaves + k];
        kmin = (a < kmin) ? a : kmin; kmax = (b > kmax) ? b : kmax;
        descents += (uint32_t)s_red[2 * kBsWaves + k];
    }
    const uint64_t span = kmax - kmin;
    const int bits = span ? 64 - __clzll(span) : 0;
    if (place && descents <= (uint32_t)kPlaceMaxDescents) {     // (uniform)
        bool refuse = false;
        if (bits > 24) {                                        // the crowd rule
            const int first = bits - 24;
            uint32_t top[ITEMS + 1];
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) top[r] = (wbase + r * kWave + l < m) ? (uint32_t)(((key[r] & kKeyMask40) - kmin) >> first) : ~0u;
            top[ITEMS] = has_behind ? (uint32_t)(((behind & kKeyMask40) - kmin) >> first) : ~0u;   // (lanes 56.. hold them)
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) {
                const uint32_t a = (uint32_t)__shfl((int)top[r], (l + kFixRun) & (kWave - 1));
                // (the round behind: lane l + 8 - 64; behind the last round the lane itself holds the word)
                const uint32_t b = (r + 1 < ITEMS) ? (uint32_t)__shfl((int)top[r + 1], (l + kFixRun) & (kWave - 1)) : top[ITEMS];
                const uint32_t other = (l < kWave - kFixRun) ? a : b;
                refuse = refuse || (top[r] != ~0u && other == top[r]);
            }
        }
        uint32_t low = 0, high = 0;                             // bit r: key r has a larger key before / a smaller one behind it
        if (descents != 0u) {
            for (int k = 0; k < kBsWaves; ++k) {
                const uint32_t held = (uint32_t)s_red[2 * kBsWaves + k];
                for (uint32_t e = 0; e < held; ++e) {
                    const uint64_t word = match[k][2 * e], valley = match[k][2 * e + 1];
                    const uint64_t peak = word & kKeyMask40;
                    const int at = (int)(word >> kPackShift);   // the valley's position; the peak stands at at - 1
#pragma unroll
                    for (int r = 0; r < ITEMS; ++r) {
                        const int i = wbase + r * kWave + l;
                        const uint64_t kk = key[r] & kKeyMask40;
                        if (i < m) {
                            low |= (at <= i && peak > kk) ? 1u << r : 0u;
                            high |= (at > i && valley < kk) ? 1u << r : 0u;
                            // (a larger peak or a smaller valley further off than the window: an inversion too far apart.
                            // What is left for the windows below is at most kPlaceWindow keys on either side of a descent)
                            refuse = refuse || (at + kPlaceWindow <= i && peak > kk) || (at > i + kPlaceWindow && valley < kk);
                        }
                    }
                }
            }
        }
        // what the registers and the list say is decided first: a bucket with an arrival in front of its own keys, or a crowd,
        // has read no window when it goes on to the passes (in order and a span of <= 24 bits: nothing can have refused)
        bool placed = bits <= 24 && descents == 0u;
        if (!placed) {
            if (refuse) sm[4] = 1u;
            __syncthreads();
            placed = sm[4] == 0u;
        }
        if (placed) {
            // every key goes straight to its place in memory; a key more than the window behind a larger one that is no peak
            // (the run before a descent) shows only here, and then the passes overwrite all of it
            refuse = false;
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) {
                const int i = wbase + r * kWave + l;
                if (i < m) {
                    const uint64_t kk = key[r] & kKeyMask40;
                    int delta = 0;
                    if (((low | high) >> r) & 1u) {
                        // both windows and the key one place beyond, loaded together (one after the other they are a chain
                        // of seventeen memory latencies; a place outside the bucket counts as nothing)
                        uint64_t back[kPlaceWindow + 1], ahead[kPlaceWindow];
#pragma unroll
                        for (int d = 1; d <= kPlaceWindow + 1; ++d) back[d - 1] = (i - d >= 0) ? in[i - d] & kKeyMask40 : 0ull;
#pragma unroll
                        for (int d = 1; d <= kPlaceWindow; ++d) ahead[d - 1] = (i + d < m) ? in[i + d] & kKeyMask40 : kKeyMask40;
#pragma unroll
                        for (int d = 0; d < kPlaceWindow; ++d) delta += ((ahead[d] < kk) ? 1 : 0) - ((back[d] > kk) ? 1 : 0);
                        refuse = refuse || back[kPlaceWindow] > kk;
                    }
                    kout[i + delta] = kk;
                    vout[i + delta] = (uint32_t)(key[r] >> kPackShift);
                }
            }
            if (descents != 0u) {
                if (refuse) sm[5] = 1u;
                __syncthreads();
                placed = sm[5] == 0u;
            }
            if (placed) {
                if (t == 0) paths[0] = sm[6] + 1u;
                return;
            }
        }
    }
    if (place && l < 2 * kPlaceMaxDescents && (uint32_t)l < 2u * ndesc) match[w][l] = 0ull;   // the wave's list: its row is zero again
    if (bits == 0) {                                            // all keys equal (or one key): order is final
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int i = wbase + r * kWave + l;
            if (i < m) { kout[i] = key[r] & kKeyMask40; vout[i] = (uint32_t)(key[r] >> kPackShift); }
        }
        return;
    }
    // keys relative to the smallest (the body index in bits 40.. is untouched: no borrow, key >= kmin)
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) key[r] -= (wbase + r * kWave + l < m) ? kmin : 0ull;
    const int full = (bits + 7) / 8;
    int first = 0, passes = full;
    bool fix = false;
    // (two top passes and runs of up to 16 keys: 20.1 against 20.8 us at N = 1M, and twice the keys per run -- not taken)
    if (full > 3) { first = bits - 24; passes = 3; fix = true; }
    for (;;) {
        for (int p = 0; p < passes; ++p) {
            const int shift = first + 8 * p;
            // peers, ranks and counts first (kept in registers), wave totals per digit by the first peer
            uint32_t rank[ITEMS], cnt[ITEMS];
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) {
                const int i = wbase + r * kWave + l;
                const bool valid = i < m;
                const uint32_t d = (uint32_t)(key[r] >> shift) & 255u;
                uint64_t peers = 0;
                if (valid) (void)__hip_atomic_fetch_or(&match[w][d], 1ull << l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_wave_barrier();
                if (valid) peers = match[w][d];
                __builtin_amdgcn_wave_barrier();
                if (valid) match[w][d] = 0ull;
                __builtin_amdgcn_wave_barrier();
                rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
                cnt[r] = (uint32_t)__popcll(peers);
                if (valid && rank[r] == 0) woff[w][d] += cnt[r];    // one lane per digit; this wave's row only
            }
            __syncthreads();
            {
                uint32_t c = 0;
                if (t < kDigits) {
#pragma unroll
                    for (int k = 0; k < kBsWaves; ++k) c += woff[k][t];
                }
                uint32_t all;
                uint32_t run = bs_scan256(c, sm, all);
                if (t < kDigits) {
#pragma unroll
                    for (int k = 0; k < kBsWaves; ++k) { const uint32_t cc = woff[k][t]; woff[k][t] = run; run += cc; }
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) {
                const int i = wbase + r * kWave + l;
                const bool valid = i < m;
                const uint32_t d = (uint32_t)(key[r] >> shift) & 255u;
                uint32_t o = 0;
                if (valid) o = woff[w][d];                          // every peer reads the same word ...
                __builtin_amdgcn_wave_barrier();
                if (valid) skey[o + rank[r]] = key[r];
                if (valid && rank[r] == 0) woff[w][d] = o + cnt[r]; // ... before the first peer advances it
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
            if (p + 1 < passes) {
#pragma unroll
                for (int r = 0; r < ITEMS; ++r) {
                    const int i = wbase + r * kWave + l;
                    key[r] = (i < m) ? skey[i] : ~0ull;
                }
                for (int k = t; k < kBsWaves * kDigits; k += kBsThreads) (&woff[0][0])[k] = 0;
                __syncthreads();
            }
        }
        if (!fix) break;
        // ---- the keys are in order of their top 24 span bits, equal ones in input order: finish every run of equal
        // top bits by counting.  Position = own position + (later keys of the run that are smaller) - (earlier keys of
        // the run that are larger); keys equal in all bits keep their order.
        const uint64_t lowmask = (1ull << first) - 1ull;
        bool too_long = false;
        if (t == 0) paths[kBucketsBig] = sm[7] + 1u;          // (the same value again after a re-run)
        // (every key goes straight to its place in memory, at most kFixRun places from a coalesced store; should a run turn
        // out too long, the full sort below overwrites all of it)
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int i = t + r * kBsThreads;
            if (i < m) {
                const uint64_t word = skey[i];
                const uint64_t kk = word & kKeyMask40;
                const uint64_t top = kk >> first, low = kk & lowmask;
                int delta = 0, j;
                for (j = i - 1; j >= 0 && i - j <= kFixRun; --j) {
                    const uint64_t q = skey[j] & kKeyMask40;
                    if ((q >> first) != top) break;
                    delta -= ((q & lowmask) > low) ? 1 : 0;
                }
                too_long = too_long || (j >= 0 && i - j > kFixRun);
                for (j = i + 1; j < m && j - i <= kFixRun; ++j) {
                    const uint64_t q = skey[j] & kKeyMask40;
                    if ((q >> first) != top) break;
                    delta += ((q & lowmask) < low) ? 1 : 0;
                }
                too_long = too_long || (j < m && j - i > kFixRun);
                kout[i + delta] = kk + kmin;
                vout[i + delta] = (uint32_t)(word >> kPackShift);
            }
        }
        if (too_long) *s_flag = 1u;
        __syncthreads();
        if (*s_flag == 0u) return;
        // a long run: the full passes (rare: bodies piled up on a few key values under a wide span).  They start from the
        // keys as the three top passes left them in LDS, relative to kmin already -- keys equal in every bit are equal in
        // their top bits and therefore still in input order there, so the stable passes end in the same order as from the
        // input itself (which, with direct input, may BE this buffer and is gone)
        if (t == 0) atomicAdd(reruns, 1u);
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int i = wbase + r * kWave + l;
            key[r] = (i < m) ? skey[i] : ~0ull;
        }
        __syncthreads();                                        // (every key is in registers before a pass writes the buffer)
        for (int k = t; k < kBsWaves * kDigits; k += kBsThreads) (&woff[0][0])[k] = 0;
        __syncthreads();
        first = 0; passes = full; fix = false;
    }
    if (t == 0) paths[kBucketsBig] = sm[7] + 1u;
    for (int i = t; i < m; i += kBsThreads) {
        const uint64_t k = skey[i];
        kout[i] = (k & kKeyMask40) + kmin;
        vout[i] = (uint32_t)(k >> kPackShift);
    }
}

// What bucket_sort_kernel needs for direct input (see "direct input" above); count == nullptr: none.
struct BucketDirect {
    const uint32_t *count = nullptr;    // the crosser counters keys_kernel left
    const uint64_t *list = nullptr;     // the crossers' packed keys, [nsub][subcap]
    const uint64_t *range_keys = nullptr;
    uint64_t *keys = nullptr;           // the packed keys in state order (keys_kernel's output)
    uint64_t *scratch = nullptr;        // the counting pass's output array: free on this path
    int64_t n = 0;
    uint32_t cap = 0, subcap = 0, len = 0;
    int nb = 0, nsub = 1;
};
constexpr int kDirectItems = 4;                                  // a range is at most 4 keys per thread of the workgroup
constexpr int kMineCap = kBsWaves * kDigits - kBucketsBig;       // arrivals of one bucket held in LDS (3,072)

// sum of v over the 1,024 threads (every thread calls); tmp: >= kBsWaves words of LDS
__device__ __forceinline__ uint32_t bs_sum1024(uint32_t v, uint32_t *tmp, uint32_t &exclusive)
{
    const uint32_t inc = wave_inclusive_sum(v);
    if (lane_id() == kWave - 1) tmp[wave_id()] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBsWaves; ++k) { const uint32_t q = tmp[k]; base += (k < wave_id()) ? q : 0u; tot += q; }
    __syncthreads();
    exclusive = base + inc - v;
    return tot;
}

// One workgroup of 1,024 threads per bucket.  bucketed: the packed keys grouped by bucket (step 1's output);
// kout / vout: the sorted plain keys and body indices; kout doubles as the second buffer of the
// through-memory path.  dz: direct input -- when the crosser counters allow it, the workgroup takes its keys from its
// range of dz.keys and from the crosser list instead, and works out its place in the output from the list.
__global__ __launch_bounds__(kBsThreads) void bucket_sort_kernel(uint64_t *__restrict__ bucketed,
                                                                  uint64_t *__restrict__ kout,
                                                                  uint32_t *__restrict__ vout,
                                                                  const uint32_t *__restrict__ bucket_total,
                                                                  const uint32_t *__restrict__ bucket_start,
                                                                  uint32_t *__restrict__ spills,
                                                                  uint32_t *__restrict__ reruns, int single_m,
                                                                  BucketDirect dz, uint32_t *__restrict__ paths, int place)
{
    __shared__ uint64_t skey[kBucketCap];
    __shared__ uint32_t woff[kBsWaves][kDigits];
    __shared__ uint64_t match[kBsWaves][kDigits];
    __shared__ uint32_t sm[8];
    __shared__ uint64_t s_or[3 * kBsWaves];
    __shared__ uint32_t s_flag;
    __shared__ uint32_t s_dz[3];                                // direct input: arrivals, arrivals from lower ranges, departures
    const int t = threadIdx.x, w = wave_id(), l = lane_id();
    // where this bucket starts and how many keys it holds: the counting pass's scatter left both (wave-uniform loads)
    // (bucket_total == nullptr: a launch of at most kBucketCap keys is ONE bucket -- the keys as keys_kernel left them, no
    // counting pass in front: three launches less for the small launches whose builds are chains of 5 us launches)
    int64_t start;
    int m;
    uint64_t *in;
    // (the counting pass's words are loaded before the decision is looked at: stale but readable when it is not taken)
    const int64_t counted_start = bucket_total ? (int64_t)bucket_start[blockIdx.x] : 0;
    const int counted_m = bucket_total ? (int)bucket_total[blockIdx.x] : single_m;
    const uint32_t crossers = dz.count ? direct_total(dz.count, dz.nsub, dz.cap, dz.subcap) : ~0u;       // (uniform)
    // placement is tried only where the input can be in order: a single-bucket launch, and the ranges of a direct build without
    // a crosser.  (uniform)
    bool placeable = place != 0 && bucket_total == nullptr;
    if (crossers == ~0u) {
        start = counted_start;
        m = counted_m;
        if (m == 0) return;
        in = bucketed + start;
    } else {
        const int b = (int)blockIdx.x;
        const int64_t r0 = ((int64_t)b * dz.len < dz.n) ? (int64_t)b * dz.len : dz.n;
        const int len = (int)((r0 + dz.len < dz.n ? r0 + dz.len : dz.n) - r0);
        if (crossers == 0u) {                                    // nobody changed bucket: the range as it stands
            placeable = place != 0;
            start = r0; m = len;
            if (m == 0) return;
            in = dz.keys + r0;
        } else {
            // every workgroup routes the whole list (<= T binary searches over 1,024 threads, range keys in LDS): what
            // every bucket gains and loses gives this bucket's place in the output, the keys sent here are set aside
            uint64_t *spl = &match[0][0];                        // [nb]
            uint64_t *mine = spl + kBucketsBig;                  // [kMineCap]
            uint32_t *delta = &woff[0][0];                       // [nb] arrived - left (mod 2^32)
            uint32_t *held = reinterpret_cast<uint32_t *>(skey);  // [nsub] entries of every list
            for (int k = t; k < dz.nb; k += kBsThreads) { spl[k] = dz.range_keys[k]; delta[k] = 0u; }
            if (t < 3) s_dz[t] = 0u;
            if (t < dz.nsub) held[t] = dz.count[kDirectStride * (1u + (uint32_t)t)];
            __syncthreads();
            // every slot of every list is looked at (nsub * subcap slots: four per thread with the default capacity)
            uint32_t most = 0;
            for (int k = 0; k < dz.nsub; ++k) most = (held[k] > most) ? held[k] : most;
            const uint32_t slots = (dz.nsub > 1) ? (uint32_t)dz.nsub * dz.subcap : most;
            const uint32_t lg_sub = 31u - (uint32_t)__clz(dz.nsub > 1 ? (int)dz.subcap : 1);   // (subcap is a power of two then)
            auto listed = [&](uint32_t x) -> bool { return dz.nsub > 1 ? (x & (dz.subcap - 1u)) < held[x >> lg_sub] : true; };
            for (uint32_t e = (uint32_t)t; e < slots; e += kBsThreads) {
                if (!listed(e)) continue;
                const uint64_t word = dz.list[e];
                const uint32_t idx = (uint32_t)(word >> kPackShift);
                const int dst = (int)bucket_of_n(word & kKeyMask40, spl, dz.nb), src = (int)(idx / dz.len);
                atomicAdd(&delta[dst], 1u);
                atomicSub(&delta[src], 1u);
                if (dst == b) {
                    const uint32_t k = atomicAdd(&s_dz[0], 1u);
                    if (k < (uint32_t)kMineCap) mine[k] = word;
                    if ((int64_t)idx < r0) atomicAdd(&s_dz[1], 1u);
                }
                if (src == b) atomicAdd(&s_dz[2], 1u);
            }
            __syncthreads();
            uint32_t part = 0, ex;
            for (int k = t; k < b; k += kBsThreads) part += delta[k];
            uint32_t *tmp = reinterpret_cast<uint32_t *>(s_or);
            const uint32_t moved = bs_sum1024(part, tmp, ex);    // net arrivals of the buckets before this one (mod 2^32)
            const uint32_t arrived = s_dz[0], lower = s_dz[1], left = s_dz[2];
            start = r0 + (int64_t)(int32_t)moved;
            m = len - (int)left + (int)arrived;
            if (m <= 0 || start < 0 || start + m > dz.n) return; // (m == 0: an emptied range; the rest cannot happen)
            if (arrived == 0u && left == 0u) {
                in = dz.keys + r0;
            } else {
                // the bucket's input in body order: arrivals from lower ranges, the keys of the range that stay, arrivals
                // from higher ranges -- into the sort's LDS buffer, or into this bucket's stretch of the scratch array when
                // it is too large for LDS (the through-memory path below wants it in memory)
                uint64_t *ko_ = kout + start;
                const uint64_t *arr = mine;
                if (arrived > (uint32_t)kMineCap) {              // more arrivals than LDS holds: listed in the output stretch
                    __syncthreads();
                    if (t == 0) s_dz[0] = 0u;
                    __syncthreads();
                    for (uint32_t e = (uint32_t)t; e < slots; e += kBsThreads) {
                        if (!listed(e)) continue;
                        const uint64_t word = dz.list[e];
                        if ((int)bucket_of_n(word & kKeyMask40, spl, dz.nb) == b) ko_[atomicAdd(&s_dz[0], 1u)] = word;
                    }
                    __threadfence_block();
                    __syncthreads();
                    arr = ko_;
                }
                uint64_t *g = (m <= kBucketCap) ? skey : dz.scratch + start;
                const uint64_t lo = spl[b], hi = (b + 1 < dz.nb) ? spl[b + 1] : kRangeKeyInf;
                uint64_t own[kDirectItems];
                uint32_t c = 0;
#pragma unroll
                for (int j = 0; j < kDirectItems; ++j) {
                    const int i = kDirectItems * t + j;
                    own[j] = (i < len) ? dz.keys[r0 + i] : kRangeKeyInf;
                    c += (i < len && stays_in(own[j] & kKeyMask40, lo, hi)) ? 1u : 0u;
                }
                const uint32_t stay = bs_sum1024(c, tmp, ex);
                uint32_t o = lower + ex;
#pragma unroll
                for (int j = 0; j < kDirectItems; ++j)
                    if (kDirectItems * t + j < len && stays_in(own[j] & kKeyMask40, lo, hi)) { if (o < (uint32_t)m) g[o] = own[j]; ++o; }
                for (uint32_t q = (uint32_t)t; q < arrived; q += kBsThreads) {
                    const uint64_t word = arr[q];
                    const uint32_t idx = (uint32_t)(word >> kPackShift);
                    uint32_t rank = 0;
                    for (uint32_t r = 0; r < arrived; ++r) rank += ((uint32_t)(arr[r] >> kPackShift) < idx) ? 1u : 0u;
                    const uint32_t slot = rank + (((int64_t)idx < r0) ? 0u : stay);
                    if (slot < (uint32_t)m) g[slot] = word;
                }
                __threadfence_block();
                __syncthreads();
                in = g;
            }
        }
    }
    uint64_t *ko = kout + start;
    uint32_t *vo = vout + start;

    if (m <= 1 * kBsThreads) { bucket_sort_lds<1>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= 2 * kBsThreads) { bucket_sort_lds<2>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= 4 * kBsThreads) { bucket_sort_lds<4>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= 5 * kBsThreads) { bucket_sort_lds<5>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= 6 * kBsThreads) { bucket_sort_lds<6>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= 8 * kBsThreads) { bucket_sort_lds<8>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }
    if (m <= kBucketCap) { bucket_sort_lds<kBucketItemsMax>(in, m, skey, woff, match, sm, s_or, &s_flag, ko, vo, reruns, paths + blockIdx.x, placeable); return; }

    // which key bits differ inside the bucket: only those bytes need a pass
    const uint64_t k0 = in[0];
    uint64_t x = 0;
    for (int i = t; i < m; i += kBsThreads) x |= (in[i] ^ k0) & kKeyMask40;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x |= __shfl_xor(x, o);
    if (l == 0) s_or[w] = x;
    __syncthreads();
    x = 0;
#pragma unroll
    for (int k = 0; k < kBsWaves; ++k) x |= s_or[k];
    const int passes = x ? (64 - __clzll(x) + 7) / 8 : 0;

    // ---- the bucket does not fit: the same stable passes through global memory, 1,024 keys per round, by this
    // workgroup alone (all its waves share one L1: workgroup barriers order the stores and the loads)
    if (t == 0 && passes > 0) atomicAdd(spills, 1u);           // (a bucket of equal keys is only copied)
    uint64_t *src = in, *dst = ko;
    uint32_t *hist = reinterpret_cast<uint32_t *>(skey);        // [256] counts, then running bases
    const uint64_t lt = (l == 0) ? 0ull : (~0ull >> (64 - l));
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p;
        if (t < kDigits) hist[t] = 0;
        for (int k = t; k < kBsWaves * kDigits; k += kBsThreads) (&woff[0][0])[k] = 0;
        __syncthreads();
        for (int i = t; i < m; i += kBsThreads) atomicAdd(&hist[(uint32_t)(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        {
            const uint32_t c = (t < kDigits) ? hist[t] : 0u;
            uint32_t all;
            const uint32_t e = bs_scan256(c, sm, all);
            if (t < kDigits) hist[t] = e;
        }
        __syncthreads();
        for (int i0 = 0; i0 < m; i0 += kBsThreads) {
            const int i = i0 + t;
            const bool valid = i < m;
            const uint64_t key = valid ? src[i] : ~0ull;
            const uint32_t d = (uint32_t)(key >> shift) & 255u;
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            const uint32_t rank = __popcll(peers & lt);
            if (valid && rank == 0) woff[w][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (valid) {
                uint32_t o = hist[d] + rank;
                for (int k = 0; k < w; ++k) o += woff[k][d];
                dst[o] = key;
            }
            __syncthreads();
            if (t < kDigits) {
                uint32_t sacc = 0;
#pragma unroll
                for (int k = 0; k < kBsWaves; ++k) { sacc += woff[k][t]; woff[k][t] = 0; }
                hist[t] += sacc;
            }
            __syncthreads();
        }
        __threadfence_block();
        __syncthreads();
        uint64_t *tmp = src; src = dst; dst = tmp;
    }
    // unpack where the keys ended up (element-wise, so doing it in place in kout is safe)
#pragma unroll 8
    for (int i = t; i < m; i += kBsThreads) {
        const uint64_t k = src[i];
        ko[i] = k & kKeyMask40;
        vo[i] = (uint32_t)(k >> kPackShift);
    }
}


}  // namespace bh
