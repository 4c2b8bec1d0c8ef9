// bh_neighbours.hpp -- k nearest neighbours and radius counts of the current state (bh_neighbours, bh_count_within).  The
// reference has no such query.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: nothing below is fused.
//
// Distance.  For a query q and body j: dx = x_j - q.x, dy = y_j - q.y, d2 = dx * dx + dy * dy in fp64 (an fp32 state is
// widened first, which is exact).  bh_neighbours gives the first k bodies in the total order (d2, caller index), bh_count_within
// the number of bodies with d2 <= r2.  A body query leaves itself out by index; nothing else is ever left out.
//
// Structure, built per call from the state (the force trees carry no cell boxes, the fp64 tree no body ranges):
//   bounds   nb_bounds_kernel: min / max of x and y and a flag for a non-finite coordinate; workgroup fold, one atomic per
//            workgroup on the ordered bit pattern of the doubles.
//   keys     Morton keys of 16 bits per axis in that box (field_cell16 / field_spread16 of bh_field.hpp) with the slot above
//            kPackShift, sorted by the LSD passes of bh_sort.hpp: hence at most 2^24 bodies.
//   copies   spos[s]: the position of the s-th sorted body as double2; sidx[s]: its caller index.
//   boxes    leaves are runs of kNbLeaf consecutive sorted bodies; node i of level l + 1 covers nodes 4 i .. 4 i + 3 of level l
//            (index arithmetic, no links); every node holds the tight bounding box of the positions it covers.  The levels lie
//            one after the other in one array, off[l] is the first node of level l, off[levels] the total.
//
// Pruning is exact (the argument stands with nb_walk below: lb <= d2 <= ub for every body of a box, as computed).  The k
// nearest search drops a node only when the lane's list is full and lb > the list's k-th d2 -- strictly: at equality a body
// with a smaller caller index can still enter.  The count drops a node when lb > r2, and takes a node whole, without opening
// it, when ub <= r2; the number of bodies of a node follows from its index.  Neither kNbLeaf, the key resolution nor the order
// of the traversal can therefore change a result: they decide only how many distances are computed.
//
// Launch shape and traversal: nb_walk's.  Body queries run in the sorted order itself, points Morton-sorted in the same box by
// field_keys_kernel.
//
// Seeding.  Before the traversal a lane inserts the bodies at the sorted positions [s - k, s + k] around its own place s (a
// body query: its sorted position, itself left out; a point: the lower bound of its key among the sorted body keys), and the
// traversal skips those positions.  The list is then full of near bodies before the first box is tested.
//
// The list: k entries of (d2, caller index) per lane in LDS, entry e of lane l at e * 64 + l (the lanes of a wave on different
// banks), sorted by (d2, caller index); a workgroup is one wavefront and its LDS is sized by k (12 * 64 * k bytes).
#pragma once

#include "bh_field.hpp"

namespace bh {

constexpr int kNbLeaf = 8;              // bodies per leaf (why 8)
constexpr int kNbMaxK = 32;             // = BH_NEIGHBOURS_MAX_K
constexpr int kNbMaxLevels = 15;        // off[] has kNbMaxLevels + 1 entries; 2^24 bodies make 12 levels
constexpr int64_t kNbMaxBodies = (int64_t)1 << (64 - kPackShift);

struct NbBox { double lox, hix, loy, hiy; };
// what the bounds pass leaves: ordered bit patterns (nb_ordered) of the four bounds, and the flag
struct NbBounds { unsigned long long lox, hix, loy, hiy, bad; };

// a map of the doubles onto the unsigned integers that keeps their order (-0.0 below +0.0)
__host__ __device__ __forceinline__ unsigned long long nb_ordered(double v)
{
    unsigned long long u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__host__ __device__ __forceinline__ double nb_unordered(unsigned long long u)
{
    u = (u >> 63) ? (u & ~(1ull << 63)) : ~u;
    double v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

// levels of the hierarchy over n > 0 bodies and their offsets: off[0] = 0, off[l + 1] = off[l] + nodes of level l; the last
// level has one node; the entries after it repeat the total.  Returns the number of levels.  `off` may be device memory
// written by one thread (nb_setup_kernel) or a host array.
__host__ __device__ inline int nb_levels(int64_t n, int32_t *off)
{
    int64_t count = (n + kNbLeaf - 1) / kNbLeaf;
    int32_t total = 0;
    int levels = 0;
    off[0] = 0;
    for (;;) {
        total += (int32_t)count;
        off[++levels] = total;
        if (count == 1) break;
        count = (count + 3) / 4;
    }
    for (int l = levels; l < kNbMaxLevels; ++l) off[l + 1] = total;
    return levels;
}

// out (zeroed except lox = loy = ~0): the bounds of the positions, and whether any coordinate is not finite
template <typename Real2>
__global__ __launch_bounds__(kBlock) void nb_bounds_kernel(const Real2 *__restrict__ pos, int64_t n, NbBounds *__restrict__ out)
{
    __shared__ double sh[4][kWavesPerBlock];
    __shared__ int sh_bad[kWavesPerBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double x0 = (double)INFINITY, x1 = -(double)INFINITY, y0 = (double)INFINITY, y1 = -(double)INFINITY;
    bool bad = false;
    if (i < n) {
        const Real2 p = pos[i];
        const double x = (double)p.x, y = (double)p.y;
        bad = !(map_finite(x) && map_finite(y));
        if (!bad) { x0 = x1 = x; y0 = y1 = y; }
    }
    x0 = wave_min(x0); x1 = wave_max(x1); y0 = wave_min(y0); y1 = wave_max(y1);
    const bool wbad = __ballot(bad) != 0ull;
    if (lane_id() == 0) {
        sh[0][wave_id()] = x0; sh[1][wave_id()] = x1; sh[2][wave_id()] = y0; sh[3][wave_id()] = y1;
        sh_bad[wave_id()] = wbad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) {
            x0 = (sh[0][w] < x0) ? sh[0][w] : x0; x1 = (sh[1][w] > x1) ? sh[1][w] : x1;
            y0 = (sh[2][w] < y0) ? sh[2][w] : y0; y1 = (sh[3][w] > y1) ? sh[3][w] : y1;
            b |= sh_bad[w];
        }
        if (x0 <= x1) {                                        // (a workgroup of bad bodies only has nothing to send)
            atomicMin(&out->lox, nb_ordered(x0)); atomicMax(&out->hix, nb_ordered(x1));
            atomicMin(&out->loy, nb_ordered(y0)); atomicMax(&out->hiy, nb_ordered(y1));
        }
        if (b) atomicOr(&out->bad, 1ull);
    }
}

// box[0..3] = lox, hix, loy, hiy as doubles (what field_keys_kernel reads); off[]: the level table of n bodies
__global__ void nb_setup_kernel(const NbBounds *__restrict__ b, int64_t n, double *__restrict__ box, int32_t *__restrict__ off)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    box[0] = nb_unordered(b->lox); box[1] = nb_unordered(b->hix);
    box[2] = nb_unordered(b->loy); box[3] = nb_unordered(b->hiy);
    nb_levels(n, off);
}

// keys[i] = Morton key of body slot i in the box | i << kPackShift
template <typename Real2>
__global__ __launch_bounds__(kBlock) void nb_keys_kernel(const Real2 *__restrict__ pos, int64_t n, const double *__restrict__ box,
                                                         uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Real2 p = pos[i];
    const uint32_t ix = field_cell16((double)p.x, box[0], box[1]), iy = field_cell16((double)p.y, box[2], box[3]);
    const uint64_t key = (uint64_t)(field_spread16(ix) | (field_spread16(iy) << 1));
    keys[i] = key | ((uint64_t)i << kPackShift);
}

// the sorted copies: spos[s] = pos[slot[s]] widened, sidx[s] = the caller index of that slot (orig null: the slot itself)
template <typename Real2>
__global__ __launch_bounds__(kBlock) void nb_gather_kernel(const Real2 *__restrict__ pos, const uint32_t *__restrict__ slot,
                                                           const uint32_t *__restrict__ orig, int64_t n, double2 *__restrict__ spos,
                                                           uint32_t *__restrict__ sidx)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t b = slot[s];
    const Real2 p = pos[b];
    spos[s] = double2{(double)p.x, (double)p.y};
    sidx[s] = orig ? orig[b] : b;
}

// level 0: the box of the bodies [i * kNbLeaf, min(n, (i + 1) * kNbLeaf))
__global__ __launch_bounds__(kBlock) void nb_leaf_kernel(const double2 *__restrict__ spos, int64_t n, int32_t count,
                                                         NbBox *__restrict__ boxes)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int64_t first = i * kNbLeaf;
    const int64_t last = (first + kNbLeaf < n) ? first + kNbLeaf : n;
    double2 p = spos[first];
    NbBox b{p.x, p.x, p.y, p.y};
    for (int64_t j = first + 1; j < last; ++j) {
        p = spos[j];
        b.lox = (p.x < b.lox) ? p.x : b.lox; b.hix = (p.x > b.hix) ? p.x : b.hix;
        b.loy = (p.y < b.loy) ? p.y : b.loy; b.hiy = (p.y > b.hiy) ? p.y : b.hiy;
    }
    boxes[i] = b;
}

// a level above: node i of `up` (count of them) = the union of nodes 4 i .. min(4 i + 3, below - 1) of `down`
__global__ __launch_bounds__(kBlock) void nb_level_kernel(const NbBox *__restrict__ down, int32_t below, NbBox *__restrict__ up,
                                                          int32_t count)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    NbBox b = down[4 * i];
    for (int c = 1; c < 4; ++c) {
        if (4 * i + c >= below) break;
        const NbBox d = down[4 * i + c];
        b.lox = (d.lox < b.lox) ? d.lox : b.lox; b.hix = (d.hix > b.hix) ? d.hix : b.hix;
        b.loy = (d.loy < b.loy) ? d.loy : b.loy; b.hiy = (d.hiy > b.hiy) ? d.hiy : b.hiy;
    }
    up[i] = b;
}

// the lower bound lb of the d2 of anything inside b, seen from q, and (UB) the upper bound: the header's formulas
template <bool UB>
__device__ __forceinline__ double nb_bound(const NbBox &b, const double2 q, double &ub)
{
    const double ax = b.lox - q.x, cx = q.x - b.hix, ay = b.loy - q.y, cy = q.y - b.hiy;
    double bx = (cx > ax) ? cx : ax, by = (cy > ay) ? cy : ay;
    bx = (bx > 0.0) ? bx : 0.0;
    by = (by > 0.0) ? by : 0.0;
    if (UB) {
        const double ex = q.x - b.lox, gx = b.hix - q.x, ey = q.y - b.loy, gy = b.hiy - q.y;
        const double fx = (ex > gx) ? ex : gx, fy = (ey > gy) ? ey : gy;
        ub = fx * fx + fy * fy;
    }
    return bx * bx + by * by;
}

// the first position s of the sorted keys (n of them) with keys[s] >= key
__device__ __forceinline__ int32_t nb_lower_bound(const uint64_t *__restrict__ keys, int32_t n, uint64_t key)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {                                          // (at most 25 rounds)
        const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a lane's list in LDS: D and I point at the lane's entry 0, entry e is kWave further
struct NbList {
    double *D;
    uint32_t *I;
    int k, cnt;
    double kd2;                    // the k-th d2 once the list is full
    uint32_t kid;                  // and its caller index
    __device__ __forceinline__ bool wants(double lb) const { return cnt < k || lb <= kd2; }
    __device__ __forceinline__ void insert(double d, uint32_t id)
    {
        if (cnt == k && (d > kd2 || (d == kd2 && id > kid))) return;
        int e = (cnt < k) ? cnt : k - 1;                       // (full: the last entry falls out)
        while (e > 0) {
            const double dp = D[(e - 1) * kWave];
            const uint32_t ip = I[(e - 1) * kWave];
            if (dp < d || (dp == d && ip < id)) break;
            D[e * kWave] = dp;
            I[e * kWave] = ip;
            --e;
        }
        D[e * kWave] = d;
        I[e * kWave] = id;
        if (cnt < k) ++cnt;
        if (cnt == k) { kd2 = D[(k - 1) * kWave]; kid = I[(k - 1) * kWave]; }
    }
};

// ---- the one traversal of the index: nb_knn_kernel, nb_count_kernel, pair_count_kernel (bh_pairs.hpp), grp_link_kernel
// (bh_groups.hpp) and mst_nearest_kernel (bh_mst.hpp) ----------------------------------------------------------------------------
//
// Why pruning on the boxes is exact.  For a box and a query, bx = max(lox - q.x, q.x - hix, 0), by likewise and
// lb = bx * bx + by * by, in the operations of d2.  Rounded subtraction, multiplication and addition are monotone, and
// rounding is symmetric in the sign: for a body in the box with q.x < lox, dx = x_j - q.x >= lox - q.x = bx as computed; with
// q.x > hix, dx <= hix - q.x = -bx; so |dx| >= bx, dx * dx >= bx * bx, and the computed d2 >= lb.  With
// ub = fx * fx + fy * fy, fx = max(q.x - lox, hix - q.x), the same argument gives |dx| <= fx, so every body of the box has
// d2 <= ub.  A caller drops a node on lb, takes it whole on ub (its bodies are counted by nb_range, never read) or opens it:
// whatever it decides on these two bounds changes how many distances are computed and no result.
//
// Launch shape: that of the side walks (bh_treewalk.hpp), whatever the workgroup -- nb_walk knows the wave only.  One lane per
// query, the 64 queries of a wavefront consecutive in the sorted order; the boxes, the level offsets and the leaf bodies read
// at wave-uniform addresses in the constant address space (scalar loads); one LaneStack of {level, node, lane mask} per wave.
// 2^24 bodies make 12 levels, and depth-first pushing of four children needs at most 3 * 12 + 4 entries.  The children are
// pushed last first: child 0 is opened first, so the traversal meets the sorted positions in ascending order.  A lane takes
// part in a node only if it took part in the parent and its own visit() says so: its nodes and bodies are those of a solo
// search in the same fixed order, whoever shares the wave.  Every loop is bounded by kNbLeaf or the depth; nobody waits.
//
//   visit(mine, node) -> bool   every lane of the wave, for every node popped.  mine: the lane took part in the parent.
//                               Whole-node work is done in here; true: the lane opens the node (false where !mine).
//   body(rest, j, px, py)       every lane, for every body j of a leaf that some lane opened; rest: this lane did.  (px, py) =
//                               spos[j], loaded once by the walker.
//   leaf_end()                  after the last body of such a leaf (optional).

// a node's bodies: the sorted positions [first, last) of node `node` of level `level` over n bodies
__host__ __device__ __forceinline__ void nb_range(int level, int64_t node, int64_t n, int64_t &first, int64_t &last)
{
    const int64_t span = (int64_t)kNbLeaf << (2 * level);
    first = node * span;
    last = (first + span < n) ? first + span : n;
}

struct NbNode {
    int level;
    int32_t node, at;              // index in its level, and in boxes[] (= off[level] + node)
    NbBox box;
    int64_t first, last;           // nb_range
};

template <typename Visit, typename Body, typename LeafEnd>
__device__ __forceinline__ void nb_walk(const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                        const double2 *__restrict__ spos, const int32_t levels, const int32_t n, const bool valid,
                                        Visit visit, Body body, LeafEnd leaf_end)
{
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const NbBox BH64_CONSTANT *cb = (const NbBox BH64_CONSTANT *)boxes;
    const int32_t BH64_CONSTANT *co = (const int32_t BH64_CONSTANT *)off;
    const double2 BH64_CONSTANT *cpos = (const double2 BH64_CONSTANT *)spos;
#pragma clang diagnostic pop

    // stack entries: level in the bits above 24, node below (a level has at most 2^21 nodes)
    auto nb_entry = [](int level, int32_t node) -> int32_t { return (level << 24) | node; };
    LaneStack st;
    const uint64_t all = __ballot(valid);
    if (all != 0ull) st.push(nb_entry(levels - 1, 0), all);
    while (st.sp > 0) {
        int32_t entry;
        uint64_t mask;
        st.pop(entry, mask);
        const int level = entry >> 24;
        const int32_t node = entry & 0xffffff;
        NbNode nd;
        nd.level = level;
        nd.node = node;
        nd.at = co[level] + node;
        nd.box.lox = cb[nd.at].lox; nd.box.hix = cb[nd.at].hix; nd.box.loy = cb[nd.at].loy; nd.box.hiy = cb[nd.at].hiy;
        nb_range(level, node, n, nd.first, nd.last);
        // (the mask is wave-uniform: it becomes the lanes' condition as it is, no lane forms 1 << lane)
        const bool rest = visit(__builtin_amdgcn_inverse_ballot_w64(mask), nd);
        const uint64_t open = __ballot(rest);
        if (open == 0ull) continue;
        if (level == 0) {
            int64_t first, last;                               // (nd's, with the level a constant: the span folds)
            nb_range(0, node, n, first, last);
            for (int32_t j = (int32_t)first; j < (int32_t)last; ++j) {
                const double px = cpos[j].x, py = cpos[j].y;
                body(rest, j, px, py);
            }
            leaf_end();
        } else {
            const int32_t below = co[level] - co[level - 1];
            for (int c = 3; c >= 0; --c)                       // (pushed last first: child 0 is opened first)
                if (4 * node + c < below) st.push(nb_entry(level - 1, 4 * node + c), open);
        }
    }
}

template <typename Visit, typename Body>
__device__ __forceinline__ void nb_walk(const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                        const double2 *__restrict__ spos, const int32_t levels, const int32_t n, const bool valid,
                                        Visit visit, Body body)
{
    nb_walk(boxes, off, spos, levels, n, valid, visit, body, [] {});
}

// k nearest bodies of the queries of rows [0, nq) of this launch: row r is the body at sorted position s0 + r (POINTS false), or
// the point points[order[r]], whose sorted key is pkeys[r] (POINTS true).  Row r of the outputs: k entries, padded with
// -1 / +inf; evals[r]: the bodies whose d2 the lane computed.  Dynamic LDS: k * kWave * 12 bytes.
template <bool POINTS>
__global__ __launch_bounds__(kWave) void nb_knn_kernel(const double2 *__restrict__ spos, const uint32_t *__restrict__ sidx,
                                                       const uint64_t *__restrict__ bkeys, const NbBox *__restrict__ boxes,
                                                       const int32_t *__restrict__ off, int32_t levels, int32_t n, int32_t k,
                                                       const double2 *__restrict__ points, const uint32_t *__restrict__ order,
                                                       const uint64_t *__restrict__ pkeys, int64_t s0, int64_t nq,
                                                       int64_t *__restrict__ out_idx, double *__restrict__ out_d2,
                                                       uint32_t *__restrict__ evals)
{
    extern __shared__ double nb_lds[];
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * kWave + lane;
    const bool valid = r < nq;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const uint32_t BH64_CONSTANT *cidx = (const uint32_t BH64_CONSTANT *)sidx;
#pragma clang diagnostic pop

    NbList list;
    list.D = nb_lds + lane;
    list.I = reinterpret_cast<uint32_t *>(nb_lds + (size_t)k * kWave) + lane;
    list.k = k; list.cnt = 0; list.kd2 = (double)INFINITY; list.kid = 0u;

    double2 q{0.0, 0.0};
    int32_t s = 0, self = -1;
    if (valid) {
        if (POINTS) {
            q = points[order[r]];
            s = nb_lower_bound(bkeys, n, pkeys[r]);
        } else {
            s = (int32_t)(s0 + r);
            self = s;
            q = spos[s];
        }
    }
    const int32_t lo = s - k, hi = s + k;                      // the seeds: the traversal skips them
    uint32_t ev = 0;
    if (valid) {
        const int32_t j1 = (hi < n - 1) ? hi : n - 1;
        for (int32_t j = (lo > 0) ? lo : 0; j <= j1; ++j) {
            if (j == self) continue;
            const double2 p = spos[j];
            const double dx = p.x - q.x, dy = p.y - q.y;
            ++ev;
            list.insert(dx * dx + dy * dy, sidx[j]);
        }
    }

    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool mine, const NbNode &nd) {
                double unused;
                const double lb = nb_bound<false>(nd.box, q, unused);
                return mine && list.wants(lb);
            },
            [&](const bool in, const int32_t j, const double px, const double py) {
                const uint32_t id = cidx[j];
                const double dx = px - q.x, dy = py - q.y;
                if (in && (j < lo || j > hi)) {
                    ++ev;
                    list.insert(dx * dx + dy * dy, id);
                }
            });

    if (valid) {
        for (int e = 0; e < k; ++e) {
            const bool have = e < list.cnt;
            out_idx[r * k + e] = have ? (int64_t)list.I[e * kWave] : (int64_t)-1;
            out_d2[r * k + e] = have ? list.D[e * kWave] : (double)INFINITY;
        }
        evals[r] = ev;
    }
}

// bodies with d2 <= r2 of the same queries (no list, no seeds); counts[r]
template <bool POINTS>
__global__ __launch_bounds__(kBlock) void nb_count_kernel(const double2 *__restrict__ spos, const NbBox *__restrict__ boxes,
                                                          const int32_t *__restrict__ off, int32_t levels, int32_t n,
                                                          const double2 *__restrict__ points, const uint32_t *__restrict__ order,
                                                          int64_t s0, int64_t nq, double r2, uint32_t *__restrict__ counts)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < nq;

    double2 q{0.0, 0.0};
    int32_t self = -1;
    if (valid) {
        if (POINTS) q = points[order[r]];
        else { self = (int32_t)(s0 + r); q = spos[self]; }
    }
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

}  // namespace bh
