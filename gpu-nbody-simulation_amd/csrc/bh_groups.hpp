// bh_groups.hpp -- friends-of-friends groups of the current state and their catalogue (bh_groups, bh_groups_catalogue).  The
// reference has no such output.  Included by bh_engine.hip after bh_neighbours.hpp, so it is compiled with -ffp-contract=off:
// nothing below is fused.
//
// Definition.  For bodies i != j: dx = x_j - x_i, dy = y_j - y_i, d2 = dx * dx + dy * dy in fp64 (an fp32 state is widened
// first, which is exact) -- the d2 of bh_count_within, symmetric in (i, j) because rounding is symmetric in the sign.  i and j
// are friends when d2 <= b2, b2 = linking_length * linking_length formed once on the host.  A group is a connected component
// of that relation; its label is the smallest caller index in it.
//
// Structure: the index of bh_neighbours.hpp as nb_build leaves it -- spos, sidx, slot, the boxes and their level table.
// Everything below works on SORTED positions s; caller indices appear at the very end (grp_flatten_kernel's atomicMin).
//
// Clique nodes.  A node of any level whose box has (hix - lox) * (hix - lox) + (hiy - loy) * (hiy - loy) <= b2 holds mutual
// friends only: for two bodies of the box |dx| <= hix - lox as computed (rounded subtraction is monotone), so d2 <= that sum
// (the argument of ub in bh_neighbours.hpp).  A child's box lies inside its parent's and its extents are not larger as
// computed, so below a clique node everything is a clique node: a leaf has a HIGHEST clique ancestor or none.
// grp_init_kernel walks up from every body's leaf while the boxes pass and sets parent[s] to the first sorted position of that
// highest node (else to s): the bodies of a dense core are one tree before a single distance is computed, and nobody pays a
// union per friend pair there.
//
// Link kernel (grp_link_kernel): nb_walk (bh_neighbours.hpp), one lane per body in sorted order; a lane takes part in a node
// only if lb <= b2.  The lane at s links to positions j < s only and leaves out a node whose first position is >= s, so every
// unordered pair is looked at once, by its later member.  A clique node
//   * that holds s: left out (its bodies are one tree since grp_init_kernel);
//   * whole (ub <= b2): one union with its first body, not opened;
//   * else: opened, and the lane links to its first friend in it only -- `done`, the end of the highest clique node of the
//     path (wave-uniform `cend`, set when that node is popped: the traversal visits positions in ascending order, so a node is
//     inside the current clique node exactly when its first position is below cend) keeps the lane out of the rest.
// Everything else links pair by pair at the leaves.  Every such decision rests on boxes, distances and sorted positions; none
// reads parent[].  The three counters -- distances computed, friend pairs found (those of grp_init_kernel included: a body and
// the first body of its clique node are friends, and the traversal never finds that pair again), hooks -- are therefore the
// same in every run; the hooks are n - groups whatever their order, since each lowers the number of trees by one.
//
// Union-find.  parent[] over sorted positions, parent[s] <= s always, a root has parent[s] == s: a root is the lowest index of its
// tree.  union(a, b) walks the two bodies up in turn, always the one with the higher index:
//   a == b:  the walks have met at a common ancestor -- one tree, done;
//   hi = max(a, b) is not a root: hi = parent[hi];
//   hi is a root: atomicCAS(&parent[hi], hi, lo).  Success: hi, a root until this instant, hangs under lo.  lo need not be a
//            root: lo < hi, so no cycle can form, and lo's tree now holds all of hi's.  Failure: somebody hooked hi first, the
//            CAS returned its new parent < hi; the walk goes on from there.
// Two walks in one tree meet at its root at the latest, and the root's own word is never read on the way (the root is never
// the higher of the two): in a group of a million bodies that one word would else be read twice per friend pair.
// Termination: every step lowers max(a, b) or the other index: all loops are bounded by the indices themselves, no thread waits
// for another, and a CAS fails only because another thread's CAS succeeded.
// Why stale reads cannot hurt.  MI355X's per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed.
// Inside the link kernel parent[] is read with agent-scope relaxed atomic loads (they pass the L1), and every WRITE to it is a
// read-modify-write atomic (the CAS, and atomicMin for shortening), performed where atomics of the agent are performed, in one
// modification order per word.  Along that order a word only decreases: self -> a lower index (the hook), then lower
// ancestors (shortening).  Hence (1) a non-root never becomes a root again; (2) whatever value of parent[x] a load returns,
// however old, is x itself or a body that was made an ancestor of x by hooks that did happen: a stale read is an older
// ancestor in the same tree; (3) two bodies whose walks meet at one index are in one tree -- stopping there is right; (4) a
// body that LOOKS like a root but has been hooked fails the CAS, which compares against the word itself and not against what
// any cache holds, and the walk continues from the true parent.  Only the CAS decides a hook.
// Shortening.  A walk hands every body it leaves behind its grandparent with atomicMin (path splitting: a walk halves the paths
// it used), and at the end the lane lowers its own parent[s] to the last common ancestor it saw.  Both write only an ancestor,
// and only to a body that a load or a failed CAS has shown below itself -- words only decrease, so it is a non-root for good.
// There is no plain store to parent[] in the
// link kernel, so there is no dirty line whose late write-back could put an old value over a hook: every modification happens
// at the word, in order, and lowers it.  Replacing the parent of a non-root by another of its ancestors leaves every body's
// root unchanged.
//
// Flatten and label are separate launches -- the kernel boundary is the only hand-off relied on -- and read parent[] only:
// root[s] by pointer chasing, atomicMin of sidx[s] into minidx[root], a member count per root (the lanes of a wave that share
// a root send one minimum and one count: the words of a large group's root would else serialise a million atomics), and the
// number of roots; label[sidx[s]] = minidx[root[s]].
//
// Catalogue: the roots with count >= min_members are numbered in any order (grp_compact_kernel), every body of such a group
// adds its five moments  m, m * x, m * y, m * vx, m * vy  (each one fp64 product) to the group's record in the fixed point of
// bh_moments.hpp: exponent 62 - E_p - L per plane from max |q_p| over ALL bodies and L = ceil(log2(max(n, 1))), contribution
// (int64) rint(ldexp(q_p, exponent)), 64-bit integer atomics (the lanes of a wave that feed one group add once).  No overflow,
// the same bits in any order.  The host orders the records by (count descending, label ascending).
#pragma once

#include "bh_neighbours.hpp"

namespace bh {

constexpr int kGrpPlanes = 5;

// what the first catalogue pass leaves: bit patterns of max |q_p| and a flag (as MapMax)
struct GrpMax {
    unsigned long long bits[kGrpPlanes];
    unsigned long long bad;
};

// counters of a call on the device
struct GrpCounters {
    unsigned long long evals, pairs, hooks;     // bh_groups' stats[3]
    unsigned long long roots;                   // all components
    unsigned long long kept;                    // those with count >= min_members
};

struct GrpExp { int32_t e[kGrpPlanes]; };

// wave-level folding of lanes that feed one word (grp_flatten_kernel, grp_sum_kernel): rounds, and the lanes that make a sum
// over the wave worth its shuffles
constexpr int kGrpRounds = 3, kGrpShare = 4;

__device__ __forceinline__ unsigned long long grp_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ uint32_t grp_load(const uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One step of the walk that stands at hi > lo: hi moves to its parent, or -- hi being a root -- is hooked under lo.  from: the
// body the walk came to hi from (kGrpNone: none), which is handed hi's parent, its grandparent.  True: hooked, the union is done.
constexpr uint32_t kGrpNone = ~0u;
__device__ __forceinline__ bool grp_step(uint32_t *parent, uint32_t &hi, uint32_t &from, uint32_t lo, uint32_t &hooks)
{
    uint32_t p = grp_load(parent, hi);
    if (p == hi) {
        p = atomicCAS(parent + hi, hi, lo);
        if (p == hi) { ++hooks; return true; }
        // (somebody else's hook came first: p < hi is hi's parent)
    }
    if (from != kGrpNone) atomicMin(parent + from, p);
    from = hi;
    hi = p;
    return false;
}

// links the trees of a and b; returns a common ancestor of both (the lower end of the hook, or where the walks met); hooks: + 1
// when this call joined two trees.  See the header.
__device__ __forceinline__ uint32_t grp_union(uint32_t *parent, uint32_t a, uint32_t b, uint32_t &hooks)
{
    uint32_t fa = kGrpNone, fb = kGrpNone;
    for (;;) {
        if (a == b) return a;
        if (a > b) { if (grp_step(parent, a, fa, b, hooks)) return b; }
        else if (grp_step(parent, b, fb, a, hooks)) return a;
    }
}

// parent[s] = the first sorted position of the highest clique node over s, or s; prelinked: the bodies with parent[s] != s
__global__ __launch_bounds__(kBlock) void grp_init_kernel(const NbBox *__restrict__ boxes, const int32_t *__restrict__ off,
                                                          int32_t levels, int32_t n, double b2, uint32_t *__restrict__ parent,
                                                          GrpCounters *__restrict__ ctr)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool linked = false;
    if (s < n) {
        const int32_t leaf = (int32_t)(s / kNbLeaf);
        int top = -1;
        for (int l = 0; l < levels; ++l) {
            const NbBox b = boxes[off[l] + (leaf >> (2 * l))];
            const double ex = b.hix - b.lox, ey = b.hiy - b.loy;
            if (!(ex * ex + ey * ey <= b2)) break;
            top = l;
        }
        uint32_t p = (uint32_t)s;
        if (top >= 0) {
            int64_t first, last;
            nb_range(top, leaf >> (2 * top), n, first, last);
            p = (uint32_t)first;
        }
        parent[s] = p;
        linked = p != (uint32_t)s;
    }
    const unsigned long long votes = __ballot(linked);
    if (lane_id() == 0 && votes) {
        const unsigned long long c = (unsigned long long)__popcll(votes);
        atomicAdd(&ctr->pairs, c);
        atomicAdd(&ctr->hooks, c);
    }
}

// the friends of the body at sorted position s among the positions below s, linked in parent[]
__global__ __launch_bounds__(kBlock) void grp_link_kernel(const double2 *__restrict__ spos, const NbBox *__restrict__ boxes,
                                                          const int32_t *__restrict__ off, int32_t levels, int32_t n, double b2,
                                                          uint32_t *__restrict__ parent, GrpCounters *__restrict__ ctr)
{
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = r < n;

    const int32_t s = valid ? (int32_t)r : 0;
    double2 q{0.0, 0.0};
    if (valid) q = spos[s];
    uint32_t mine = (uint32_t)s;           // s or an ancestor of s: where the lane's next union starts
    uint32_t evals = 0, pairs = 0, hooks = 0;
    int32_t done = 0;                      // the lane has nothing more to find below this position ...
    int64_t cend = 0;                      // ... the end of the highest clique node of the path (wave-uniform)
    bool inside = false;                   // the node last visited lies in a clique node (itself or one above; wave-uniform)
    nb_walk(boxes, off, spos, levels, n, valid,
            [&](const bool took, const NbNode &nd) {
                double ub;
                const double lb = nb_bound<true>(nd.box, q, ub);
                const double ex = nd.box.hix - nd.box.lox, ey = nd.box.hiy - nd.box.loy;
                const bool clique = ex * ex + ey * ey <= b2;               // (wave-uniform)
                if (clique && nd.first >= cend) cend = nd.last;
                inside = nd.first < cend;
                bool in = took && lb <= b2 && nd.first < s && nd.first >= done;
                if (clique && s < nd.last) in = false;                     // (the lane's own clique node)
                const bool whole = in && clique && ub <= b2;
                if (whole) {
                    mine = grp_union(parent, mine, (uint32_t)nd.first, hooks);
                    ++pairs;
                    done = (int32_t)cend;
                }
                return in && !whole;
            },
            [&](const bool rest, const int32_t j, const double px, const double py) {
                const double dx = px - q.x, dy = py - q.y;
                if (rest && j < s && j >= done) {
                    ++evals;
                    if (dx * dx + dy * dy <= b2) {
                        mine = grp_union(parent, mine, (uint32_t)j, hooks);
                        ++pairs;
                        if (inside) done = (int32_t)cend;
                    }
                }
            });
    if (valid && mine != (uint32_t)s) atomicMin(parent + s, mine);
    const unsigned long long e = grp_wave_sum(evals), p = grp_wave_sum(pairs), h = grp_wave_sum(hooks);
    if (lane == 0) {
        if (e) atomicAdd(&ctr->evals, e);
        if (p) atomicAdd(&ctr->pairs, p);
        if (h) atomicAdd(&ctr->hooks, h);
    }
}

// root[s]; minidx[root] = the smallest caller index of the tree (minidx preset to ~0), count[root] its bodies (zeroed); roots
__global__ __launch_bounds__(kBlock) void grp_flatten_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ sidx,
                                                             int32_t n, uint32_t *__restrict__ root, uint32_t *__restrict__ minidx,
                                                             uint32_t *__restrict__ count, GrpCounters *__restrict__ ctr)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool is_root = false;
    uint32_t x = 0, id = ~0u;
    if (s < n) {
        x = (uint32_t)s;
        for (;;) { const uint32_t p = parent[x]; if (p == x) break; x = p; }
        root[s] = x;
        is_root = x == (uint32_t)s;
        id = sidx[s];
    }
    // The bodies lie in curve order, so the lanes of a wave have few roots: up to kGrpRounds times the lanes that share the root
    // of the first lane left send one minimum and one count (a million bodies of one group would else queue at two words); the
    // other lanes send their own.  Minimum and sum do not depend on the grouping.
    unsigned long long todo = __ballot(s < n);
    for (int round = 0; round < kGrpRounds && todo != 0ull; ++round) {
        const int first = __builtin_ctzll(todo);
        const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)x, first);
        const bool same = s < n && x == x0;
        const unsigned long long share = __ballot(same);
        todo &= ~share;
        uint32_t lowest = same ? id : ~0u;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)lowest, d, kWave);
            lowest = (o < lowest) ? o : lowest;
        }
        if (lane_id() == first) {
            atomicMin(minidx + x0, lowest);
            atomicAdd(count + x0, (uint32_t)__popcll(share));
        }
    }
    if (((todo >> lane_id()) & 1ull) != 0ull) {
        atomicMin(minidx + x, id);
        atomicAdd(count + x, 1u);
    }
    const unsigned long long votes = __ballot(is_root);
    if (lane_id() == 0 && votes) atomicAdd(&ctr->roots, (unsigned long long)__popcll(votes));
}

// label[caller index of s] = the smallest caller index of its group
__global__ __launch_bounds__(kBlock) void grp_label_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ minidx,
                                                           const uint32_t *__restrict__ sidx, int32_t n, long long *__restrict__ label)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s < n) label[sidx[s]] = (long long)minidx[root[s]];
}

// the roots with count >= min_members get a record g (in any order): gid[root] = g, rec_label[g], rec_count[g]
__global__ __launch_bounds__(kBlock) void grp_compact_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ minidx,
                                                             const uint32_t *__restrict__ count, int32_t n, uint32_t min_members,
                                                             uint32_t *__restrict__ gid, uint32_t *__restrict__ rec_label,
                                                             uint32_t *__restrict__ rec_count, GrpCounters *__restrict__ ctr)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n || root[s] != (uint32_t)s || count[s] < min_members) return;
    const uint32_t g = (uint32_t)atomicAdd(&ctr->kept, 1ull);
    gid[s] = g;
    rec_label[g] = minidx[s];
    rec_count[g] = count[s];
}

template <typename Real2, typename Real>
__device__ __forceinline__ void grp_moments(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel, const Real *__restrict__ mass,
                                            int64_t i, double (&q)[kGrpPlanes])
{
    const Real2 pp = pos[i], vv = vel[i];
    const double m = (double)mass[i];
    q[0] = m;
    q[1] = m * (double)pp.x;
    q[2] = m * (double)pp.y;
    q[3] = m * (double)vv.x;
    q[4] = m * (double)vv.y;
}

// max |q_p| over all bodies (out zeroed); bad: a velocity, mass or moment that is not finite (positions: the bounds pass)
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void grp_max_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                         const Real *__restrict__ mass, int64_t n, GrpMax *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a[kGrpPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    if (i < n) {
        const Real2 vv = vel[i];
        double q[kGrpPlanes];
        grp_moments(pos, vel, mass, i, q);
        bad = !(map_finite((double)vv.x) && map_finite((double)vv.y));
#pragma unroll
        for (int p = 0; p < kGrpPlanes; ++p) bad |= !map_finite(q[p]);
#pragma unroll
        for (int p = 0; p < kGrpPlanes; ++p) a[p] = bad ? 0.0 : fabs(q[p]);
    }
#pragma unroll
    for (int p = 0; p < kGrpPlanes; ++p) a[p] = wave_max(a[p]);
    const bool wbad = __ballot(bad) != 0ull;
    if (lane_id() == 0) {
#pragma unroll
        for (int p = 0; p < kGrpPlanes; ++p) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(a[p]);
            if (bits) atomicMax(&out->bits[p], bits);
        }
        if (wbad) atomicOr(&out->bad, 1ull);
    }
}

// sums[g][p] += the fixed-point moments of every body whose group has a record (sums zeroed)
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void grp_sum_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                         const Real *__restrict__ mass, const uint32_t *__restrict__ slot,
                                                         const uint32_t *__restrict__ root, const uint32_t *__restrict__ count,
                                                         const uint32_t *__restrict__ gid, int32_t n, uint32_t min_members, GrpExp ex,
                                                         unsigned long long *__restrict__ sums)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool kept = false;
    uint32_t g = 0;
    long long v[kGrpPlanes] = {0, 0, 0, 0, 0};
    if (s < n) {
        const uint32_t rt = root[s];
        kept = count[rt] >= min_members;
        if (kept) {
            g = gid[rt];
            double q[kGrpPlanes];
            grp_moments(pos, vel, mass, (int64_t)slot[s], q);
#pragma unroll
            for (int p = 0; p < kGrpPlanes; ++p) v[p] = (long long)rint(ldexp(q[p], ex.e[p]));
        }
    }
    // The bodies lie in curve order, so the lanes of a wave feed few groups: up to kGrpRounds times the group of the first lane
    // left is summed over the wave and added once per plane (when at least kGrpShare lanes share it); the other lanes add
    // their own.  Integer sums: the same bits either way.
    unsigned long long todo = __ballot(kept);
    for (int round = 0; round < kGrpRounds && todo != 0ull; ++round) {
        const int first = __builtin_ctzll(todo);
        const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)g, first);
        const bool same = kept && g == g0;
        const unsigned long long share = __ballot(same);
        todo &= ~share;
        if (__popcll(share) < kGrpShare) {
#pragma unroll
            for (int p = 0; p < kGrpPlanes; ++p)
                if (same && v[p]) atomicAdd(sums + (size_t)g * kGrpPlanes + p, (unsigned long long)v[p]);
            continue;
        }
#pragma unroll
        for (int p = 0; p < kGrpPlanes; ++p) {
            const unsigned long long t = grp_wave_sum(same ? (unsigned long long)v[p] : 0ull);
            if (lane_id() == first && t) atomicAdd(sums + (size_t)g0 * kGrpPlanes + p, t);
        }
    }
    const bool left = ((todo >> lane_id()) & 1ull) != 0ull;
#pragma unroll
    for (int p = 0; p < kGrpPlanes; ++p)
        if (left && v[p]) atomicAdd(sums + (size_t)g * kGrpPlanes + p, (unsigned long long)v[p]);
}

}  // namespace bh
