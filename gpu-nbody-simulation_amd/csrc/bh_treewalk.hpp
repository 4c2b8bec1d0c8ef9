// bh_treewalk.hpp -- the one traversal of the side walks: the potential walk (bh_diag.hpp) and the field at arbitrary
// points (bh_field.hpp).  Included through bh_engine.hip, so it is compiled with -ffp-contract=off: no multiply-add below
// is fused unless it is written as one.  (The force walks keep their own loops: bh_walk_f64.hpp, bh_walk_exact.hpp,
// bh_walk_fast.hip.)
//
// Term set.  EXACTLY the nodes the precision's force walk takes for a walker at p (project.cu:617-658): the same
// empty-node cut-off, the same acceptance -- read from the node data the force walks compare against (the NodeD `size`
// slot as a d2 threshold or a size per DiagAccept, QuadF.thr) with the mode's own d2 expression -- the same depth-cap
// aggregates and fp32 bucket leaves.  A caller states two things only: whether a leaf is the walker's own (`self`; the
// fp32 tree skips a body at d2 == 0 instead), and what an accepted node adds to which sums (`term`).
//
// Launch shape: the one the fp32 and fp64 throughput walks were measured best with -- one wavefront per 64 consecutive
// walkers of a sorted order, the nodes read with scalar loads (wave-uniform addresses in the constant address space), a
// four-sibling quad per stack entry, the traversal stack in VGPRs addressed by lane with the mask of the lanes that
// opened the quad.  A lane's terms run in the fixed depth-first order of the wave's traversal restricted to the lane's
// own nodes (siblings in index order, then the opened quads last first): what a lane sums does not depend on who shares
// its wavefront.
#pragma once

#include "bh_tree.hpp"
#include "bh_walk_f64.hpp"

namespace bh {

// acceptance of a subdivided fp64 cell, as the force walk of the mode states it
enum DiagAccept : int {
    kAcceptThr = 0,        // BH_PRECISION_F64: thr < d2, d2 = fma(dx, dx, dy * dy) (walk_f64_kernel)
    kAcceptExactThr = 1,   // BH_PRECISION_F64_EXACT: d2 >= thr, d2 = dx * dx + dy * dy (walk_exact_kernel, THR)
    kAcceptSize = 2        // BH_PRECISION_F64_EXACT + BH_FLAG_WALK_PORTABLE: size / d < theta (walk_exact_kernel, !THR)
};

// register-lane traversal stack, 128 entries of {node or quad index, lane mask}: entry k in lane k & 63 of the first or
// second triple of VGPRs, wave-uniform pointer sp (depth-first pushing every opened quad needs at most 3 * max_depth + 4)
struct LaneStack {
    int32_t base = 0, lo = 0, hi = 0, base2 = 0, lo2 = 0, hi2 = 0;
    int sp = 0;
    __device__ __forceinline__ void push(int32_t idx, uint64_t mask)
    {
        if (sp < kWave) {
            base = bh64_writelane_i32(idx, sp, base);
            lo = bh64_writelane_i32((int32_t)(uint32_t)mask, sp, lo);
            hi = bh64_writelane_i32((int32_t)(uint32_t)(mask >> 32), sp, hi);
        } else if (sp < 2 * kWave) {
            base2 = bh64_writelane_i32(idx, sp - kWave, base2);
            lo2 = bh64_writelane_i32((int32_t)(uint32_t)mask, sp - kWave, lo2);
            hi2 = bh64_writelane_i32((int32_t)(uint32_t)(mask >> 32), sp - kWave, hi2);
        }
        ++sp;                  // (beyond 128 cannot happen: 3 * 31 + 4 entries at max_depth 32)
    }
    __device__ __forceinline__ void pop(int32_t &idx, uint64_t &mask)
    {
        --sp;
        if (sp < kWave) {
            idx = __builtin_amdgcn_readlane(base, sp);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, sp) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, sp);
        } else {
            idx = __builtin_amdgcn_readlane(base2, sp - kWave);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi2, sp - kWave) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane(lo2, sp - kWave);
        }
    }
};

// ---- fp64 tree (NodeD / LinkD): the root alone, then quads of four siblings ------------------------------------------
// self(occ): the leaf with this occupant is the walker's own and is skipped.  term(m, dx, dy, s2, d), s2 = d2 + eps2,
// d = sqrt(s2) + 1e-15 (project.cu:634 at eps2 = 0): an accepted node.  Acceptance is decided on the geometric d2 -- eps2,
// the square of the Plummer softening length (bh_set_softening), enters the term only; d2 + 0.0 is d2 bit for bit (d2 >= +0
// or NaN), so eps2 = 0 is the unsoftened walk.  kAcceptSize keeps the geometric d for its criterion; the term takes that one
// again where eps2 = 0 and a softened d of its own otherwise.  EAGER_D false (the field, whose term is a square root
// and four divisions): d and the term run under the accepting lanes only, behind a wave-uniform test that skips them
// where no lane accepts -- except that kAcceptSize, whose criterion itself needs it, forms the geometric d for every node
// (and with eps2 > 0 the term's d under the accepting lanes as well).  EAGER_D true
// (the potential, whose term is one division): d for every node and no such test -- deciding first was measured never
// faster for the fp64 potential walk and 2 to 10 % slower at 65,536 bodies ("One traversal").  d is
// a function of d2 alone, so where it is formed changes no bit.
template <int ACCEPT, bool EAGER_D, typename Self, typename Term>
__device__ __forceinline__ void walk_nodes_f64(const NodeD *__restrict__ gd, const LinkD *__restrict__ ld, const double2 p,
                                               const bool valid, const double theta, const double eps2, Self self, Term term)
{
    const int lane = lane_id();
    LaneStack st;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const NodeD BH64_CONSTANT *cg = (const NodeD BH64_CONSTANT *)gd;
    const LinkD BH64_CONSTANT *cl = (const LinkD BH64_CONSTANT *)ld;
#pragma clang diagnostic pop

    auto eval = [&](int32_t node, uint64_t mask) {
        NodeD q;
        q.cx = cg[node].cx; q.cy = cg[node].cy; q.m = cg[node].m; q.size = cg[node].size;
        LinkD k;
        k.child = cl[node].child; k.occ = cl[node].occ;
        if (q.m <= 1e-15) return;                                  // project.cu:617
        const double dx = q.cx - p.x, dy = q.cy - p.y;
        const double d2 = (ACCEPT == kAcceptThr) ? fma(dx, dx, dy * dy) : dx * dx + dy * dy;
        const bool leaf = k.child < 0;
        const double s2 = d2 + eps2;
        double d = 0.0, dg = 0.0;
        if (ACCEPT == kAcceptSize) dg = sqrt(d2) + 1e-15;          // project.cu:643: the criterion itself needs the geometric d
        // the term's d: with eps2 = 0 (wave-uniform) s2 is d2 bit for bit, and kAcceptSize's dg serves again -- one square
        // root per node, as before there was a softening; otherwise a root of its own
        auto term_d = [&] { return (ACCEPT == kAcceptSize && eps2 == 0.0) ? dg : sqrt(s2) + 1e-15; };      // project.cu:634
        bool take;
        if (EAGER_D) d = term_d();
        if (ACCEPT == kAcceptSize) {
            take = leaf ? !self(k.occ) : q.size / dg < theta;
        } else if (ACCEPT == kAcceptThr) {
            take = leaf ? !self(k.occ) : q.size < d2;
        } else {
            take = leaf ? !self(k.occ) : d2 >= q.size;
        }
        const bool mine = ((mask >> lane) & 1ull) != 0ull;
        const bool acc = mine && take;
        if (EAGER_D) {
            if (acc) term(q.m, dx, dy, s2, d);
        } else if (__ballot(acc) != 0ull) {                        // wave-uniform: no lane takes it, no sqrt and no division
            if (acc) {
                d = term_d();
                term(q.m, dx, dy, s2, d);
            }
        }
        if (!leaf) {
            const uint64_t open = mask & __ballot(!take);
            if (open != 0) st.push(k.child, open);
        }
    };

    eval(0, __ballot(valid));
    while (st.sp > 0) {
        int32_t base;
        uint64_t mask;
        st.pop(base, mask);
#pragma unroll
        for (int c = 0; c < 4; ++c) eval(base + c, mask);
    }
}

// ---- QuadF tree (BH_PRECISION_F32, BH_PRECISION_MIXED): walk_fast_kernel's eval and bucket ---------------------------
// term(m, dx, dy, d2), d2 > 0: an accepted node or a bucket body (the geometric d2: a softened term adds eps2 itself).
// walk_quads_f32_from walks the tree whose root quad is
// `root`: 0 for the context's own tree, the first quad of a received block for a peer's locally-essential tree (bh_let.hpp:
// its child links are already indices into `quads`, its depth-cap buckets already aggregates, so `aux` is only ever read
// for the own tree).  Every call starts from an empty stack: a lane's terms of one tree do not depend on the trees walked
// before it.
template <typename Term>
__device__ __forceinline__ void walk_quads_f32_from(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                                    const float2 *__restrict__ spos, const float *__restrict__ smass,
                                                    const int32_t root, const float2 p, const bool valid, Term term)
{
    const int lane = lane_id();
    LaneStack st;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const QuadF BH64_CONSTANT *cq = (const QuadF BH64_CONSTANT *)quads;
    const NodeAux BH64_CONSTANT *ca = (const NodeAux BH64_CONSTANT *)aux;
    const float2 BH64_CONSTANT *cpos = (const float2 BH64_CONSTANT *)spos;
    const float BH64_CONSTANT *cmass = (const float BH64_CONSTANT *)smass;
#pragma clang diagnostic pop

    // one node: empty (m == 0) skipped; accepted iff d2 > thr (leaf: thr = 0, which skips a walker at the leaf's own
    // place; bucket: +inf, opened by all)
    auto eval = [&](const float cx, const float cy, const float m, const float thr, const int32_t child, const uint64_t mask) {
        if (__float_as_int(m) == 0) return;
        const float dx = cx - p.x, dy = cy - p.y;
        const float d2 = __builtin_fmaf(dx, dx, dy * dy);
        const uint64_t farm = __ballot(d2 > thr);
        if ((mask & farm) >> lane & 1ull) term(m, dx, dy, d2);
        if (child != -1) {                                         // subdivided cell (> 0) or bucket reference (<= -2)
            const uint64_t open = mask & ~farm;
            if (open != 0) st.push(child, open);
        }
    };
    // a depth-cap cell of several bodies (compat off), body by body; a body at the walker's place contributes nothing
    auto bucket = [&](const int32_t node, const uint64_t mask) {
        const int32_t first = ca[node].first, count = ca[node].count;
        for (int32_t j = first; j < first + count; ++j) {
            const float2 o = float2{cpos[j].x, cpos[j].y};
            const float om = cmass[j];
            const float dx = o.x - p.x, dy = o.y - p.y;
            const float d2 = __builtin_fmaf(dx, dx, dy * dy);
            if ((mask & __ballot(d2 > 0.f)) >> lane & 1ull) term(om, dx, dy, d2);
        }
    };
    auto eval_quad = [&](const int32_t q, const uint64_t mask) {
#pragma unroll
        for (int c = 0; c < 4; ++c) eval(cq[q].xy[2 * c], cq[q].xy[2 * c + 1], cq[q].m[c], cq[q].thr[c], cq[q].child[c], mask);
    };

    eval_quad(root, __ballot(valid));                              // the root quad: the root in slot 0
    while (st.sp > 0) {
        int32_t base;
        uint64_t mask;
        st.pop(base, mask);
        if (base > 0) eval_quad(base, mask);
        else if (base <= -2) bucket(-base - 2, mask);              // (-1, a leaf, is never pushed)
    }
}

// the context's own tree: root quad 0
template <typename Term>
__device__ __forceinline__ void walk_quads_f32(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                               const float2 *__restrict__ spos, const float *__restrict__ smass, const float2 p,
                                               const bool valid, Term term)
{
    walk_quads_f32_from(quads, aux, spos, smass, 0, p, valid, term);
}

}  // namespace bh
