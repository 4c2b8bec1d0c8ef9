// bh_field.hpp -- the Barnes-Hut field at arbitrary points (bh_field_at): acceleration, potential and term count at
// caller coordinates that are nobody's.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: no
// multiply-add below is fused unless it is written as one.
//
// Term set.  Exactly the terms the precision's force walk would take for a body standing at the point that is no body of
// the tree: the `mass <= 1e-15` cut-off (fp32: m == 0), the acceptance read from the node data the force walk compares
// against (the NodeD size slot as a threshold or a size per DiagAccept, QuadF.thr) with the mode's own d2 expression,
// depth-cap aggregates as point masses, fp32 bucket leaves body by body -- and NO self skip by index: a leaf is always
// taken.
//   fp64 modes: d = sqrt(d2) + 1e-15, f = (G M) / d2, a += f * (dx / d), phi -= (G M) / d (project.cu:630-658 with
//               m_i = 1), IEEE sqrt and division.  A point that coincides with a body gets what that expression gives:
//               inf * 0, a non-finite acceleration.
//   F32 / MIXED: the point is rounded to fp32 here; ri = v_rsq_f32(d2), w = m ri ri ri, the terms w dx, w dy and m ri in
//               fp32, summed in fp64 and multiplied by G in fp64 at the end.  A node or bucket body at d2 == 0 gives nothing.
//
// Order of the points.  One wavefront walks 64 points together and opens the union of their walks, so the points are
// put in Morton order first: field_keys_kernel maps a point to 16 bits per axis in the tree's root box (clamped: points
// outside are valid) with the point's index of the launch in the key word above bit 40, and the LSD passes of bh_sort.hpp
// (radix_hist / radix_rowscan / radix_scatter_w, the packed-key instantiations the tree build already uses) sort the 32
// key bits.  The walk kernels read points[order[s]] and write the results at order[s]: caller order.
//
// Walk.  The launch shape of the potential walk (bh_diag.hpp): one wavefront per 64 sorted points, node data through
// the constant address space (scalar loads), the DiagStack register-lane stack with one entry per opened quad and the
// mask of the lanes that opened it.  Acceptance is decided on d2; the square root and the divisions run under the
// accepting lanes only, behind a wave-uniform test that skips them where no lane accepts (DESIGN section 12 measured what
// evaluating d for every node costs) -- except in the kAcceptSize variant, whose criterion itself needs d.
// A lane's terms are added in the fixed depth-first order of the wave's traversal restricted to the lane's own nodes
// (siblings in index order, then the opened quads last first), with plain fp64 adds: a point's result does not depend
// on which points share its wavefront, launch or call.
#pragma once

#include "bh_diag.hpp"

namespace bh {

constexpr int64_t kFieldChunk = (int64_t)1 << 20;     // points per launch (their indices travel in key bits 40..59)
constexpr int kFieldSortItems = 4;                     // keys per thread in the sort passes: tiles of 1,024
constexpr int kFieldKeyBits = 32;                      // 16 bits per axis

// the bits of v (< 2^16) spread to the even positions
__device__ __forceinline__ uint32_t field_spread16(uint32_t v)
{
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// cell of a coordinate among 65,536 across [lo, hi], clamped; a degenerate box puts everything in cell 0
__device__ __forceinline__ uint32_t field_cell16(double x, double lo, double hi)
{
    const double w = hi - lo;
    if (!(w > 0.0) || !(w < 1.7e308)) return 0u;
    double t = (x - lo) * (65536.0 / w);
    t = (t > 0.0) ? t : 0.0;                                   // (also a NaN, which the host has refused already)
    t = (t < 65535.0) ? t : 65535.0;
    return (uint32_t)t;
}

// keys[i] = Morton key of point i of the launch in the root box | i << kPackShift
__global__ __launch_bounds__(kBlock) void field_keys_kernel(const double2 *__restrict__ points, int64_t k,
                                                            const double *__restrict__ box, uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= k) return;
    const double2 p = points[i];
    const uint32_t ix = field_cell16(p.x, box[0], box[1]), iy = field_cell16(p.y, box[2], box[3]);
    const uint64_t key = (uint64_t)(field_spread16(ix) | (field_spread16(iy) << 1));
    keys[i] = key | ((uint64_t)i << kPackShift);
}

// ---- fp64 tree (BH_PRECISION_F64_EXACT, BH_PRECISION_F64): one wavefront per 64 sorted points ----------------------
template <int ACCEPT>
__global__ __launch_bounds__(kBlock) void field_f64_kernel(const NodeD *__restrict__ gd, const LinkD *__restrict__ ld,
                                                           const uint32_t *__restrict__ order, const double2 *__restrict__ points,
                                                           int64_t k, double theta, double G, const TreeCounters *ctr,
                                                           double2 *__restrict__ accel, double *__restrict__ phi,
                                                           uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < k;
    const uint32_t slot = valid ? order[s] : 0u;
    const double2 p = valid ? points[slot] : double2{0.0, 0.0};
    double ax = 0.0, ay = 0.0, ph = 0.0;
    uint32_t cnt = 0;
    DiagStack st;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const NodeD BH64_CONSTANT *cg = (const NodeD BH64_CONSTANT *)gd;
    const LinkD BH64_CONSTANT *cl = (const LinkD BH64_CONSTANT *)ld;
#pragma clang diagnostic pop

    auto eval = [&](int32_t node, uint64_t mask) {
        NodeD q;
        q.cx = cg[node].cx; q.cy = cg[node].cy; q.m = cg[node].m; q.size = cg[node].size;
        const int32_t child = cl[node].child;
        if (q.m <= 1e-15) return;                                  // project.cu:617
        const double dx = q.cx - p.x, dy = q.cy - p.y;
        const double d2 = (ACCEPT == kAcceptThr) ? fma(dx, dx, dy * dy) : dx * dx + dy * dy;
        const bool leaf = child < 0;
        double d = 0.0;
        bool take;
        if (ACCEPT == kAcceptSize) {
            d = sqrt(d2) + 1e-15;                                  // project.cu:634: the criterion itself needs d
            take = leaf || q.size / d < theta;                     // project.cu:643
        } else if (ACCEPT == kAcceptThr) {
            take = leaf || q.size < d2;
        } else {
            take = leaf || d2 >= q.size;
        }
        const bool mine = ((mask >> lane) & 1ull) != 0ull;
        const bool acc = mine && take;
        if (__ballot(acc) != 0ull) {                               // wave-uniform: no lane takes it, no sqrt and no division
            if (acc) {
                if (ACCEPT != kAcceptSize) d = sqrt(d2) + 1e-15;
                const double gm = G * q.m;
                const double f = gm / d2;                          // project.cu:651-658 with m_i = 1
                ax += f * (dx / d);
                ay += f * (dy / d);
                ph += gm / d;
                ++cnt;
            }
        }
        if (!leaf) {
            const uint64_t open = mask & __ballot(!take);
            if (open != 0) st.push(child, open);
        }
    };

    eval(0, __ballot(valid));                                 // the root alone, then quads of four siblings
    while (st.sp > 0) {
        int32_t base;
        uint64_t mask;
        st.pop(base, mask);
#pragma unroll
        for (int c = 0; c < 4; ++c) eval(base + c, mask);
    }
    if (valid) {
        accel[slot] = double2{ax, ay};
        phi[slot] = -ph;
        counts[slot] = cnt;
    }
}

// ---- QuadF tree (BH_PRECISION_F32, BH_PRECISION_MIXED): the fp32 walk's terms, fp64 sums ------------------------------
__global__ __launch_bounds__(kBlock) void field_f32_kernel(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                                           const float2 *__restrict__ spos, const float *__restrict__ smass,
                                                           const uint32_t *__restrict__ order, const double2 *__restrict__ points,
                                                           int64_t k, double G, const TreeCounters *ctr,
                                                           double2 *__restrict__ accel, double *__restrict__ phi,
                                                           uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < k;
    const uint32_t slot = valid ? order[s] : 0u;
    const double2 pd = valid ? points[slot] : double2{0.0, 0.0};
    const float2 p = float2{(float)pd.x, (float)pd.y};             // the point as the fp32 walk would hold it
    double ax = 0.0, ay = 0.0, ph = 0.0;
    uint32_t cnt = 0;
    DiagStack st;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const QuadF BH64_CONSTANT *cq = (const QuadF BH64_CONSTANT *)quads;
    const NodeAux BH64_CONSTANT *ca = (const NodeAux BH64_CONSTANT *)aux;
    const float2 BH64_CONSTANT *cpos = (const float2 BH64_CONSTANT *)spos;
    const float BH64_CONSTANT *cmass = (const float BH64_CONSTANT *)smass;
#pragma clang diagnostic pop

    // the fp32 walk's term of a mass m at (dx, dy), d2 > 0 (walk_fast_kernel: rsq, m ri ri ri)
    auto term = [&](const float m, const float dx, const float dy, const float d2) {
        const float ri = __builtin_amdgcn_rsqf(d2);
        const float mri = m * ri;
        const float w = mri * ri * ri;
        ax += (double)(w * dx);
        ay += (double)(w * dy);
        ph += (double)mri;
        ++cnt;
    };
    // one node: empty (m == 0) skipped; accepted iff d2 > thr (leaf: thr = 0; bucket: +inf, opened by all)
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
    // a depth-cap cell of several bodies (compat off), body by body; a body at the point itself contributes nothing
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

    eval_quad(0, __ballot(valid));                                 // quad 0: the root in slot 0
    while (st.sp > 0) {
        int32_t base;
        uint64_t mask;
        st.pop(base, mask);
        if (base > 0) eval_quad(base, mask);
        else if (base <= -2) bucket(-base - 2, mask);              // (-1, a leaf, is never pushed)
    }
    if (valid) {
        accel[slot] = double2{G * ax, G * ay};
        phi[slot] = -G * ph;
        counts[slot] = cnt;
    }
}

}  // namespace bh
