// bh_field.hpp -- the Barnes-Hut field at arbitrary points (bh_field_at): acceleration, potential and term count at
// caller coordinates that are nobody's.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: no
// multiply-add below is fused unless it is written as one.
//
// Term set.  Exactly the terms the precision's force walk would take for a body standing at the point that is no body of
// the tree: the traversal of bh_treewalk.hpp with NO self skip by index -- a leaf is always taken.
//   fp64 modes: d = sqrt(d2) + 1e-15, f = (G M) / d2, a += f * (dx / d), phi -= (G M) / d (project.cu:630-658 with
//               m_i = 1), IEEE sqrt and division.  A point that coincides with a body gets what that expression gives:
//               inf * 0, a non-finite acceleration.
//   F32 / MIXED: the point is rounded to fp32 here; ri = v_rsq_f32(d2), w = m ri ri ri, the terms w dx, w dy and m ri in
//               fp32, summed in fp64 and multiplied by G in fp64 at the end.  A node or bucket body at d2 == 0 gives nothing.
//   Plummer softening (bh_set_softening): the same expressions at s2 = d2 + eps2 -- d = sqrt(s2) + 1e-15, f = (G M) / s2;
//               ri = v_rsq_f32(d2 + eps2) -- on the unchanged term set.  eps2 = 0 adds 0.0 / 0.f: the unsoftened field bit for bit.
//
// Order of the points.  One wavefront walks 64 points together and opens the union of their walks, so the points are
// put in Morton order first: field_keys_kernel maps a point to 16 bits per axis in the tree's root box (clamped: points
// outside are valid) with the point's index of the launch in the key word above bit 40, and the LSD passes of bh_sort.hpp
// (radix_hist / radix_rowscan / radix_scatter_w, the packed-key instantiations the tree build already uses) sort the 32
// key bits.  The walk kernels read points[order[s]] and write the results at order[s]: caller order.
//
// Walk.  One wavefront per 64 sorted points through the traversal of bh_treewalk.hpp; a lane's terms are added in that
// traversal's fixed order with plain fp64 adds: a point's result does not depend on which points share its wavefront,
// launch or call.
#pragma once

#include "bh_treewalk.hpp"

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
                                                           int64_t k, double theta, double G, double eps2,
                                                           const TreeCounters *ctr, double2 *__restrict__ accel,
                                                           double *__restrict__ phi, uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < k;
    const uint32_t slot = valid ? order[s] : 0u;
    const double2 p = valid ? points[slot] : double2{0.0, 0.0};
    double ax = 0.0, ay = 0.0, ph = 0.0;
    uint32_t cnt = 0;
    walk_nodes_f64<ACCEPT, false>(
        gd, ld, p, valid, theta, eps2, [](int32_t) { return false; },
        [&](double m, double dx, double dy, double s2, double d) {
            const double gm = G * m;
            const double f = gm / s2;                              // project.cu:651-658 with m_i = 1
            ax += f * (dx / d);
            ay += f * (dy / d);
            ph += gm / d;
            ++cnt;
        });
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
                                                           int64_t k, double G, float eps2, const TreeCounters *ctr,
                                                           double2 *__restrict__ accel, double *__restrict__ phi,
                                                           uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < k;
    const uint32_t slot = valid ? order[s] : 0u;
    const double2 pd = valid ? points[slot] : double2{0.0, 0.0};
    const float2 p = float2{(float)pd.x, (float)pd.y};             // the point as the fp32 walk would hold it
    double ax = 0.0, ay = 0.0, ph = 0.0;
    uint32_t cnt = 0;
    // the fp32 walk's term of a mass m at (dx, dy), d2 > 0 (walk_fast_kernel: rsq, m ri ri ri)
    walk_quads_f32(quads, aux, spos, smass, p, valid, [&](const float m, const float dx, const float dy, const float d2) {
        const float ri = __builtin_amdgcn_rsqf(d2 + eps2);
        const float mri = m * ri;
        const float w = mri * ri * ri;
        ax += (double)(w * dx);
        ay += (double)(w * dy);
        ph += (double)mri;
        ++cnt;
    });
    if (valid) {
        accel[slot] = double2{G * ax, G * ay};
        phi[slot] = -G * ph;
        counts[slot] = cnt;
    }
}

}  // namespace bh
