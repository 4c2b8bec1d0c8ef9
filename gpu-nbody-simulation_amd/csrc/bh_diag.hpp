// bh_diag.hpp -- on-device diagnostics: the potential walk and the energy / momentum reductions (bh_compute_potential,
// bh_energy; in the distributed step bh_let_potential, bh_let_energy).  The reference has no potential or energy at all: its only outputs are positions, forces and the quadtree
// files.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: every fused multiply-add below is written out.
//
// Potential walk.  phi_i = -G sum_j M_j / d_ij over EXACTLY the terms the precision's force walk takes for body i: the
// traversal of bh_treewalk.hpp with the force walk's self skip (the tests compare per-body term counts).  One wavefront per
// 64 consecutive bodies of the sorted order; every body is walked in one launch.
//   fp64 modes: term M / d, d = sqrt(d2) + 1e-15 (project.cu:630-634) -- IEEE sqrt and division, correctly rounded --
//               summed per lane with Neumaier compensation, times -G at the end.
//   F32 / MIXED: the fp32 walk's d2 from the fp32 sorted positions, its 1/d = v_rsq_f32(d2), the fp32 term M / d,
//               accumulated in fp64.
//   Plummer softening (bh_set_softening): the terms above at s2 = d2 + eps2 -- sqrt(s2) + 1e-15, v_rsq_f32(d2 + eps2) -- on the
//               unchanged term set; eps2 = 0 adds 0.0 / 0.f, the identity, and is the unsoftened potential bit for bit.
//
// Reductions.  One fp64 term per body for each of: m, m x, m y, m vx, m vy, m (x vy - y vx), m |v|^2, m phi.  kDiagParts
// workgroups take fixed grid-strided bodies, each lane keeps a Neumaier (sum, compensation) pair per quantity, and the
// pairs are folded in a fixed tree inside the workgroup and then, in a second one-workgroup launch, over the workgroups:
// the same state gives the same bits every call.  Eight doubles reach the host.
#pragma once

#include "bh_treewalk.hpp"

namespace bh {

constexpr int kDiagParts = 256;        // workgroups of the first reduction pass (= threads of the second)
constexpr int kDiagQuantities = 8;     // m, mx, my, mvx, mvy, Lz, m|v|^2, m phi

// Neumaier: s + x into the pair (s, c)
__device__ __forceinline__ void neumaier_add(double &s, double &c, double x)
{
    const double t = s + x;
    c += (fabs(s) >= fabs(x)) ? ((s - t) + x) : ((x - t) + s);
    s = t;
}

// (s, c) += (s2, c2)
__device__ __forceinline__ void neumaier_fold(double &s, double &c, double s2, double c2)
{
    neumaier_add(s, c, s2);
    c += c2;
}

// ---- fp64 tree (BH_PRECISION_F64_EXACT, BH_PRECISION_F64): one wavefront per 64 sorted bodies ---------------------
// phi / counts are written at the body's caller index (the state order of these modes).
template <bool COMPAT, int ACCEPT>
__global__ __launch_bounds__(kBlock) void potential_f64_kernel(const NodeD *__restrict__ gd, const LinkD *__restrict__ ld,
                                                               const uint32_t *__restrict__ perm, const double2 *__restrict__ pos,
                                                               int64_t n, double theta, double G, double eps2,
                                                               const TreeCounters *ctr, double *__restrict__ phi,
                                                               uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n;
    const int64_t body = valid ? (int64_t)perm[s] : -1;
    const double2 p = valid ? pos[body] : double2{0.0, 0.0};
    const int32_t body32 = (int32_t)body, alt32 = -2 - body32;     // occ == i, occ + 2 == -i (project.cu:646)
    double sum = 0.0, comp = 0.0;
    uint32_t cnt = 0;
    walk_nodes_f64<ACCEPT, true>(
        gd, ld, p, valid, theta, eps2,
        [&](int32_t occ) { return occ == body32 || (COMPAT && occ == alt32); },   // project.cu:623-626, 646
        [&](double m, double, double, double, double d) { neumaier_add(sum, comp, m / d); ++cnt; });
    if (valid) {
        phi[body] = -G * (sum + comp);
        if (counts) counts[body] = cnt;
    }
}

// ---- QuadF tree (BH_PRECISION_F32, BH_PRECISION_MIXED): the fp32 walk's terms; self and coincident bodies give nothing
// phi / counts are written at the body's device slot perm[s] (the state order of these modes).
__global__ __launch_bounds__(kBlock) void potential_f32_kernel(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                                               const float2 *__restrict__ spos, const float *__restrict__ smass,
                                                               const uint32_t *__restrict__ perm, int64_t n, double G,
                                                               float eps2, const TreeCounters *ctr, double *__restrict__ phi,
                                                               uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n;
    const float2 p = valid ? spos[s] : float2{0.f, 0.f};
    double sum = 0.0;
    uint32_t cnt = 0;
    walk_quads_f32(quads, aux, spos, smass, p, valid, [&](float m, float, float, float d2) {
        const float ri = __builtin_amdgcn_rsqf(d2 + eps2);
        sum += (double)(m * ri);
        ++cnt;
    });
    if (valid) {
        const uint32_t slot = perm[s];
        phi[slot] = -G * sum;
        if (counts) counts[slot] = cnt;
    }
}

// ---- forest of the distributed step (LET mode, bh_let.hpp): the own tree, then every peer's received tree ------------
// The trees in the order of the one-wave forest force walk (bh_walk_fast.hip): the own tree from quad 0 -- own buckets body by
// body, a body at the walker's place gives nothing -- then the received locally-essential tree of every peer in rank order,
// the own rank skipped, from its root quad forest_base + t * let_cap (remote buckets arrive as aggregates, links past a
// truncated block are cut by the packer: the walk never leaves the forest array).  Same term and accumulation as
// potential_f32_kernel; one traversal per tree from an empty stack, so a lane's sum is its own nodes in that fixed order.
// Writes phi and counts at the body's device slot perm[s], nothing else.
__global__ __launch_bounds__(kBlock) void forest_potential_f32_kernel(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                                                      const float2 *__restrict__ spos, const float *__restrict__ smass,
                                                                      const uint32_t *__restrict__ perm, int64_t n, double G,
                                                                      float eps2, const TreeCounters *ctr, int32_t n_trees, int32_t self_rank,
                                                                      int64_t forest_base, int64_t let_cap, double *__restrict__ phi,
                                                                      uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n;
    const float2 p = valid ? spos[s] : float2{0.f, 0.f};
    double sum = 0.0;
    uint32_t cnt = 0;
    for (int32_t t = -1; t < n_trees; ++t) {                       // (wave-uniform: kernel arguments only)
        if (t == self_rank) continue;
        const int32_t root = (t < 0) ? 0 : (int32_t)(forest_base + (int64_t)t * let_cap);
        walk_quads_f32_from(quads, aux, spos, smass, root, p, valid, [&](float m, float, float, float d2) {
            const float ri = __builtin_amdgcn_rsqf(d2 + eps2);
            sum += (double)(m * ri);
            ++cnt;
        });
    }
    if (valid) {
        const uint32_t slot = perm[s];
        phi[slot] = -G * sum;
        if (counts) counts[slot] = cnt;
    }
}

// ---- reductions -------------------------------------------------------------------------------------------------------
// fold the (s, c) pairs of the workgroup's lanes in a fixed tree; lane 0 holds the result
__device__ __forceinline__ void diag_block_fold(double (&sv)[kDiagQuantities], double (&cv)[kDiagQuantities], double *sh_s,
                                                double *sh_c)
{
#pragma unroll
    for (int q = 0; q < kDiagQuantities; ++q) {
        sh_s[threadIdx.x] = sv[q];
        sh_c[threadIdx.x] = cv[q];
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) {
                double a = sh_s[threadIdx.x], b = sh_c[threadIdx.x];
                neumaier_fold(a, b, sh_s[threadIdx.x + h], sh_c[threadIdx.x + h]);
                sh_s[threadIdx.x] = a;
                sh_c[threadIdx.x] = b;
            }
            __syncthreads();
        }
        sv[q] = sh_s[0];
        cv[q] = sh_c[0];
        __syncthreads();
    }
}

// pass 1: kDiagParts workgroups, body i taken by thread i mod (kDiagParts * kBlock); part[g][q] = {sum, compensation}
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void energy_partial_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                                const Real *__restrict__ mass, const double *__restrict__ phi,
                                                                int64_t n, double *__restrict__ part)
{
    __shared__ double sh_s[kBlock], sh_c[kBlock];
    double sv[kDiagQuantities], cv[kDiagQuantities];
#pragma unroll
    for (int q = 0; q < kDiagQuantities; ++q) { sv[q] = 0.0; cv[q] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)kDiagParts * kBlock) {
        const double m = (double)mass[i];
        const Real2 pp = pos[i], vv = vel[i];
        const double x = (double)pp.x, y = (double)pp.y, vx = (double)vv.x, vy = (double)vv.y;
        const double t[kDiagQuantities] = {m, m * x, m * y, m * vx, m * vy, m * (x * vy - y * vx), m * (vx * vx + vy * vy),
                                           m * phi[i]};
#pragma unroll
        for (int q = 0; q < kDiagQuantities; ++q) neumaier_add(sv[q], cv[q], t[q]);
    }
    diag_block_fold(sv, cv, sh_s, sh_c);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kDiagQuantities; ++q) {
            part[(size_t)blockIdx.x * 2 * kDiagQuantities + 2 * q] = sv[q];
            part[(size_t)blockIdx.x * 2 * kDiagQuantities + 2 * q + 1] = cv[q];
        }
    }
}

// pass 2: one workgroup of kDiagParts threads folds the workgroups' pairs; out[q] = sum + compensation
__global__ __launch_bounds__(kBlock) void energy_final_kernel(const double *__restrict__ part, double *__restrict__ out)
{
    static_assert(kDiagParts == kBlock, "one thread per partial record");
    __shared__ double sh_s[kBlock], sh_c[kBlock];
    double sv[kDiagQuantities], cv[kDiagQuantities];
#pragma unroll
    for (int q = 0; q < kDiagQuantities; ++q) {
        sv[q] = part[(size_t)threadIdx.x * 2 * kDiagQuantities + 2 * q];
        cv[q] = part[(size_t)threadIdx.x * 2 * kDiagQuantities + 2 * q + 1];
    }
    diag_block_fold(sv, cv, sh_s, sh_c);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kDiagQuantities; ++q) out[q] = sv[q] + cv[q];
    }
}

}  // namespace bh
