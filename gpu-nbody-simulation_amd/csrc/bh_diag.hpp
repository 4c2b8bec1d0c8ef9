// bh_diag.hpp -- on-device diagnostics: the potential walk and the energy / momentum reductions (bh_compute_potential,
// bh_energy).  The reference has no potential or energy at all: its only outputs are positions, forces and the quadtree
// files.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: every fused multiply-add below is written out.
//
// Potential walk.  phi_i = -G sum_j M_j / d_ij over EXACTLY the terms the precision's force walk takes for body i
// (project.cu:617-658): the same empty-node cut-off, the same acceptance decisions, the same self skip, the same depth-cap
// aggregates and fp32 bucket leaves.  The acceptance is read from the node data the force walks compare against -- the d2
// thresholds (or sizes) in the NodeD `size` slot, QuadF.thr -- with the force walks' own d2 expression for the mode, so the
// decisions are the force walk's bit for bit (the tests compare per-body term counts).  Launch shape: the one the fp32 and
// fp64 throughput walks were measured best with -- one wavefront per 64 consecutive bodies of the sorted order, the nodes
// read with scalar loads (wave-uniform addresses in the constant address space), a four-sibling quad per load, the
// traversal stack in three VGPRs addressed by lane (entry k in lane k & 63 of the first or second triple: 128 entries;
// depth-first pushing every opened child needs at most 3 * max_depth + 4).  Every body is walked in one launch.
//   fp64 modes: d2 as the force walk forms it, d = sqrt(d2) + 1e-15 (project.cu:630-634), term M / d -- IEEE sqrt and
//               division, correctly rounded -- summed per lane with Neumaier compensation, times -G at the end.
//   F32 / MIXED: the fp32 walk's d2 = fmaf(dx, dx, dy * dy) from the fp32 sorted positions, its 1/d = v_rsq_f32(d2), the
//               fp32 term M / d, accumulated in fp64.
//
// Reductions.  One fp64 term per body for each of: m, m x, m y, m vx, m vy, m (x vy - y vx), m |v|^2, m phi.  kDiagParts
// workgroups take fixed grid-strided bodies, each lane keeps a Neumaier (sum, compensation) pair per quantity, and the
// pairs are folded in a fixed tree inside the workgroup and then, in a second one-workgroup launch, over the workgroups:
// the same state gives the same bits every call.  Eight doubles reach the host.
#pragma once

#include "bh_tree.hpp"
#include "bh_walk_f64.hpp"

namespace bh {

constexpr int kDiagParts = 256;        // workgroups of the first reduction pass (= threads of the second)
constexpr int kDiagQuantities = 8;     // m, mx, my, mvx, mvy, Lz, m|v|^2, m phi

// acceptance of a subdivided fp64 cell, as the force walk of the mode states it
enum DiagAccept : int {
    kAcceptThr = 0,        // BH_PRECISION_F64: thr < d2, d2 = fma(dx, dx, dy * dy) (walk_f64_kernel)
    kAcceptExactThr = 1,   // BH_PRECISION_F64_EXACT: d2 >= thr, d2 = dx * dx + dy * dy (walk_exact_kernel, THR)
    kAcceptSize = 2        // BH_PRECISION_F64_EXACT + BH_FLAG_WALK_PORTABLE: size / d < theta (walk_exact_kernel, !THR)
};

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

// register-lane traversal stack, 128 entries of {node or quad index, lane mask}: wave-uniform pointer sp
struct DiagStack {
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

// ---- fp64 tree (BH_PRECISION_F64_EXACT, BH_PRECISION_F64): one wavefront per 64 sorted bodies ---------------------
// phi / counts are written at the body's caller index (the state order of these modes).
template <bool COMPAT, int ACCEPT>
__global__ __launch_bounds__(kBlock) void potential_f64_kernel(const NodeD *__restrict__ gd, const LinkD *__restrict__ ld,
                                                               const uint32_t *__restrict__ perm, const double2 *__restrict__ pos,
                                                               int64_t n, double theta, double G, const TreeCounters *ctr,
                                                               double *__restrict__ phi, uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n;
    const int64_t body = valid ? (int64_t)perm[s] : -1;
    const double2 p = valid ? pos[body] : double2{0.0, 0.0};
    const int32_t body32 = (int32_t)body, alt32 = -2 - body32;     // occ == i, occ + 2 == -i (project.cu:646)
    double sum = 0.0, comp = 0.0;
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
        LinkD k;
        k.child = cl[node].child; k.occ = cl[node].occ;
        if (q.m <= 1e-15) return;                                  // project.cu:617
        const double dx = q.cx - p.x, dy = q.cy - p.y;
        const double d2 = (ACCEPT == kAcceptThr) ? fma(dx, dx, dy * dy) : dx * dx + dy * dy;
        const double d = sqrt(d2) + 1e-15;                         // project.cu:634
        const bool leaf = k.child < 0;
        bool take;
        if (leaf) take = !(k.occ == body32 || (COMPAT && k.occ == alt32));   // project.cu:623-626, 646
        else if (ACCEPT == kAcceptThr) take = q.size < d2;
        else if (ACCEPT == kAcceptExactThr) take = d2 >= q.size;
        else take = q.size / d < theta;                            // project.cu:643
        const bool mine = (mask >> lane) & 1ull;
        if (mine && take) { neumaier_add(sum, comp, q.m / d); ++cnt; }
        if (!leaf) {
            const uint64_t open = mask & __ballot(!take);
            if (open != 0) st.push(k.child, open);
        }
    };

    eval(0, __ballot(valid));                                 // the root alone, then quads of four siblings
    while (st.sp > 0) {
        int32_t base;
        uint64_t mask;
        st.pop(base, mask);
#pragma unroll
        for (int k = 0; k < 4; ++k) eval(base + k, mask);
    }
    if (valid) {
        phi[body] = -G * (sum + comp);
        if (counts) counts[body] = cnt;
    }
}

// ---- QuadF tree (BH_PRECISION_F32, BH_PRECISION_MIXED): the fp32 walk's terms (walk_fast_kernel's eval and bucket) --
// phi / counts are written at the body's device slot perm[s] (the state order of these modes).
__global__ __launch_bounds__(kBlock) void potential_f32_kernel(const QuadF *__restrict__ quads, const NodeAux *__restrict__ aux,
                                                               const float2 *__restrict__ spos, const float *__restrict__ smass,
                                                               const uint32_t *__restrict__ perm, int64_t n, double G,
                                                               const TreeCounters *ctr, double *__restrict__ phi,
                                                               uint32_t *__restrict__ counts)
{
    if (ctr->overflow) return;
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < n;
    const float2 p = valid ? spos[s] : float2{0.f, 0.f};
    double sum = 0.0;
    uint32_t cnt = 0;
    DiagStack st;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const QuadF BH64_CONSTANT *cq = (const QuadF BH64_CONSTANT *)quads;
    const NodeAux BH64_CONSTANT *ca = (const NodeAux BH64_CONSTANT *)aux;
    const float2 BH64_CONSTANT *cpos = (const float2 BH64_CONSTANT *)spos;
    const float BH64_CONSTANT *cmass = (const float BH64_CONSTANT *)smass;
#pragma clang diagnostic pop

    // one node: empty (m == 0) skipped; accepted iff d2 > thr (leaf: thr = 0, the self skip; bucket: +inf, opened by all)
    auto eval = [&](const float cx, const float cy, const float m, const float thr, const int32_t child, const uint64_t mask) {
        if (__float_as_int(m) == 0) return;
        const float dx = cx - p.x, dy = cy - p.y;
        const float d2 = __builtin_fmaf(dx, dx, dy * dy);
        const uint64_t farm = __ballot(d2 > thr);
        if ((mask & farm) >> lane & 1ull) {
            const float ri = __builtin_amdgcn_rsqf(d2);
            sum += (double)(m * ri);
            ++cnt;
        }
        if (child != -1) {                                         // subdivided cell (> 0) or bucket reference (<= -2)
            const uint64_t open = mask & ~farm;
            if (open != 0) st.push(child, open);
        }
    };
    // a depth-cap cell of several bodies (compat off), body by body; self and coincident bodies contribute nothing
    auto bucket = [&](const int32_t node, const uint64_t mask) {
        const int32_t first = ca[node].first, count = ca[node].count;
        for (int32_t j = first; j < first + count; ++j) {
            const float2 o = float2{cpos[j].x, cpos[j].y};
            const float om = cmass[j];
            const float dx = o.x - p.x, dy = o.y - p.y;
            const float d2 = __builtin_fmaf(dx, dx, dy * dy);
            if ((mask & __ballot(d2 > 0.f)) >> lane & 1ull) {
                const float ri = __builtin_amdgcn_rsqf(d2);
                sum += (double)(om * ri);
                ++cnt;
            }
        }
    };
    auto eval_quad = [&](const int32_t q, const uint64_t mask) {
#pragma unroll
        for (int k = 0; k < 4; ++k) eval(cq[q].xy[2 * k], cq[q].xy[2 * k + 1], cq[q].m[k], cq[q].thr[k], cq[q].child[k], mask);
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
