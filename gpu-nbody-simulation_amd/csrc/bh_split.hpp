// bh_split.hpp -- the kick and the drift as operators of their own (bh_kick, bh_drift), and the time-step criterion
// (bh_timestep).  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: a multiply-add below is fused
// exactly where it is written as fma(), and nowhere else.
//
// The walk epilogues fuse `v += a dt; p += v dt` (updateAccVelPos, project.cu:819-836) into the walk.  Here the two halves
// run separately on the accelerations the last NON-integrating force walk left in the context's force buffer, which is
// indexed by device slot like pos and vel: one lane per slot, no permutation.  Per precision the arithmetic is the
// epilogue's, operation for operation (tests/split_ref.py on tests/integrator_ref.py):
//   kick   F32        v' = fma32(a, (float)h, v)                    a: the fp32 acc_out value
//          MIXED      v' = fma64((double)a32, h, v)                 the fp64 h, unrounded
//          F64        a = F / m_i (one IEEE division: the buffer holds (G m_i) * sum), v' = fma64(a, h, v)
//          F64_EXACT  a = F / m_i, v' = v + a * h, unfused: updateAccelerations then updateVelocities (project.cu:795-809)
//   drift  F32        p' = fma32(v, (float)h, p)
//          MIXED/F64  p' = fma64(v, h, p)
//          F64_EXACT  p' = p + v * h, unfused (updatePositions, project.cu:811-817)
// In the two fp64 precisions a body of mass exactly 0 gets a = 0 / 0 = NaN, as the reference's updateAccelerations gives it.
//
// bh_timestep: a2_i = ax^2 + ay^2 in fp64 (fp32 accelerations widened first; fp64 precisions: a = F / m_i as above), reduced
// to the largest a2 and the caller index that has it -- the smallest caller index on a tie.  A non-finite a2 counts as
// +inf.  (a2, index) pairs under "larger a2, then smaller index" are totally ordered, so the maximum does not depend on
// the order of the reduction: two calls return the same bits.  Two passes of fixed shape like the energy sums: kTsParts
// workgroups stride over the slots, one workgroup folds their records.
#pragma once

#include "bh_prims.hpp"

namespace bh {

constexpr int kTsParts = 256;          // workgroups of the first pass = lanes of the second

// ---- kick ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kick_f32_kernel(const float2 *__restrict__ acc, float2 *__restrict__ vel, int64_t n, float h)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float2 a = acc[i];
    float2 v = vel[i];
    v.x = fmaf(a.x, h, v.x);
    v.y = fmaf(a.y, h, v.y);
    vel[i] = v;
}

__global__ __launch_bounds__(kBlock) void kick_mixed_kernel(const float2 *__restrict__ acc, double2 *__restrict__ vel, int64_t n, double h)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float2 a = acc[i];
    double2 v = vel[i];
    v.x = fma((double)a.x, h, v.x);
    v.y = fma((double)a.y, h, v.y);
    vel[i] = v;
}

__global__ __launch_bounds__(kBlock) void kick_f64_kernel(const double2 *__restrict__ force, const double *__restrict__ mass,
                                                          double2 *__restrict__ vel, int64_t n, double h)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double2 f = force[i];
    const double m = mass[i];
    const double ax = f.x / m, ay = f.y / m;
    double2 v = vel[i];
    v.x = fma(ax, h, v.x);
    v.y = fma(ay, h, v.y);
    vel[i] = v;
}

// (the unit's -ffp-contract=off keeps product and sum apart, as in the exact walks' epilogue; the pragma says so here too)
__global__ __launch_bounds__(kBlock) void kick_exact_kernel(const double2 *__restrict__ force, const double *__restrict__ mass,
                                                            double2 *__restrict__ vel, int64_t n, double h)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double2 f = force[i];
    const double m = mass[i];
    const double ax = f.x / m, ay = f.y / m;
    double2 v = vel[i];
    v.x += ax * h;
    v.y += ay * h;
    vel[i] = v;
}

// ---- drift --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void drift_f32_kernel(const float2 *__restrict__ vel, float2 *__restrict__ pos, int64_t n, float h)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float2 v = vel[i];
    float2 p = pos[i];
    p.x = fmaf(v.x, h, p.x);
    p.y = fmaf(v.y, h, p.y);
    pos[i] = p;
}

__global__ __launch_bounds__(kBlock) void drift_f64_kernel(const double2 *__restrict__ vel, double2 *__restrict__ pos, int64_t n, double h)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double2 v = vel[i];
    double2 p = pos[i];
    p.x = fma(v.x, h, p.x);
    p.y = fma(v.y, h, p.y);
    pos[i] = p;
}

__global__ __launch_bounds__(kBlock) void drift_exact_kernel(const double2 *__restrict__ vel, double2 *__restrict__ pos, int64_t n, double h)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double2 v = vel[i];
    double2 p = pos[i];
    p.x += v.x * h;
    p.y += v.y * h;
    pos[i] = p;
}

// ---- the time-step criterion ----------------------------------------------------------------------------------------
struct TsRecord {
    double a2;             // -1: no body
    int64_t index;         // caller index
};

// keep the larger a2; on a tie the smaller caller index
__device__ __forceinline__ void ts_take(double &a2, int64_t &index, double b2, int64_t bindex)
{
    if (b2 > a2 || (b2 == a2 && bindex < index)) { a2 = b2; index = bindex; }
}

// lane 0 ends up with the workgroup's record
__device__ __forceinline__ void ts_block_fold(double &a2, int64_t &index, double *sh_a, int64_t *sh_i)
{
    sh_a[threadIdx.x] = a2;
    sh_i[threadIdx.x] = index;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            double a = sh_a[threadIdx.x];
            int64_t k = sh_i[threadIdx.x];
            ts_take(a, k, sh_a[threadIdx.x + h], sh_i[threadIdx.x + h]);
            sh_a[threadIdx.x] = a;
            sh_i[threadIdx.x] = k;
        }
        __syncthreads();
    }
    a2 = sh_a[0];
    index = sh_i[0];
}

// pass 1.  Acc2 = float2: `acc` holds accelerations (mass unused); double2: forces, divided by the body's mass.
// orig: slot -> caller index, nullptr when the slots are the caller's indices.
template <typename Acc2>
__global__ __launch_bounds__(kBlock) void timestep_partial_kernel(const Acc2 *__restrict__ acc, const double *__restrict__ mass,
                                                                  const uint32_t *__restrict__ orig, int64_t n, TsRecord *__restrict__ part)
{
    __shared__ double sh_a[kBlock];
    __shared__ int64_t sh_i[kBlock];
    double best = -1.0;
    int64_t best_i = INT64_MAX;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)kTsParts * kBlock) {
        const Acc2 f = acc[i];
        double ax = (double)f.x, ay = (double)f.y;
        if constexpr (sizeof(f.x) == sizeof(double)) {
            const double m = mass[i];
            ax = ax / m;
            ay = ay / m;
        }
        double a2 = ax * ax + ay * ay;
        if (!(a2 < (double)INFINITY)) a2 = (double)INFINITY;      // inf and NaN alike
        ts_take(best, best_i, a2, orig ? (int64_t)orig[i] : i);
    }
    ts_block_fold(best, best_i, sh_a, sh_i);
    if (threadIdx.x == 0) part[blockIdx.x] = TsRecord{best, best_i};
}

// pass 2: one workgroup, one lane per record of pass 1
__global__ __launch_bounds__(kBlock) void timestep_final_kernel(const TsRecord *__restrict__ part, TsRecord *__restrict__ out)
{
    static_assert(kTsParts == kBlock, "one thread per partial record");
    __shared__ double sh_a[kBlock];
    __shared__ int64_t sh_i[kBlock];
    const TsRecord r = part[threadIdx.x];
    double best = r.a2;
    int64_t best_i = r.index;
    ts_block_fold(best, best_i, sh_a, sh_i);
    if (threadIdx.x == 0) out[0] = TsRecord{best, best_i};
}

}  // namespace bh
