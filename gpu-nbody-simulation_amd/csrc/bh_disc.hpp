// bh_disc.hpp -- a disc the engine can make and analyse (bh_initialize_disc, bh_rotation_curve, bh_set_disc_velocities): the
// positions of a Kuzmin-Toomre disc, the sums behind the rotation curve of the engine's own forces, and velocities drawn about
// a radial table.  The reference has no such thing.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: nothing
// below is fused.  Nothing below calls libm beyond sqrt, which is correctly rounded: a numpy twin gives the same bits.
//
// 1. disc_init_kernel.  Surface density M a / (2 pi (R^2 + a^2)^(3/2)) cut at r_max; the enclosed mass fraction is
//    1 - a / sqrt(R^2 + a^2), inverted in closed form.  Body i from (seed, i) alone, with F = 1 - a / sqrt(r_max^2 + a^2) from
//    the host (1: no cut):
//      stream 96:       u = u01(w0, w1) * F;  t = u * (2 - u);  R = (a * sqrt(t)) / (1 - u)
//      stream 128 + k:  p = 2 u01(w0, w1) - 1;  q = 2 u01(w2, w3) - 1;  s = p * p + q * q;  taken when 2^-1022 <= s <= 1, else
//                       k + 1, k < 64; the 64th draw stands whatever its s ((1, 0) when its s < 2^-1022)
//      c = p / sqrt(s);  z = q / sqrt(s);  x = R * c;  y = R * z  (rounded to the state type), v = 0, every mass the same.
//
// 2. curve_max_kernel, curve_deposit_kernel.  Per body, in fp64 in exactly this order (an fp32 value is widened first), with the
//    centre (cx, cy) and the force buffer, which holds accelerations (fp32 / mixed) or forces (fp64 tree):
//      dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy;  r = sqrt(r2)
//      (ax, ay) = the acceleration, or (Fx / m, Fy / m): what bh_get_accel returns
//      q0 = m   q1 = m * r   q2 = m * (dx * ax + dy * ay)   q3 = m * (dx * ay - dy * ax)
//    Slots by radial_slot on r2, nb + 2 of them, nb <= 1022: planes 0-3 are the sums of q0-q3 in the fixed point of the moment
//    maps, one exponent each from the system-wide maxima; plane 4 is the body count.  The histogram (SlotHist, bh_binned.hpp)
//    is always workgroup-private in LDS (5 x (nb + 2) words and the nb + 1 squared edges): one code path.
//
// 3. disc_velocities_kernel.  k <= 1024 strictly ascending radii Rn with their squares, three tables vt, sr, st.  Per slot, with
//    the caller index i of the slot (through orig where the state has been re-ordered):
//      dx, dy, r2 as above;  r2 < 2^-1022:  v = (ucx, ucy)
//      r = sqrt(r2);  j = the number of squared radii <= r2
//      j = 0: f = y[0];  j = k: f = y[k - 1];  else t = (r - Rn[j-1]) / (Rn[j] - Rn[j-1]);  f = y[j-1] + t * (y[j] - y[j-1])
//      g1 = ((int64) sum of the 12 words of streams 192 .. 194  -  6 (2^32 - 1)) * 2^-32;  g2 likewise from 195 .. 197
//      vr = sr * g1;  vtt = vt + st * g2
//      vx = ucx + (vr * dx - vtt * dy) / r;  vy = ucy + (vr * dy + vtt * dx) / r   (rounded to the state type)
//    g is an Irwin-Hall deviate: mean 0 exactly, variance 1 - 2^-64, |g| <= 6, exact in fp64 -- no log, no cos.
//
// Launch shape of the radial kernels for 2 and 3: persistent workgroups that stride over the bodies.  All memory traffic is
// ordinary vector loads, stores and atomics; no workgroup waits for another.
#pragma once

#include "bh_init.hpp"
#include "bh_radial.hpp"

namespace bh {

constexpr int kDiscPlanes = 4;                 // fixed-point planes; plane kDiscPlanes is the count
constexpr int kDiscMaxBins = 1022;             // = BH_DISC_MAX_BINS: nb + 2 slots fit the LDS histogram
constexpr int kDiscLdsSlots = 1024;
constexpr int kDiscMaxTable = 1024;            // = BH_DISC_MAX_TABLE
constexpr int kDiscTables = 5;                 // Rn^2, Rn, vt, sr, st: k doubles each, in this order
constexpr uint32_t kDiscRadiusStream = 96, kDiscDirStream0 = 128, kDiscDirTries = 64, kDiscG1Stream0 = 192, kDiscG2Stream0 = 195;

struct DiscMax {
    unsigned long long bits[kDiscPlanes];      // bit patterns of max |q_p|
    unsigned long long bad;                    // != 0: a non-finite position, mass, acceleration, r2 or contribution
};
struct DiscExp { int32_t e[kDiscPlanes]; };

template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void disc_init_kernel(Real2 *__restrict__ pos, Real2 *__restrict__ vel, Real *__restrict__ mass,
                                                           int64_t n, uint64_t seed, double a, double F, double m)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4];
    Philox::draw(seed, (uint64_t)i, kDiscRadiusStream, w);
    const double u = u01(w[0], w[1]) * F;
    const double t = u * (2.0 - u);
    const double R = (a * sqrt(t)) / (1.0 - u);
    double p = 0.0, q = 0.0, s = 0.0;
    for (uint32_t k = 0; k < kDiscDirTries; ++k) {
        Philox::draw(seed, (uint64_t)i, kDiscDirStream0 + k, w);
        p = 2.0 * u01(w[0], w[1]) - 1.0;
        q = 2.0 * u01(w[2], w[3]) - 1.0;
        s = p * p + q * q;
        if (s >= kRadMinR2 && s <= 1.0) break;
    }
    double c = 1.0, z = 0.0;
    if (s >= kRadMinR2) {
        const double rs = sqrt(s);
        c = p / rs;
        z = q / rs;
    }
    pos[i] = Real2{(Real)(R * c), (Real)(R * z)};
    vel[i] = Real2{(Real)0, (Real)0};
    mass[i] = (Real)m;
}

// Acc2 = float2: the buffer holds accelerations; double2: forces, divided by the mass.  Returns whether every input is finite.
template <typename Real2, typename Real, typename Acc2>
__device__ __forceinline__ bool curve_body(const Real2 *__restrict__ pos, const Real *__restrict__ mass, const Acc2 *__restrict__ force,
                                           int64_t i, const RadCentre &c, double &r2, double (&q)[kDiscPlanes])
{
    const Real2 pp = pos[i];
    const Acc2 ff = force[i];
    const double m = (double)mass[i];
    const double dx = (double)pp.x - c.cx, dy = (double)pp.y - c.cy;
    r2 = dx * dx + dy * dy;
    const double r = sqrt(r2);
    double ax = (double)ff.x, ay = (double)ff.y;
    if constexpr (sizeof(ff.x) == sizeof(double)) { ax = ax / m; ay = ay / m; }
    q[0] = m;
    q[1] = m * r;
    q[2] = m * (dx * ax + dy * ay);
    q[3] = m * (dx * ay - dy * ax);
    return map_finite((double)pp.x) && map_finite((double)pp.y) && map_finite(m) && map_finite(ax) && map_finite(ay);
}

// pass 1: out must be zeroed.  A thread folds its trips, fold_maxima (bh_binned.hpp) the workgroup.
template <typename Real2, typename Real, typename Acc2>
__global__ __launch_bounds__(kBlock) void curve_max_kernel(const Real2 *__restrict__ pos, const Real *__restrict__ mass,
                                                           const Acc2 *__restrict__ force, int64_t n, RadCentre ctr,
                                                           DiscMax *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double a[kDiscPlanes] = {0.0, 0.0, 0.0, 0.0};
    int flag = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, q[kDiscPlanes];
        bool bad = !curve_body(pos, mass, force, i, ctr, r2, q) || !map_finite(r2);
#pragma unroll
        for (int p = 0; p < kDiscPlanes; ++p) bad |= !map_finite(q[p]);
#pragma unroll
        for (int p = 0; p < kDiscPlanes; ++p)
            if (!bad && fabs(q[p]) > a[p]) a[p] = fabs(q[p]);
        flag |= bad ? 1 : 0;
    }
    if (fold_maxima(a, flag, out) & 1) atomicOr(&out->bad, 1ull);
}

// pass 2: planes[p][slot] += contribution, planes[4][slot] += 1, S = nb + 2 <= kDiscLdsSlots slots per plane, through a
// SlotHist (bh_binned.hpp) in its private form alone (tile 0, a constant): 5 * S words of dynamic LDS and the nb + 1 squared edges.
template <typename Real2, typename Real, typename Acc2>
__global__ __launch_bounds__(kBlock) void curve_deposit_kernel(const Real2 *__restrict__ pos, const Real *__restrict__ mass,
                                                               const Acc2 *__restrict__ force, int64_t n, RadCentre ctr,
                                                               const double *__restrict__ e2_mem, int nb, DiscExp ex,
                                                               long long *__restrict__ planes)
{
    extern __shared__ unsigned long long disc_lds[];
    const SlotHist h = slot_hist(disc_lds, kDiscPlanes + 1, nb, 0, e2_mem, planes, pos, n, ctr);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, q[kDiscPlanes];
        curve_body(pos, mass, force, i, ctr, r2, q);
        const int s = radial_slot(h.e2, nb, r2);
#pragma unroll
        for (int p = 0; p < kDiscPlanes; ++p) h.put(p, s, (long long)rint(ldexp(q[p], ex.e[p])));
        h.put(kDiscPlanes, s, 1ll);
    }
    h.flush();
}

// the sum of the twelve words of three streams, centred and scaled: exact in fp64
__device__ __forceinline__ double disc_deviate(uint64_t seed, uint64_t index, uint32_t stream0)
{
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        uint32_t w[4];
        Philox::draw(seed, index, stream0 + k, w);
        sum += (uint64_t)w[0] + (uint64_t)w[1] + (uint64_t)w[2] + (uint64_t)w[3];
    }
    return (double)((int64_t)sum - (int64_t)6 * (int64_t)0xFFFFFFFFll) * (1.0 / 4294967296.0);
}

__device__ __forceinline__ double disc_table(const double *__restrict__ y, int j, int k, double t)
{
    if (j == 0) return y[0];
    if (j == k) return y[k - 1];
    return y[j - 1] + t * (y[j] - y[j - 1]);
}

// tables: kDiscTables x k doubles (Rn^2, Rn, vt, sr, st), copied to dynamic LDS of the same size.  orig: null where a slot is the
// caller index.  Only vel is written.
template <typename Real2>
__global__ __launch_bounds__(kBlock) void disc_velocities_kernel(const Real2 *__restrict__ pos, Real2 *__restrict__ vel,
                                                                 const uint32_t *__restrict__ orig, int64_t n, RadCentre ctr,
                                                                 uint64_t seed, const double *__restrict__ tables, int k)
{
    extern __shared__ double disc_tab[];
    for (int t = threadIdx.x; t < kDiscTables * k; t += kBlock) disc_tab[t] = tables[t];
    __syncthreads();
    const double *R2 = disc_tab, *Rn = disc_tab + k, *vt = disc_tab + 2 * k, *sr = disc_tab + 3 * k, *st = disc_tab + 4 * k;
    using Real = decltype(Real2{}.x);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const Real2 pp = pos[i];
        const double dx = (double)pp.x - ctr.cx, dy = (double)pp.y - ctr.cy;
        const double r2 = dx * dx + dy * dy;
        if (r2 < kRadMinR2) { vel[i] = Real2{(Real)ctr.ux, (Real)ctr.uy}; continue; }
        const double r = sqrt(r2);
        const int j = radial_slot(R2, k - 1, r2);
        const double t = (j > 0 && j < k) ? (r - Rn[j - 1]) / (Rn[j] - Rn[j - 1]) : 0.0;
        const uint64_t index = orig ? (uint64_t)orig[i] : (uint64_t)i;
        const double g1 = disc_deviate(seed, index, kDiscG1Stream0), g2 = disc_deviate(seed, index, kDiscG2Stream0);
        const double vr = disc_table(sr, j, k, t) * g1;
        const double vtt = disc_table(vt, j, k, t) + disc_table(st, j, k, t) * g2;
        const double vx = ctr.ux + (vr * dx - vtt * dy) / r, vy = ctr.uy + (vr * dy + vtt * dx) / r;
        vel[i] = Real2{(Real)vx, (Real)vy};
    }
}
}  // namespace bh
