// bh_radial.hpp -- radial profiles and Lagrangian radii about a centre (bh_radial_profile, bh_radial_max, bh_radial_deposit,
// bh_lagrangian_radii, bh_radial_select): the radial counterpart of the moment maps.  The reference has no such output.
// Included by bh_engine.hip, so it is compiled with -ffp-contract=off: nothing below is fused.
//
// Per body, in fp64 in exactly this order (an fp32 state is widened first, which is exact), with the centre (cx, cy) and the
// centre velocity (ucx, ucy):
//   dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy
//   ux = vx - ucx;  uy = vy - ucy;  a = dx * ux + dy * uy;  b = dx * uy - dy * ux
//   r2 >= 2^-1022:  r = sqrt(r2);  vr = a / r;  vt = b / r          r2 < 2^-1022 (zero or subnormal): vr = vt = 0
//   q0 = m   q1 = m * vr   q2 = m * vt   q3 = m * (vr * vr)   q4 = m * (vt * vt)
// Slots: nb + 2 of them, decided on r2 against the squared edges e2[0 .. nb] alone: slot = the number of edges with
// e2[k] <= r2 (0: inside edges[0]; nb + 1: at or beyond edges[nb]; a body on an edge belongs to the bin above it).
// Planes 0-4 are the sums of q0-q4 in the fixed point of the moment maps (bh_moments.hpp: max |q_p| over the whole system,
// exponent 62 - E_p - L, (int64) rint(ldexp(q_p, exponent)), 64-bit integer atomics); plane 5 is the body count.
//
// Lagrangian radii: w_i = rint(ldexp(m_i, e0)).  The radius of a mass fraction is found by a radix select over the bit pattern
// of r2 (non-negative doubles order like their patterns; r2 is never -0): 8 rounds of 8 bits from the top, each one pass over
// the bodies that returns, for up to 32 prefixes (the digits already decided), 256 x {sum w, count}.  No sort, no gather, and
// every number that decides anything is an integer sum: the same on any launch shape, body order or number of ranks.
//
// Launch shape: a fixed grid of persistent workgroups that stride over the bodies; the deposit (SlotHist, bh_binned.hpp) and the
// select keep a workgroup-private histogram in LDS (64-bit LDS atomics) and flush every non-zero entry to memory once.  All memory traffic is
// ordinary vector loads, stores and atomics.
#pragma once

#include "bh_moments.hpp"

namespace bh {

constexpr int kRadPlanes = 5;                  // fixed-point planes; plane kRadPlanes is the count
constexpr int kRadMaxBins = 4096;              // = BH_RADIAL_MAX_BINS
constexpr int kRadMaxFractions = 32;           // = BH_RADIAL_MAX_FRACTIONS
constexpr int kRadDigitBits = 8;               // = BH_RADIAL_DIGIT_BITS
constexpr int kRadDigits = 1 << kRadDigitBits;
constexpr int kRadRounds = 64 / kRadDigitBits;
constexpr int kRadLdsSlots = 1024;             // slots of the LDS histogram: 6 planes x 1,024 x 8 B = 48 KiB
constexpr int kRadSelChunk = 8;                // prefixes of one select launch: 8 x 256 x {sum w, count} x 8 B = 32 KiB
constexpr double kRadMinR2 = 2.2250738585072014e-308;      // 2^-1022: below it r2 gives no direction

struct RadMax {
    unsigned long long bits[kRadPlanes];       // bit patterns of max |q_p|
    unsigned long long bad;                    // != 0: a non-finite position, velocity, mass, r2 or moment
    unsigned long long negative;               // != 0: a mass < 0
};
struct RadExp { int32_t e[kRadPlanes]; };

// VEL = false (the Lagrangian radii): the velocities are not read, q1 .. q4 are 0.  Returns whether every input is finite.
template <bool VEL, typename Real2, typename Real>
__device__ __forceinline__ bool radial_body(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel, const Real *__restrict__ mass,
                                            int64_t i, const RadCentre &c, double &r2, double (&q)[kRadPlanes])
{
    const Real2 pp = pos[i];
    const double m = (double)mass[i];
    const double dx = (double)pp.x - c.cx, dy = (double)pp.y - c.cy;
    r2 = dx * dx + dy * dy;
    bool ok = map_finite((double)pp.x) && map_finite((double)pp.y) && map_finite(m);
    double vr = 0.0, vt = 0.0;
    if constexpr (VEL) {
        const Real2 vv = vel[i];
        ok = ok && map_finite((double)vv.x) && map_finite((double)vv.y);
        const double ux = (double)vv.x - c.ux, uy = (double)vv.y - c.uy;
        const double a = dx * ux + dy * uy, b = dx * uy - dy * ux;
        if (r2 >= kRadMinR2) {
            const double r = sqrt(r2);
            vr = a / r;
            vt = b / r;
        }
    }
    q[0] = m;
    q[1] = m * vr;
    q[2] = m * vt;
    q[3] = m * (vr * vr);
    q[4] = m * (vt * vt);
    return ok;
}

// pass 1: out must be zeroed.  gridDim.x workgroups stride over the bodies (the one atomic per plane and workgroup all land on
// one line: at N = 1M, 4,096 workgroups of one trip took 0.247 ms, 512 of eight trips 0.047 ms); a thread folds its trips,
// fold_maxima (bh_binned.hpp) folds the workgroup's threads in LDS and sends one atomic per plane.
template <bool VEL, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void radial_max_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                            const Real *__restrict__ mass, int64_t n, RadCentre ctr,
                                                            RadMax *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double a[kRadPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int flag = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, q[kRadPlanes];
        bool bad = !radial_body<VEL>(pos, vel, mass, i, ctr, r2, q) || !map_finite(r2);
#pragma unroll
        for (int p = 0; p < kRadPlanes; ++p) bad |= !map_finite(q[p]);
#pragma unroll
        for (int p = 0; p < kRadPlanes; ++p)
            if (!bad && fabs(q[p]) > a[p]) a[p] = fabs(q[p]);
        flag |= (bad ? 1 : 0) | (q[0] < 0.0 ? 2 : 0);
    }
    const int f = fold_maxima(a, flag, out);   // bit 0: bad, bit 1: a negative mass
    if (f & 1) atomicOr(&out->bad, 1ull);
    if (f & 2) atomicOr(&out->negative, 1ull);
}

// pass 2: planes[p][slot] += contribution, planes[5][slot] += 1, S = nb + 2 slots per plane.  gridDim.x workgroups stride over
// the bodies into a SlotHist (bh_binned.hpp) of 6 planes in dynamic LDS:
//   PRIVATE  (S <= kRadLdsSlots): its private form, 6 * S words and the nb + 1 squared edges.
//   !PRIVATE: its tiled form with a tile of kRadLdsSlots slots, 6 * kRadLdsSlots words.
// The same integers either way, so the same planes.
template <bool PRIVATE, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void radial_deposit_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                                const Real *__restrict__ mass, int64_t n, RadCentre ctr,
                                                                const double *__restrict__ e2_mem, int nb, RadExp ex,
                                                                long long *__restrict__ planes)
{
    extern __shared__ unsigned long long rad_lds[];
    const SlotHist h = slot_hist(rad_lds, kRadPlanes + 1, nb, PRIVATE ? 0 : kRadLdsSlots, e2_mem, planes, pos, n, ctr);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, q[kRadPlanes];
        radial_body<true>(pos, vel, mass, i, ctr, r2, q);
        const int s = radial_slot(h.e2, nb, r2);
#pragma unroll
        for (int p = 0; p < kRadPlanes; ++p) h.put(p, s, (long long)rint(ldexp(q[p], ex.e[p])));
        h.put(kRadPlanes, s, 1ll);
    }
    h.flush();
}

// One round of the radix select.  key = the bit pattern of r2; a body belongs to prefix k when key >> hi_shift == prefix[k]
// (round 0: hi_shift = 64, every body belongs to the one empty prefix 0); its digit is (key >> lo_shift) & 255;
// hist[k][digit] += {w, 1} with w = rint(ldexp(m, e0)).  A body that is not finite, has a negative mass, or whose |m| exceeds
// m_limit = 2^(62 - L - e0) (its w, or n of them, could leave int64) contributes nothing and raises its bit of *flags.
struct RadSelect {
    double cx, cy, m_limit;
    int32_t e0, hi_shift, lo_shift, np;
    unsigned long long prefix[kRadSelChunk];
};
constexpr unsigned long long kRadFlagBad = 1, kRadFlagNegative = 2, kRadFlagLarge = 4;

template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void radial_select_kernel(const Real2 *__restrict__ pos, const Real *__restrict__ mass, int64_t n,
                                                               RadSelect s, long long *__restrict__ hist,
                                                               unsigned long long *__restrict__ flags)
{
    __shared__ unsigned long long h[kRadSelChunk * kRadDigits * 2];
    const int words = s.np * kRadDigits * 2;
    for (int k = threadIdx.x; k < words; k += kBlock) h[k] = 0ull;
    __syncthreads();
    unsigned long long flag = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const Real2 pp = pos[i];
        const double m = (double)mass[i];
        const double dx = (double)pp.x - s.cx, dy = (double)pp.y - s.cy;
        const double r2 = dx * dx + dy * dy;
        unsigned long long f = 0;
        if (!(map_finite((double)pp.x) && map_finite((double)pp.y) && map_finite(m) && map_finite(r2))) f |= kRadFlagBad;
        else if (m < 0.0) f |= kRadFlagNegative;
        else if (m > s.m_limit) f |= kRadFlagLarge;
        flag |= f;
        if (f) continue;
        const unsigned long long key = (unsigned long long)__double_as_longlong(r2);
        const unsigned long long high = s.hi_shift >= 64 ? 0ull : key >> s.hi_shift;
        int k = -1;
#pragma unroll
        for (int j = 0; j < kRadSelChunk; ++j)
            if (j < s.np && s.prefix[j] == high) k = j;
        if (k < 0) continue;
        const int at = (k * kRadDigits + (int)((key >> s.lo_shift) & (unsigned long long)(kRadDigits - 1))) * 2;
        const long long w = (long long)rint(ldexp(m, s.e0));
        if (w) atomicAdd(&h[at], (unsigned long long)w);
        atomicAdd(&h[at + 1], 1ull);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < words; k += kBlock) {
        const unsigned long long v = h[k];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(hist + k), v);
    }
    if (flag) atomicOr(flags, flag);
}
}  // namespace bh
