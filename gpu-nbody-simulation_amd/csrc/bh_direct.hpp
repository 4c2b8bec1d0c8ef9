// bh_direct.hpp -- exact O(N^2) forces of the current state (bh_direct_forces, and the direct half of bh_force_check).
// Included by bh_engine.hip, so it is compiled with -ffp-contract=off: no multiply-add below is fused.
//
// Contract: for a target body i (a caller index) the force is computeForces of main_approach_1.cpp:53-75, bit for bit:
//   for j = 0 .. n-1 in CALLER order, j != i by index:
//     dx = p[j].x - p[i].x;  d2 = 0.0 + dx*dx;  dy = p[j].y - p[i].y;  d2 += dy*dy;
//     d = sqrt(d2);  k = ((G*m_i)*m_j) / (d2*d);  sx += k*dx;  sy += k*dy
// in fp64 with IEEE sqrt and division (correctly rounded) in every precision.  An fp32 state is widened exactly, so the
// result is the direct sum of the state the device holds.  Coincident bodies give inf / NaN where the reference does.
// Plummer softening (bh_set_softening): s2 = d2 + eps2, d = sqrt(s2), k = ((G*m_i)*m_j) / (s2*d), same order, j == i still
// skipped by index; distinct coincident bodies then give a finite zero force.  d2 >= +0 or NaN here, so d2 + 0.0 is d2 bit
// for bit: the one kernel serves eps2 = 0 as the contract above.
//
// Launch shape: one lane per target, 256-lane workgroups, every target in one launch (n_threads does not apply).  The
// j-bodies go through LDS in tiles of kDirectTile caller indices (x, y, m as fp64: 24 KB); every lane of the workgroup
// then reads the same LDS address, a broadcast.  The j loop is unrolled by four so that the sqrt and division sequences of
// neighbouring j overlap; the two running sums still take their terms strictly in j order.  The last tile is masked by its
// count, never padded (a zero-mass dummy at distance 0 would add 0/0, and even a +0 term can turn a -0 sum into +0).
// fp32 / mixed states live in device (slot) order: the tile loads read body j through slot_of (caller index -> slot),
// which direct_slot_kernel scatters from orig[]; nullptr when the slots are the caller's indices.
#pragma once

#include "bh_prims.hpp"

namespace bh {

constexpr int kDirectTile = 1024;      // j-bodies per LDS tile

// slot_of[orig[s]] = s: the inverse of the slot -> caller index map of a re-ordered state
__global__ __launch_bounds__(kBlock) void direct_slot_kernel(const uint32_t *__restrict__ orig, int64_t n,
                                                             uint32_t *__restrict__ slot_of)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s < n) slot_of[orig[s]] = (uint32_t)s;
}

// out[t] = direct-sum force on body targets[t] (targets == nullptr: body t0 + t), t < n_targets; state pos / mass in slot
// order, slot_of as above (nullptr: identity).  Every lane of a workgroup takes part in the tile loads and barriers.
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void direct_forces_kernel(const Real2 *__restrict__ pos, const Real *__restrict__ mass,
                                                               const uint32_t *__restrict__ slot_of,
                                                               const int64_t *__restrict__ targets, int64_t t0,
                                                               int64_t n_targets, int64_t n, double G, double eps2,
                                                               double2 *__restrict__ out)
{
    __shared__ double2 tp[kDirectTile];
    __shared__ double tm[kDirectTile];
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < n_targets;
    int64_t i = -1;                                     // (lanes past the last target: no body, no skip, no store)
    double xi = 0.0, yi = 0.0, gmi = 0.0;
    if (live) {
        i = targets ? targets[t] : t0 + t;
        const int64_t si = slot_of ? (int64_t)slot_of[i] : i;
        const Real2 p = pos[si];
        xi = (double)p.x; yi = (double)p.y;
        gmi = G * (double)mass[si];                     // G * m_i: the reference's left-to-right product, hoisted
    }
    double sx = 0.0, sy = 0.0;
    for (int64_t j0 = 0; j0 < n; j0 += kDirectTile) {
        const int cnt = (int)std::min<int64_t>(kDirectTile, n - j0);
        __syncthreads();                                // (the previous tile has been read)
        for (int k = threadIdx.x; k < cnt; k += kBlock) {
            const int64_t j = j0 + k;
            const int64_t sj = slot_of ? (int64_t)slot_of[j] : j;
            const Real2 p = pos[sj];
            tp[k] = make_double2((double)p.x, (double)p.y);
            tm[k] = (double)mass[sj];
        }
        __syncthreads();
        const int64_t self = i - j0;                    // the target's own index within this tile (outside: never met)
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const double2 pj = tp[k];
            const double dx = pj.x - xi;
            double d2 = 0.0;
            d2 += dx * dx;
            const double dy = pj.y - yi;
            d2 += dy * dy;
            const double s2 = d2 + eps2;
            const double d = sqrt(s2);
            const double f = (gmi * tm[k]) / (s2 * d);
            if (k != self) {
                sx += f * dx;
                sy += f * dy;
            }
        }
    }
    if (live) out[t] = make_double2(sx, sy);
}

}  // namespace bh
