// bh_modes.hpp -- azimuthal Fourier modes per radial bin about a centre (bh_azimuthal_modes, bh_modes_max, bh_modes_deposit):
// A_k(bin) = sum m exp(i k phi), k = 0 .. M, and with rates D_k(bin) = sum m w exp(i k phi), w the body's angular velocity --
// bar strength, phase and pattern speed of a disc.  The reference has no such output.
// Included by bh_engine.hip, so it is compiled with -ffp-contract=off: nothing below is fused.
//
// Per body, in fp64 in exactly this order (an fp32 state is widened first, which is exact), with the centre (cx, cy) and the
// centre velocity (ucx, ucy):
//   dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy
//   r2 >= 2^-1022:  r = sqrt(r2);  c1 = dx / r;  s1 = dy / r          r2 < 2^-1022 (no direction): c1 = s1 = 0, w = 0
//   c_0 = 1;  s_0 = 0;  k = 1 .. M:  c_k = c_{k-1} * c1 - s_{k-1} * s1;  s_k = s_{k-1} * c1 + c_{k-1} * s1
//   rates:  ux = vx - ucx;  uy = vy - ucy;  b = dx * uy - dy * ux;  w = b / r2;  mw = m * w
// (c1 = s1 = 0 makes every c_k, s_k with k >= 1 a zero, as the contract asks of a body without a direction.)  The recurrence is
// the definition of cos k phi and sin k phi here: no trigonometric function, so a numpy twin gives the same bits.
// Planes, P = (RATES ? 2 : 1) (1 + 2 M) + 1 of them over the radial slots (radial_slot on r2):
//   A: m c_0, then m c_k, m s_k for k = 1 .. M;   D (rates): mw c_0, then mw c_k, mw s_k;   last: the body count.
// Fixed point of the moment maps with TWO exponents: eA from maxA = max |m c_k|, |m s_k| over all bodies and k, eD from maxD, the
// same with mw; a contribution is (int64) rint(ldexp(q, e)), zero contributions are skipped.
//
// Launch shape of the radial kernels: persistent workgroups that stride over the bodies, a workgroup-private histogram in
// dynamic LDS (SlotHist, bh_binned.hpp: 64-bit LDS atomics), every non-zero word flushed once.  The harmonic loop is a run-time loop and every k's
// contributions are deposited as they are produced: the registers do not grow with M.  All memory traffic is ordinary vector
// loads, stores and atomics; no workgroup waits for another.
#pragma once

#include "bh_radial.hpp"

namespace bh {

constexpr int kModMaxM = 16;                   // = BH_MODES_MAX_M
constexpr int kModMaxBins = kRadMaxBins;       // = BH_MODES_MAX_BINS
constexpr int kModMaxPlanes = 2 * (1 + 2 * kModMaxM) + 1;

struct ModMax {
    unsigned long long bits[2];                // bit patterns of maxA, maxD
    unsigned long long bad;                    // != 0: a non-finite position, velocity (rates), mass, r2 or contribution
};

// what the harmonic loop starts from: returns whether every input is finite (the contributions are the caller's to test)
template <bool RATES, typename Real2, typename Real>
__device__ __forceinline__ bool modes_body(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel, const Real *__restrict__ mass,
                                           int64_t i, const RadCentre &c, double &r2, double &c1, double &s1, double &m, double &mw)
{
    const Real2 pp = pos[i];
    m = (double)mass[i];
    const double dx = (double)pp.x - c.cx, dy = (double)pp.y - c.cy;
    r2 = dx * dx + dy * dy;
    bool ok = map_finite((double)pp.x) && map_finite((double)pp.y) && map_finite(m);
    const bool dir = r2 >= kRadMinR2;
    c1 = 0.0; s1 = 0.0; mw = 0.0;
    if (dir) {
        const double r = sqrt(r2);
        c1 = dx / r;
        s1 = dy / r;
    }
    if constexpr (RATES) {
        const Real2 vv = vel[i];
        ok = ok && map_finite((double)vv.x) && map_finite((double)vv.y);
        const double ux = (double)vv.x - c.ux, uy = (double)vv.y - c.uy;
        const double b = dx * uy - dy * ux;
        const double w = dir ? b / r2 : 0.0;
        mw = m * w;
    }
    return ok;
}

// pass 1: out must be zeroed.  A thread folds its trips into {maxA, maxD}, fold_maxima (bh_binned.hpp) the workgroup.
template <bool RATES, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void modes_max_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                           const Real *__restrict__ mass, int64_t n, RadCentre ctr, int M,
                                                           ModMax *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double a[2] = {0.0, 0.0};                  // maxA, maxD
    int flag = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, c1, s1, m, mw;
        bool bad = !modes_body<RATES>(pos, vel, mass, i, ctr, r2, c1, s1, m, mw) || !map_finite(r2) || !map_finite(mw);
        double ba = fabs(m), bd = fabs(mw);    // (k = 0: c_0 = 1)
        double c = 1.0, s = 0.0;
        for (int k = 1; k <= M; ++k) {
            const double cn = c * c1 - s * s1, sn = s * c1 + c * s1;
            c = cn; s = sn;
            const double qc = m * c, qs = m * s;
            bad |= !map_finite(qc) || !map_finite(qs);
            ba = fmax(ba, fmax(fabs(qc), fabs(qs)));
            if constexpr (RATES) {
                const double rc = mw * c, rs = mw * s;
                bad |= !map_finite(rc) || !map_finite(rs);
                bd = fmax(bd, fmax(fabs(rc), fabs(rs)));
            }
        }
        if (!bad) { if (ba > a[0]) a[0] = ba; if (bd > a[1]) a[1] = bd; }
        flag |= bad ? 1 : 0;
    }
    if (fold_maxima(a, flag, out) & 1) atomicOr(&out->bad, 1ull);
}

// pass 2: planes[p][slot] += contribution, planes[P - 1][slot] += 1, S = nb + 2 slots per plane, through a SlotHist
// (bh_binned.hpp) of P planes in dynamic LDS: tile == 0, its private form, or a tile of `tile` slots -- the host's modes_plan
// decides, and sizes the LDS.  No static LDS at all.
template <bool RATES, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void modes_deposit_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                               const Real *__restrict__ mass, int64_t n, RadCentre ctr,
                                                               const double *__restrict__ e2_mem, int nb, int M, int tile, int eA, int eD,
                                                               long long *__restrict__ planes)
{
    extern __shared__ unsigned long long mod_lds[];
    const int nA = 1 + 2 * M;
    const int P = (RATES ? 2 : 1) * nA + 1;
    const SlotHist h = slot_hist(mod_lds, P, nb, tile, e2_mem, planes, pos, n, ctr);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double r2, c1, s1, m, mw;
        modes_body<RATES>(pos, vel, mass, i, ctr, r2, c1, s1, m, mw);
        const int slot = radial_slot(h.e2, nb, r2);
        h.put(0, slot, (long long)rint(ldexp(m, eA)));
        if constexpr (RATES) h.put(nA, slot, (long long)rint(ldexp(mw, eD)));
        double c = 1.0, s = 0.0;
        for (int k = 1; k <= M; ++k) {
            const double cn = c * c1 - s * s1, sn = s * c1 + c * s1;
            c = cn; s = sn;
            h.put(2 * k - 1, slot, (long long)rint(ldexp(m * c, eA)));
            h.put(2 * k, slot, (long long)rint(ldexp(m * s, eA)));
            if constexpr (RATES) {
                h.put(nA + 2 * k - 1, slot, (long long)rint(ldexp(mw * c, eD)));
                h.put(nA + 2 * k, slot, (long long)rint(ldexp(mw * s, eD)));
            }
        }
        h.put(P - 1, slot, 1ll);
    }
    h.flush();
}
}  // namespace bh
