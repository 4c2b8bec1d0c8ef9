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
// dynamic LDS (64-bit LDS atomics), every non-zero word flushed once.  The harmonic loop is a run-time loop and every k's
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

// pass 1: out must be zeroed.  As radial_max_kernel: a thread folds its trips, the workgroup folds its threads in LDS, lane 0
// sends one atomic per maximum.
template <bool RATES, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void modes_max_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                           const Real *__restrict__ mass, int64_t n, RadCentre ctr, int M,
                                                           ModMax *__restrict__ out)
{
    __shared__ double sh[2][kBlock];
    __shared__ int sh_flag[kBlock];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double a = 0.0, d = 0.0;
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
        if (!bad) { if (ba > a) a = ba; if (bd > d) d = bd; }
        flag |= bad ? 1 : 0;
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = d;
    sh_flag[threadIdx.x] = flag;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double b = sh[p][threadIdx.x + h];
                if (b > sh[p][threadIdx.x]) sh[p][threadIdx.x] = b;
            }
            sh_flag[threadIdx.x] |= sh_flag[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(sh[p][0]);
            if (b) atomicMax(&out->bits[p], b);
        }
        if (sh_flag[0] & 1) atomicOr(&out->bad, 1ull);
    }
}

// pass 2: planes[p][slot] += contribution, planes[P - 1][slot] += 1, S = nb + 2 slots per plane.  gridDim.x workgroups stride
// over the bodies; every workgroup has at least one body (the host sizes the grid so).  Dynamic LDS, no static LDS at all (the
// private histogram may take the whole 64 KiB a launch can ask for):
//   tile == 0 (private): P * S words of histogram, then the nb + 1 squared edges.
//   tile > 0:  P * tile words.  The edges are searched in memory; a first trip over the workgroup's bodies takes the range of
//              slots they touch (in the first two words of the LDS, before the histogram is cleared); a range of at most `tile`
//              slots is summed in LDS at that offset, P rows of the range's width; a wider one goes to memory directly.
// The same integers either way, so the same planes.
template <bool RATES, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void modes_deposit_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                               const Real *__restrict__ mass, int64_t n, RadCentre ctr,
                                                               const double *__restrict__ e2_mem, int nb, int M, int tile, int eA, int eD,
                                                               long long *__restrict__ planes)
{
    extern __shared__ unsigned long long mod_lds[];
    const int S = nb + 2;
    const int nA = 1 + 2 * M;
    const int P = (RATES ? 2 : 1) * nA + 1;
    unsigned long long *hist = mod_lds;
    const double *e2 = e2_mem;
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    int s0 = 0, width = S;
    bool tiled = true;                         // (workgroup-uniform)
    if (tile == 0) {
        double *e2_lds = reinterpret_cast<double *>(mod_lds + (size_t)P * S);
        for (int k = threadIdx.x; k <= nb; k += kBlock) e2_lds[k] = e2_mem[k];
        e2 = e2_lds;
    } else {
        int *range = reinterpret_cast<int *>(mod_lds);             // first and last slot touched
        if (threadIdx.x == 0) { range[0] = INT32_MAX; range[1] = INT32_MIN; }
        __syncthreads();
        int lo = INT32_MAX, hi = INT32_MIN;
        for (int64_t i = first; i < n; i += stride) {
            const Real2 pp = pos[i];
            const double dx = (double)pp.x - ctr.cx, dy = (double)pp.y - ctr.cy;
            const int s = radial_slot(e2, nb, dx * dx + dy * dy);
            lo = min(lo, s); hi = max(hi, s);
        }
        if (lo <= hi) { atomicMin(&range[0], lo); atomicMax(&range[1], hi); }
        __syncthreads();
        s0 = range[0];
        width = range[1] - s0 + 1;             // (>= 1: the workgroup has a body)
        tiled = width <= tile;
        __syncthreads();                       // (every thread has read the range before the words are cleared)
        if (!tiled) { s0 = 0; width = S; }
    }
    if (tiled)
        for (int k = threadIdx.x; k < P * width; k += kBlock) hist[k] = 0ull;
    __syncthreads();
    // row p of the histogram (tiled) or of the planes (not): where slot s of plane p is
    auto put = [&](int p, int s, long long v) {
        if (!v) return;
        if (tiled) atomicAdd(&hist[p * width + (s - s0)], (unsigned long long)v);
        else atomicAdd(reinterpret_cast<unsigned long long *>(planes + (int64_t)p * S + s), (unsigned long long)v);
    };
    for (int64_t i = first; i < n; i += stride) {
        double r2, c1, s1, m, mw;
        modes_body<RATES>(pos, vel, mass, i, ctr, r2, c1, s1, m, mw);
        const int slot = radial_slot(e2, nb, r2);
        put(0, slot, (long long)rint(ldexp(m, eA)));
        if constexpr (RATES) put(nA, slot, (long long)rint(ldexp(mw, eD)));
        double c = 1.0, s = 0.0;
        for (int k = 1; k <= M; ++k) {
            const double cn = c * c1 - s * s1, sn = s * c1 + c * s1;
            c = cn; s = sn;
            put(2 * k - 1, slot, (long long)rint(ldexp(m * c, eA)));
            put(2 * k, slot, (long long)rint(ldexp(m * s, eA)));
            if constexpr (RATES) {
                put(nA + 2 * k - 1, slot, (long long)rint(ldexp(mw * c, eD)));
                put(nA + 2 * k, slot, (long long)rint(ldexp(mw * s, eD)));
            }
        }
        put(P - 1, slot, 1ll);
    }
    if (tiled) {
        __syncthreads();
        for (int k = threadIdx.x; k < P * width; k += kBlock) {
            const int p = k / width, t = k - p * width;
            const unsigned long long v = hist[k];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(planes + (int64_t)p * S + s0 + t), v);
        }
    }
}
}  // namespace bh
