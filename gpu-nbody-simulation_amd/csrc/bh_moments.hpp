// bh_moments.hpp -- moment maps: the mass, momentum and velocity-square of every body deposited on a caller's grid
// (bh_moment_map, bh_moment_map_max, bh_moment_map_deposit).  The reference has no such output: its pictures are drawn on
// the host from the downloaded state.  Included by bh_engine.hip, so it is compiled with -ffp-contract=off: nothing below is
// fused.
//
// Per body, in fp64 in exactly this order (an fp32 state is widened first, which is exact):
//   q0 = m      q1 = m * vx      q2 = m * vy      q3 = m * (vx * vx + vy * vy)
// Grid: nx x ny cells over [xmin, xmax) x [ymin, ymax); sx = nx / (xmax - xmin), sy = ny / (ymax - ymin), one IEEE
// division each, formed on the host.
//   NGP  tx = (x - xmin) * sx; the body goes whole to cell floor(tx) when 0 <= tx < nx and x < xmax; y likewise.  (x < xmax is
//        what keeps a body exactly at xmax outside: (xmax - xmin) * sx can round below nx.)
//   CIC  tx = (x - xmin) * sx - 0.5, ix = floor(tx), fx = tx - ix; corners (ix, 1 - fx) and (ix + 1, fx); y likewise; the
//        weight of a corner is wx * wy; corners outside the grid are dropped, the others kept.
// "Outside" is decided on the fp64 tx before any conversion to an integer: a body at 1e300 (or an overflowing product)
// fails every comparison and converts nothing.
//
// Fixed-point accumulation.  A first pass reduces max |q_p| per plane -- a maximum does not depend on the order -- and
// whether any coordinate, velocity or mass is not finite.  With E_p the frexp exponent of that maximum (max < 2^E_p) and
// L = ceil(log2(max(n, 1))) of the WHOLE system's body count, a contribution is
//   (int64) rint(ldexp(q_p * (wx * wy), 62 - E_p - L))           (NGP: q_p itself)
// added with a 64-bit integer atomic.  |q w| < 2^E_p, so a contribution is at most 2^(62 - L) and n <= 2^L of them (a body
// gives a cell at most one) stay within 2^62: no overflow.  Integer addition is associative: the planes do not depend on
// the launch shape, the order of the bodies in memory, or how many contexts deposited parts of the system into grids that
// are then added.  Each contribution is rounded once, by at most half a unit of 2^-(62 - E_p - L).
// A maximum of 0 gives the exponent 0 (every contribution of that plane is 0 anyway).
//
// Launch shape: one thread per body over the state as it lies in memory (after a physical re-order that is the curve order,
// so neighbouring lanes hit neighbouring cells), workgroups of kBlock; a workgroup whose bodies touch few cells sums them in
// LDS first (moment_deposit_kernel).  All memory traffic is ordinary vector loads, stores and atomics.
#pragma once

#include "bh_binned.hpp"

namespace bh {

constexpr int kMapPlanes = 4;
constexpr int64_t kMapMaxCells = (int64_t)1 << 24;     // = BH_MAP_MAX_CELLS: 4 planes of int64 are 512 MiB there

// what the first pass leaves: the bit patterns of max |q_p| (non-negative doubles order like their patterns) and a flag
struct MapMax {
    unsigned long long bits[kMapPlanes];
    unsigned long long bad;            // != 0: a non-finite coordinate, velocity, mass or moment
};

struct MapGrid {
    double xmin, xmax, ymin, ymax, sx, sy;
    int32_t nx, ny;
    int32_t e[kMapPlanes];             // 62 - E_p - L
};

__device__ __forceinline__ bool map_finite(double v) { return fabs(v) < (double)INFINITY; }      // false for NaN too

template <typename Real2, typename Real>
__device__ __forceinline__ void map_moments(const Real2 *__restrict__ vel, const Real *__restrict__ mass, int64_t i,
                                            double (&q)[kMapPlanes])
{
    const Real2 vv = vel[i];
    const double m = (double)mass[i], vx = (double)vv.x, vy = (double)vv.y;
    q[0] = m;
    q[1] = m * vx;
    q[2] = m * vy;
    q[3] = m * (vx * vx + vy * vy);
}

// pass 1: out must be zeroed.  One thread per body; fold_maxima (bh_binned.hpp) folds the workgroup and sends its atomics.
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void moment_max_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                            const Real *__restrict__ mass, int64_t n, MapMax *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a[kMapPlanes] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    if (i < n) {
        const Real2 pp = pos[i], vv = vel[i];
        bad = !(map_finite((double)pp.x) && map_finite((double)pp.y) && map_finite((double)vv.x) && map_finite((double)vv.y) &&
                map_finite((double)mass[i]));
        double q[kMapPlanes];
        map_moments(vel, mass, i, q);
#pragma unroll
        for (int p = 0; p < kMapPlanes; ++p) bad |= !map_finite(q[p]);        // finite inputs whose moment overflows fp64
#pragma unroll
        for (int p = 0; p < kMapPlanes; ++p) a[p] = bad ? 0.0 : fabs(q[p]);
    }
    if (fold_maxima(a, bad, out)) atomicOr(&out->bad, 1ull);
}

// pass 2: planes[p][iy][ix] += contribution; *deposited += bodies with at least one corner inside (one atomic per wave).
// The workgroup takes the bounding box of the cells its 256 bodies touch (LDS min / max).  When the box has at most kMapTileCells
// cells -- the usual case once the state lies in curve order -- the contributions are summed in a workgroup-private tile in LDS
// (64-bit LDS atomics, 32 KiB) and every non-zero tile cell goes to memory once; else every contribution goes to memory
// directly.  The same integers either way, so the same planes.  Contributions that round to zero are skipped.
constexpr int kMapTileCells = 1024;

template <bool CIC, typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void moment_deposit_kernel(const Real2 *__restrict__ pos, const Real2 *__restrict__ vel,
                                                                const Real *__restrict__ mass, int64_t n, MapGrid g,
                                                                long long *__restrict__ planes,
                                                                unsigned long long *__restrict__ deposited)
{
    __shared__ unsigned long long tile[kMapPlanes][kMapTileCells];
    __shared__ int box[4];             // x0, x1, y0, y1 of the cells touched
    if (threadIdx.x == 0) { box[0] = INT32_MAX; box[1] = INT32_MIN; box[2] = INT32_MAX; box[3] = INT32_MIN; }
    for (int k = threadIdx.x; k < kMapPlanes * kMapTileCells; k += kBlock) (&tile[0][0])[k] = 0ull;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t plane = (int64_t)g.nx * g.ny;
    constexpr int NC = CIC ? 4 : 1;
    int cxs[NC], cys[NC];
    double ws[NC];
    bool oks[NC];
    double q[kMapPlanes] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < NC; ++k) { oks[k] = false; cxs[k] = 0; cys[k] = 0; ws[k] = 0.0; }
    bool inside = false;
    if (i < n) {
        const Real2 pp = pos[i];
        const double x = (double)pp.x, y = (double)pp.y;
        map_moments(vel, mass, i, q);
        if constexpr (!CIC) {
            const double tx = (x - g.xmin) * g.sx, ty = (y - g.ymin) * g.sy;
            inside = tx >= 0.0 && tx < (double)g.nx && x < g.xmax && ty >= 0.0 && ty < (double)g.ny && y < g.ymax;
            if (inside) { oks[0] = true; cxs[0] = (int)floor(tx); cys[0] = (int)floor(ty); }
        } else {
            const double tx = (x - g.xmin) * g.sx - 0.5, ty = (y - g.ymin) * g.sy - 0.5;
            const double flx = floor(tx), fly = floor(ty);
            const double fx = tx - flx, fy = ty - fly;
            const bool okx[2] = {flx >= 0.0 && flx < (double)g.nx, flx >= -1.0 && flx < (double)(g.nx - 1)};
            const bool oky[2] = {fly >= 0.0 && fly < (double)g.ny, fly >= -1.0 && fly < (double)(g.ny - 1)};
            const double wx[2] = {1.0 - fx, fx}, wy[2] = {1.0 - fy, fy};
            inside = (okx[0] || okx[1]) && (oky[0] || oky[1]);
            if (inside) {
                const int ix = (int)flx, iy = (int)fly;
#pragma unroll
                for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                    for (int cx = 0; cx < 2; ++cx) {
                        const int k = 2 * cy + cx;
                        oks[k] = okx[cx] && oky[cy];
                        cxs[k] = ix + cx; cys[k] = iy + cy;
                        ws[k] = wx[cx] * wy[cy];
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if (oks[k]) {
                atomicMin(&box[0], cxs[k]); atomicMax(&box[1], cxs[k]);
                atomicMin(&box[2], cys[k]); atomicMax(&box[3], cys[k]);
            }
    }
    __syncthreads();
    const int x0 = box[0], y0 = box[2];
    const int64_t w = (int64_t)box[1] - x0 + 1, h = (int64_t)box[3] - y0 + 1;
    const bool any = box[1] >= x0;
    const bool tiled = any && w * h <= kMapTileCells;                       // (workgroup-uniform)
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (!oks[k]) continue;
#pragma unroll
        for (int p = 0; p < kMapPlanes; ++p) {
            const long long v = (long long)rint(ldexp(CIC ? q[p] * ws[k] : q[p], g.e[p]));
            if (!v) continue;
            if (tiled) atomicAdd(&tile[p][(cys[k] - y0) * (int)w + (cxs[k] - x0)], (unsigned long long)v);
            else atomicAdd(reinterpret_cast<unsigned long long *>(planes + p * plane + (int64_t)cys[k] * g.nx + cxs[k]), (unsigned long long)v);
        }
    }
    if (tiled) {
        __syncthreads();
        const int cells = (int)(w * h);
        for (int k = threadIdx.x; k < kMapPlanes * cells; k += kBlock) {
            const int p = k / cells, t = k - p * cells;
            const unsigned long long v = tile[p][t];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(planes + p * plane + (int64_t)(y0 + t / (int)w) * g.nx + (x0 + t % (int)w)), v);
        }
    }
    const unsigned long long votes = __ballot(inside);
    if ((threadIdx.x & (kWave - 1)) == 0 && votes) atomicAdd(deposited, (unsigned long long)__popcll(votes));
}
}  // namespace bh
