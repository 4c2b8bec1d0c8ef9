// bh_binned.hpp -- what the binned fixed-point sums share on the device: the tail of a first pass (fold_maxima) and the
// workgroup's histogram over radial slots (SlotHist).  The moment maps, the radial profiles, the azimuthal modes and the rotation
// curve all find max |q_p| per plane in a first pass and sum (int64) rint(ldexp(q_p, e_p)) per slot in a second; the sums are
// integers, so the planes depend on the per-body arithmetic alone -- map_moments, radial_body, modes_body, curve_body, which
// stay with their families -- and not on anything in here.  Included by bh_moments.hpp, the lowest header of that chain; part
// of the bh_engine.hip unit alone (-ffp-contract=off).  All memory traffic is ordinary vector loads, stores and atomics.
#pragma once

#include "bh_prims.hpp"

namespace bh {

struct RadCentre { double cx, cy, ux, uy; };

// the number of squared edges e2[0 .. nb] that are <= r2
__device__ __forceinline__ int radial_slot(const double *e2, int nb, double r2)
{
    int lo = 0, hi = nb + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e2[mid] <= r2) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The tail of a first pass: a thread brings the maxima a[P] of its bodies and its flag word; the workgroup (kBlock threads, all
// of them call) folds both in LDS, P * kBlock doubles and kBlock words of static LDS; thread 0 sends one atomic per non-zero
// maximum on its bit pattern (non-negative doubles order like their patterns; out->bits must have been zeroed) and gets the
// workgroup's flag word back, every other thread 0: what a flag means and where it goes is the kernel's.
template <int P, typename Rec>
__device__ __forceinline__ int fold_maxima(const double (&a)[P], int flag, Rec *__restrict__ out)
{
    __shared__ double sh[P][kBlock];
    __shared__ int sh_flag[kBlock];
#pragma unroll
    for (int p = 0; p < P; ++p) sh[p][threadIdx.x] = a[p];
    sh_flag[threadIdx.x] = flag;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const double b = sh[p][threadIdx.x + h];
                if (b > sh[p][threadIdx.x]) sh[p][threadIdx.x] = b;
            }
            sh_flag[threadIdx.x] |= sh_flag[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(sh[p][0]);
        if (b) atomicMax(&out->bits[p], b);
    }
    return sh_flag[0];
}

// A workgroup's sums over the S = nb + 2 radial slots of P planes, planes[p][slot] in memory.  gridDim.x workgroups stride over
// the bodies; every workgroup has at least one body (the host sizes the grid so).  slot_hist sets it up in the launch's dynamic
// LDS (no static LDS: a private histogram may take the whole 64 KiB a launch can ask for):
//   tile == 0 (private): P * S words of histogram, then the nb + 1 squared edges, copied there for radial_slot.
//   tile > 0:  P * tile words.  The edges are searched in memory; a first trip over the workgroup's bodies takes the range of
//              slots they touch (in the first two words of the LDS, before the histogram is cleared); a range of at most `tile`
//              slots is summed in LDS at that offset, P rows of the range's width; a wider one goes to memory directly.
// The same integers either way, so the same planes.  A tile that is a constant of the kernel leaves one path in its code.
struct SlotHist {
    unsigned long long *hist;                  // P rows of `width` words (tiled)
    long long *planes;
    const double *e2;                          // the edges radial_slot searches: in LDS (private) or in memory
    int P, S, s0, width;
    bool tiled;                                // (workgroup-uniform)

    // v into slot s of plane p; contributions that round to zero are skipped
    __device__ __forceinline__ void put(int p, int s, long long v) const
    {
        if (!v) return;
        if (tiled) atomicAdd(&hist[p * width + (s - s0)], (unsigned long long)v);
        else atomicAdd(reinterpret_cast<unsigned long long *>(planes + (int64_t)p * S + s), (unsigned long long)v);
    }

    // after the last put: every non-zero word of the histogram goes to memory once
    __device__ __forceinline__ void flush() const
    {
        if (!tiled) return;
        __syncthreads();
        for (int k = threadIdx.x; k < P * width; k += kBlock) {
            const int p = k / width, t = k - p * width;
            const unsigned long long v = hist[k];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(planes + (int64_t)p * S + s0 + t), v);
        }
    }
};

template <typename Real2>
__device__ __forceinline__ SlotHist slot_hist(unsigned long long *lds, int P, int nb, int tile, const double *__restrict__ e2_mem,
                                              long long *__restrict__ planes, const Real2 *__restrict__ pos, int64_t n,
                                              const RadCentre &ctr)
{
    const int S = nb + 2;
    SlotHist h{lds, planes, e2_mem, P, S, 0, S, true};
    if (tile == 0) {
        double *e2_lds = reinterpret_cast<double *>(lds + (size_t)P * S);
        for (int k = threadIdx.x; k <= nb; k += kBlock) e2_lds[k] = e2_mem[k];
        h.e2 = e2_lds;
    } else {
        int *range = reinterpret_cast<int *>(lds);                 // first and last slot touched
        if (threadIdx.x == 0) { range[0] = INT32_MAX; range[1] = INT32_MIN; }
        __syncthreads();
        int lo = INT32_MAX, hi = INT32_MIN;
        const int64_t stride = (int64_t)gridDim.x * kBlock;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
            const Real2 pp = pos[i];
            const double dx = (double)pp.x - ctr.cx, dy = (double)pp.y - ctr.cy;
            const int s = radial_slot(e2_mem, nb, dx * dx + dy * dy);
            lo = min(lo, s); hi = max(hi, s);
        }
        if (lo <= hi) { atomicMin(&range[0], lo); atomicMax(&range[1], hi); }
        __syncthreads();
        h.s0 = range[0];
        h.width = range[1] - h.s0 + 1;         // (>= 1: the workgroup has a body)
        h.tiled = h.width <= tile;
        __syncthreads();                       // (every thread has read the range before the words are cleared)
        if (!h.tiled) { h.s0 = 0; h.width = S; }
    }
    if (h.tiled)
        for (int k = threadIdx.x; k < P * h.width; k += kBlock) lds[k] = 0ull;
    __syncthreads();
    return h;
}
}  // namespace bh
