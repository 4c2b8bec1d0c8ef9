// bh_bounds.hpp -- the root box's bounds records, shared by the tree build and the walk kernels.
#pragma once

#include "bh_prims.hpp"

namespace bh {

// The root box of step s+1 is the min/max of the positions that step s's walk wrote.  Outside LET mode it is kept in
// kBoundSlots running {xlo, xhi, ylo, yhi} records: every workgroup of an integrating walk over all bodies -- in however many
// passes -- folds its min/max into one of them with four atomics (slot = workgroup index mod kBoundSlots).  When no walk has
// left the bounds (the first build after an upload, n < 2), the positions pass bounds_partial folds them in instead.  The next
// build's keys_kernel reduces the 64 records in every one of its workgroups -- 2 KB from L2 -- pads the box and clears the
// step's counters; prep_kernel, two launches on, puts the records back to +-inf (no reader counter: it was 4,100 atomics on one
// word).  Records from a walk that are still all +-inf mean that the walk returned at once on an overflowed tree: the box in
// memory stays.  min / max are exact and order-free: any set of workgroups gives the same box, bit for bit.
constexpr int kBoundSlots = 64;
__device__ __forceinline__ void bounds_to_slot(double xlo, double xhi, double ylo, double yhi, double *slots, uint32_t group)
{
    double *s = slots + 4 * (group & (uint32_t)(kBoundSlots - 1));
    atomicMin(s + 0, xlo); atomicMax(s + 1, xhi); atomicMin(s + 2, ylo); atomicMax(s + 3, yhi);
}

// Block-level min/max of per-thread bounds, folded into `slots` (may be null); `partial` (may be null: only the fp32 walk in LET
// mode passes it) also gets this workgroup's four doubles.  All threads of the block must call it (it synchronises).
__device__ __forceinline__ void block_bounds(double xlo, double xhi, double ylo, double yhi, double *slots,
                                             double *__restrict__ partial = nullptr)
{
    __shared__ double sm[4][kWavesPerBlock];
    xlo = wave_min(xlo); xhi = wave_max(xhi); ylo = wave_min(ylo); yhi = wave_max(yhi);
    if (lane_id() == 0) { sm[0][wave_id()] = xlo; sm[1][wave_id()] = xhi; sm[2][wave_id()] = ylo; sm[3][wave_id()] = yhi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) {
            xlo = (sm[0][w] < xlo) ? sm[0][w] : xlo;  xhi = (xhi < sm[1][w]) ? sm[1][w] : xhi;
            ylo = (sm[2][w] < ylo) ? sm[2][w] : ylo;  yhi = (yhi < sm[3][w]) ? sm[3][w] : yhi;
        }
        if (partial) { partial[0] = xlo; partial[1] = xhi; partial[2] = ylo; partial[3] = yhi; }
        if (slots) bounds_to_slot(xlo, xhi, ylo, yhi, slots, blockIdx.x);
    }
}
// ... of one position per thread (none where !valid)
__device__ __forceinline__ void block_bounds(bool valid, double x, double y, double *slots, double *__restrict__ partial = nullptr)
{
    block_bounds(valid ? x : INFINITY, valid ? x : -INFINITY, valid ? y : INFINITY, valid ? y : -INFINITY, slots, partial);
}

// The constants of keys_kernel's one-multiply cell lookup (bh_tree.hpp, key_of_fast), written behind the root
// box by whoever sets it: box[4], box[5] = 2^Dm / width per axis; box[6], box[7] = the distance from a grid
// line, in cells, beyond which the lookup is provably the bisection's result (2.0 = never: degenerate or
// non-finite box, or a box so far from the origin that its grid lines are not resolved to a quarter cell).
__device__ __forceinline__ void write_key_consts_axis(double *box, int a, int Dm)
{
    const double side = (double)(1u << Dm);
    const double eps = (double)(Dm + 8) * 1.1102230246251565e-16 * side;
    const double lo = box[2 * a], hi = box[2 * a + 1];
    const double w = hi - lo, big = fmax(fabs(lo), fabs(hi));
    const double scale = side / w, margin = eps * (big / w);
    const bool ok = isfinite(scale) && scale > 0.0 && margin < 0.25;      // (a NaN margin fails the compare)
    box[4 + a] = ok ? scale : 0.0;
    box[6 + a] = ok ? margin : 2.0;
}
__device__ __forceinline__ void write_key_consts(double *__restrict__ box, int Dm)
{
    write_key_consts_axis(box, 0, Dm);
    write_key_consts_axis(box, 1, Dm);
}

}  // namespace bh
