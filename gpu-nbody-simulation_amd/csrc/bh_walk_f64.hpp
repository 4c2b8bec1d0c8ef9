// bh_walk_f64.hpp -- fp64 theta-walk for THROUGHPUT (BH_PRECISION_F64): the reference's arithmetic type
// (project.cu:38-65) with the walk design of the fp32 kernel instead of the reference's visiting order.
// Replaces computeForcesGpu (project.cu:679-793) + updateAccVelPos (project.cu:819-836) like bh_walk_exact.hpp,
// and runs on exactly the tree the exact mode builds (keys by fp64 bisection, stable sort, cells, bottom-up
// centre-of-mass pass in the reference's child order): every node -- box, mass, centre of mass, occupant --
// is BITWISE the reference's.  What differs from BH_PRECISION_F64_EXACT is the walk only:
//   * free visiting order.  The four children of an opened cell are four consecutive NodeD / LinkD records
//     (node ids 1+4r .. 4+4r): one 128-byte + one 32-byte scalar load per opened cell instead of one 40-byte load
//     per visited node, and all four are evaluated before the next load is issued.  The first child some lane
//     opens stays in scalar registers and is the next cell taken (no push / pop); the others go to a
//     register-lane stack (entry k in lane k of three VGPRs, 128 entries: depth-first needs <= 3 * max_depth + 1).
//     A body's terms are therefore added in another order than the reference's: results agree with the oracle
//     to summation rounding (tests: <= 1e-12 relative), not bit for bit.
//   * the acceptance criterion on d^2 (round 4).  The reference accepts a cell when size / d < theta with
//     d = sqrt(d2) + 1e-15 (project.cu:634, 643), i.e. when d2 > (size / theta - 1e-15)^2: the build stores that
//     right-hand side in the node's `size` slot (f64_walk_threshold, bh_tree.hpp; only this walk reads the slot in this
//     precision), and ONE compare on d2 decides -- the reciprocal square root and everything after it are needed by
//     the accepting lanes only and are skipped for the cells every lane opens.  Decisions can differ from the
//     oracle's only where size / d is within a few 1e-16 of theta: the tests find identical per-body interaction
//     counts.
//   * 1/d by v_rsq_f64 and ONE Newton step instead of IEEE sqrt and three divisions per interaction
//     (project.cu:634, 651-655): v_rsq_f64 is good to ~2^-26, so with e = 1 - d2 y0^2 the step y = y0 + y0 e / 2
//     leaves 3 e^2 / 8 ~ 3e-16; the force is G m_i M d_vec / (d2 * d) with 1 / d2 = y^2 and
//     1 / d = 1 / (sqrt(d2) + 1e-15) = y - 1e-15 y^2 (second order: 1e-20 relative for d >= 1e-5).
//   * self skip, empty-node cut-off, depth-cap aggregation: the reference's rules unchanged (occupant index,
//     `mass <= 1e-15`, project.cu:617, 646), so reference_compat means what it means in the exact mode.
//   * the traversal loop is hand-written gfx950 assembly (walk64_asm; round 4), the C++ loop beside it states the same
//     abstract machine with the same operations in the same order and gives the same bits
//     (BH_FLAG_WALK_PORTABLE / BH_FLAG_WALK_STATS select it; tests/test_gpu_f64.py).
// Explicit fma() throughout: this header is compiled with -ffp-contract=off like the rest of the engine unit.
#pragma once

#include "bh_tree.hpp"

namespace bh {

#define BH64_CONSTANT __attribute__((address_space(4)))
extern "C" __device__ int bh64_writelane_i32(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

typedef int32_t w64_v16i __attribute__((ext_vector_type(16)));
typedef int32_t w64_v8i __attribute__((ext_vector_type(8)));

struct Quad64 {            // four sibling nodes as the scalar loads deliver them
    w64_v16i a, b;         // NodeD x 4: {cx, cy, m, thr} each, 8 dwords per node
    w64_v8i l;             // LinkD x 4: {child, occ}
};

__device__ __forceinline__ double w64_f64(int32_t lo, int32_t hi)
{
    return __hiloint2double(hi, lo);
}

// Four wavefronts per workgroup.  (Round 3's compiler-scheduled loop preferred one -- a workgroup's slot is only re-used when
// its LAST wave has finished, and its waves' walks take 0.3x .. 3x the mean: 1.088 -> 1.067 ms.  With the assembly loop at
// 8 resident waves it is the other way round, 0.682 -> 0.673 ms at N = 1M: profiles/r04_f64/walk_ab.txt.)
#ifndef BH_F64_BLOCK
#define BH_F64_BLOCK 256
#endif
constexpr int kF64Block = BH_F64_BLOCK;

// ---- the hand-written traversal loop ------------------------------------------------------------------------------
// What bounds this walk: every fp64 vector instruction costs a SIMD ~5.3 cycles per wave, v_rsq_f64 17
// (scripts/calib/f64_issue_calib.hip), so an evaluated node is ~26 vector cycles up to the compare and ~75 more where
// some lane accepts -- several times the scalar work around it, which other waves' vector instructions overlap.  Round 3's
// kernel wrapped hand-written arithmetic in compiler-scheduled control flow (21 scalar instructions and 8 branches per
// node; lane masks and the hand-off slot as booleans in SGPR pairs; the vector pipe 69 % busy).  Here, per child:
//   s_cmp + branch   empty-node cut-off on the mass's high dword (the exact `m <= 1e-15` out of line)
//   4 x fp64         dx, dy, d2
//   s_cmp + branch   leaf?  (a leaf narrows EXEC by the occupant test, v_cmpx_ne_u32, out of line)
//   v_cmpx_lt_f64    thr < d2: EXEC := the accepting lanes, vcc likewise
//   s_andn2 (SCC)    open = mask & ~vcc; nobody opens -> straight to the force
//   hand-off / push  the first opened child of the quad stays in s72 / s[68:69], the others are pushed (v_writelane x 3)
//   s_cbranch_execz  no lane accepts: the twelve instructions of the force are skipped
//   force            v_rsq_f64, Newton step (4), 1/d2, 1/d, weight (5), two v_fma_f64 into the sums -- under EXEC
//   s_mov exec       back to the quad's mask
// One quad per iteration (a quad is 40 SGPRs: two in flight do not fit the 102 a wave can have -- and they are not needed:
// a quad is ~300-400 vector cycles of work against a ~600-cycle round trip, three resident waves keep the pipe busy).
// Fixed SGPRs: s[24:55] the four nodes {cx, cy, m, thr} x 4, s[56:63] the links {child, occ} x 4, s[64:65] the quad's lane
// mask, s66 its index, s67 offsets, s[68:69] / s72 mask and index of the handed-over child (s72 == -1: none), s[70:71] open
// mask.  Fixed VGPRs: v[20:23] the body's position, v[24:27] dx dy, v[28:29] d2, v[30:31] y, v[32:35] scratch, v[36:39]
// the sums, v40 the body's index, v41 the index the reference's depth-cap occupant code compares equal to
// (reference_compat), v42..v44 / v45..v47 the stack (entry k in lane k & 63 of the first / second triple).
// Hazards the assembler does not handle inside inline assembly (gfx940 family): one wait state between v_rsq_f64 and its
// use; four between a VALU write of EXEC (v_cmpx) and v_writelane / v_readfirstlane -- the push path has s_andn2, two
// branches, an s_cmp and an s_nop in between, a pop is reached through the loop head; m0 is written at least one
// instruction before a lane select uses it.
// -DBH_ASM_GUARD=1 (first run of a rewritten loop on hardware): a wave leaves after 2^22 iterations whatever its
// stack says.
#if defined(BH_ASM_GUARD) && BH_ASM_GUARD
#define BH64_GUARD_INIT "s_mov_b32 s73, 0\n"
#define BH64_GUARD "s_add_u32 s73, s73, 1\n s_cmp_gt_u32 s73, 0x400000\n s_cbranch_scc1 Ldone_%=\n"
#define BH64_GUARD_CLOBBER "s73",
#else
#define BH64_GUARD_INIT ""
#define BH64_GUARD ""
#define BH64_GUARD_CLOBBER
#endif
// A/B hooks (scripts/f64_variants.sh; the product builds with neither): -DBH64_SETPRIO=1 raises a wave's priority from an
// iteration's start to its s_waitcnt as the fp32 loop does; -DBH64_LDS_PAD=bytes pads the workgroup's LDS to limit residency.
#if defined(BH64_SETPRIO) && BH64_SETPRIO
#define BH64_PRIO_UP "s_setprio 2\n"
#define BH64_PRIO_DOWN "s_setprio 0\n"
#else
#define BH64_PRIO_UP ""
#define BH64_PRIO_DOWN ""
#endif
// EPS: "" or BH64_EPS_ADD (Plummer softening: s2 = d2 + eps2 in place, after every decision has been taken on d2)
#define BH64_EPS_NONE ""
#define BH64_EPS_ADD "v_add_f64 v[28:29], v[28:29], %[eps2]\n"
#define BH64_FORCE(M, EPS)                                                                          \
    EPS                                                                                             \
    "v_rsq_f64_e32 v[30:31], v[28:29]\n"                                                            \
    "s_nop 0\n"                                                                                     \
    "v_mul_f64 v[32:33], v[28:29], v[30:31]\n"              /* t = d2 y0                */         \
    "v_fma_f64 v[34:35], -v[32:33], v[30:31], 1.0\n"        /* e = 1 - d2 y0^2          */         \
    "v_mul_f64 v[32:33], v[30:31], v[34:35]\n"              /* h = y0 e                 */         \
    "v_fma_f64 v[30:31], v[32:33], 0.5, v[30:31]\n"         /* y = y0 + h / 2           */         \
    "v_mul_f64 v[34:35], v[30:31], v[30:31]\n"              /* a = 1 / d2               */         \
    "v_fma_f64 v[32:33], v[34:35], %[ntiny], v[30:31]\n"    /* b = y - 1e-15 y^2 = 1/d  */         \
    "v_mul_f64 v[34:35], v[34:35], " M "\n"                 /* a M                      */         \
    "v_mul_f64 v[34:35], v[34:35], v[32:33]\n"              /* w = M / (d2 d)           */         \
    "v_fma_f64 v[36:37], v[34:35], v[24:25], v[36:37]\n"                                            \
    "v_fma_f64 v[38:39], v[34:35], v[26:27], v[38:39]\n"
#define BH64_CHILD(CX, CY, M, MHI, THR, CS, TAG, EPS)                                               \
    "s_cmp_gt_i32 " MHI ", 0x3cd203af\n"                    /* m > 1e-15 for sure */                \
    "s_cbranch_scc0 Lrare" TAG "_%=\n"                                                              \
    "Lcont" TAG "_%=:\n"                                                                            \
    "v_add_f64 v[24:25], " CX ", -v[20:21]\n"                                                       \
    "v_add_f64 v[26:27], " CY ", -v[22:23]\n"                                                       \
    "s_cmp_lt_i32 " CS ", 0\n"                                                                      \
    "v_mul_f64 v[28:29], v[26:27], v[26:27]\n"                                                      \
    "v_fma_f64 v[28:29], v[24:25], v[24:25], v[28:29]\n"                                            \
    "s_cbranch_scc1 Lleaf" TAG "_%=\n"                                                              \
    "v_cmpx_lt_f64_e32 vcc, " THR ", v[28:29]\n"                                                    \
    "s_andn2_b64 s[70:71], s[64:65], vcc\n"                                                         \
    "s_cbranch_scc0 Lforce" TAG "_%=\n"                     /* nobody opens */                      \
    "s_cmp_gt_i32 s72, -1\n"                                                                        \
    "s_cbranch_scc1 Lpush" TAG "_%=\n"                                                              \
    "s_mov_b32 s72, " CS "\n"                               /* handed over in registers */          \
    "s_mov_b64 s[68:69], s[70:71]\n"                                                                \
    "Lforce" TAG "_%=:\n"                                                                           \
    "s_cbranch_execz Lskip" TAG "_%=\n"                                                             \
    BH64_FORCE(M, EPS)                                                                              \
    "Lskip" TAG "_%=:\n"                                                                            \
    "s_mov_b64 exec, s[64:65]\n"                                                                    \
    "Lnext" TAG "_%=:\n"
// out of line: the exact empty test (bits of 1e-15: 0x3CD203AF'9EE75616; for doubles that are not NaN a <= b is the same
// on their sign-magnitude integers, and a node's mass is a sum of the bodies' masses or +0.0), the occupant test of a
// leaf (project.cu:646), the push
#define BH64_STUBS(MLO, MHI, CS, OS, TAG, COMPAT_CMP, PUSHCHK)                                      \
    "Lrare" TAG "_%=:\n"                                                                            \
    "s_cmp_lt_i32 " MHI ", 0x3cd203af\n"                                                            \
    "s_cbranch_scc1 Lnext" TAG "_%=\n"                                                              \
    "s_cmp_le_u32 " MLO ", 0x9ee75616\n"                                                            \
    "s_cbranch_scc1 Lnext" TAG "_%=\n"                                                              \
    "s_branch Lcont" TAG "_%=\n"                                                                    \
    "Lleaf" TAG "_%=:\n"                                                                            \
    "v_cmpx_ne_u32_e32 vcc, " OS ", v40\n"                                                          \
    COMPAT_CMP(OS)                                                                                  \
    "s_branch Lforce" TAG "_%=\n"                                                                   \
    "Lpush" TAG "_%=:\n"                                                                            \
    "s_nop 0\n"                                                                                     \
    PUSHCHK(TAG)                                                                                    \
    "v_writelane_b32 v42, " CS ", m0\n"                                                             \
    "v_writelane_b32 v43, s70, m0\n"                                                                \
    "v_writelane_b32 v44, s71, m0\n"                                                                \
    "LpushBack" TAG "_%=:\n"                                                                        \
    "s_add_u32 m0, m0, 1\n"                                                                         \
    "s_branch Lforce" TAG "_%=\n"
#define BH64_COMPAT_ON(OS) "v_cmpx_ne_u32_e32 vcc, " OS ", v41\n"
#define BH64_COMPAT_OFF(OS) ""
// (the lane select of v_writelane and the shift count of s_lshl_b64 use m0[5:0]: entry k sits in lane k & 63)
#define BH64_PUSHCHK(TAG) "s_bitcmp1_b32 m0, 6\n s_cbranch_scc1 LpushHi" TAG "_%=\n"
#define BH64_NOCHK(TAG) ""
#define BH64_PUSH_HI(CS, TAG)                                                                       \
    "LpushHi" TAG "_%=:\n"                                                                          \
    "v_writelane_b32 v45, " CS ", m0\n"                                                             \
    "v_writelane_b32 v46, s70, m0\n"                                                                \
    "v_writelane_b32 v47, s71, m0\n"                                                                \
    "s_branch LpushBack" TAG "_%=\n"
#define BH64_POP_FAST                                                                               \
    "s_lshl_b64 exec, 1, m0\n"                                                                      \
    "v_readfirstlane_b32 s66, v42\n v_readfirstlane_b32 s64, v43\n v_readfirstlane_b32 s65, v44\n"
#define BH64_POP_DEEP                                                                               \
    "s_lshl_b64 exec, 1, m0\n"                                                                      \
    "s_bitcmp1_b32 m0, 6\n"                                                                         \
    "s_cbranch_scc1 LpopHi_%=\n"                                                                    \
    "v_readfirstlane_b32 s66, v42\n v_readfirstlane_b32 s64, v43\n v_readfirstlane_b32 s65, v44\n"  \
    "s_branch Lload_%=\n"                                                                           \
    "LpopHi_%=:\n"                                                                                  \
    "v_readfirstlane_b32 s66, v45\n v_readfirstlane_b32 s64, v46\n v_readfirstlane_b32 s65, v47\n"
#define BH64_LOOP(POP, COMPAT_CMP, PUSHCHK, HI_STUBS, EPS)                                          \
    "v_mov_b32_e32 v20, %[pxl]\n v_mov_b32_e32 v21, %[pxh]\n"                                       \
    "v_mov_b32_e32 v22, %[pyl]\n v_mov_b32_e32 v23, %[pyh]\n"                                       \
    "v_mov_b32_e32 v36, %[sxl]\n v_mov_b32_e32 v37, %[sxh]\n"                                       \
    "v_mov_b32_e32 v38, %[syl]\n v_mov_b32_e32 v39, %[syh]\n"                                       \
    "v_mov_b32_e32 v40, %[body]\n"                                                                  \
    "v_sub_u32_e32 v41, -2, v40\n"                          /* occ + 2 == -body, project.cu:646 */  \
    "s_mov_b32 m0, 0\n"                                                                             \
    BH64_GUARD_INIT                                                                                 \
    "Lloop_%=:\n"                                                                                   \
    BH64_GUARD                                                                                      \
    BH64_PRIO_UP                                                                                    \
    "s_cmp_gt_i32 s72, -1\n"                                                                        \
    "s_cbranch_scc1 Lhave_%=\n"                                                                     \
    "s_sub_u32 m0, m0, 1\n"                                 /* SCC = borrow: the stack was empty */ \
    "s_cbranch_scc1 Ldone_%=\n"                                                                     \
    POP                                                                                             \
    "s_branch Lload_%=\n"                                                                           \
    "Lhave_%=:\n"                                                                                   \
    "s_mov_b32 s66, s72\n"                                                                          \
    "s_mov_b64 s[64:65], s[68:69]\n"                                                                \
    "Lload_%=:\n"                                                                                   \
    "s_lshl_b32 s67, s66, 5\n"                                                                      \
    "s_load_dwordx16 s[24:39], %[gd], s67\n"                                                        \
    "s_load_dwordx16 s[40:55], %[gd], s67 offset:0x40\n"                                            \
    "s_lshl_b32 s67, s66, 3\n"                                                                      \
    "s_load_dwordx8 s[56:63], %[ld], s67\n"                                                         \
    "s_mov_b32 s72, -1\n"                                                                           \
    "s_mov_b64 exec, s[64:65]\n"                                                                    \
    "s_waitcnt lgkmcnt(0)\n"                                                                        \
    BH64_PRIO_DOWN                                                                                  \
    BH64_CHILD("s[24:25]", "s[26:27]", "s[28:29]", "s29", "s[30:31]", "s56", "0", EPS)              \
    BH64_CHILD("s[32:33]", "s[34:35]", "s[36:37]", "s37", "s[38:39]", "s58", "1", EPS)              \
    BH64_CHILD("s[40:41]", "s[42:43]", "s[44:45]", "s45", "s[46:47]", "s60", "2", EPS)              \
    BH64_CHILD("s[48:49]", "s[50:51]", "s[52:53]", "s53", "s[54:55]", "s62", "3", EPS)              \
    "s_branch Lloop_%=\n"                                                                           \
    BH64_STUBS("s28", "s29", "s56", "s57", "0", COMPAT_CMP, PUSHCHK)                                \
    BH64_STUBS("s36", "s37", "s58", "s59", "1", COMPAT_CMP, PUSHCHK)                                \
    BH64_STUBS("s44", "s45", "s60", "s61", "2", COMPAT_CMP, PUSHCHK)                                \
    BH64_STUBS("s52", "s53", "s62", "s63", "3", COMPAT_CMP, PUSHCHK)                                \
    HI_STUBS                                                                                        \
    "Ldone_%=:\n"                                                                                   \
    BH64_PRIO_DOWN                                                                                  \
    "s_mov_b64 exec, -1\n"                                  /* (the kernel runs the traversal with all lanes enabled) */ \
    "v_mov_b32_e32 %[sxl], v36\n v_mov_b32_e32 %[sxh], v37\n"                                       \
    "v_mov_b32_e32 %[syl], v38\n v_mov_b32_e32 %[syh], v39\n"
#define BH64_HI_STUBS BH64_PUSH_HI("s56", "0") BH64_PUSH_HI("s58", "1") BH64_PUSH_HI("s60", "2") BH64_PUSH_HI("s62", "3")
#define BH64_OPERANDS(EXTRA_IN)                                                                     \
    : [sxl] "+v"(sxl), [sxh] "+v"(sxh), [syl] "+v"(syl), [syh] "+v"(syh), "+{s72}"(first), "+{s[68:69]}"(mask)         \
    : [gd] "s"(gd), [ld] "s"(ld), [ntiny] "s"(ntiny), [pxl] "v"(pxl), [pxh] "v"(pxh), [pyl] "v"(pyl), [pyh] "v"(pyh),  \
      [body] "v"(body) EXTRA_IN                                                                     \
    : BH64_GUARD_CLOBBER                                                                            \
      "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s32", "s33", "s34", "s35", "s36", "s37", "s38", "s39",   \
      "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55",   \
      "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s70", "s71",                 \
      "m0", "vcc", "scc", "memory",                                                                 \
      "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35",   \
      "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47"

// Walks the subtree below quad `first` (node id of its first sibling) for the lanes in `mask`; the sums continue from
// (sx, sy).  gd / ld: the node and link arrays; byte offsets are 32-bit (the caller checks node_cap * 32 < 4 GiB).
// SOFT: eps2 (> 0) in a pair of VGPRs -- the vector file has sixteen to spare, the scalar file none.
#define BH64_NO_EXTRA
#define BH64_EPS_IN , [eps2] "v"(eps2)
#define BH64_WALK(POP, COMPAT_CMP, PUSHCHK, HI_STUBS)                                                                  \
    do {                                                                                                               \
        if constexpr (SOFT) asm volatile(BH64_LOOP(POP, COMPAT_CMP, PUSHCHK, HI_STUBS, BH64_EPS_ADD) BH64_OPERANDS(BH64_EPS_IN)); \
        else asm volatile(BH64_LOOP(POP, COMPAT_CMP, PUSHCHK, HI_STUBS, BH64_EPS_NONE) BH64_OPERANDS(BH64_NO_EXTRA)); \
    } while (0)
template <bool COMPAT, bool DEEP, bool SOFT>
__device__ __forceinline__ void walk64_asm(const char BH64_CONSTANT *gd, const char BH64_CONSTANT *ld, int32_t first, uint64_t mask,
                                           double px, double py, int32_t body, double eps2, double &sx, double &sy)
{
    const double ntiny = -1e-15;
    int32_t pxl = __double2loint(px), pxh = __double2hiint(px), pyl = __double2loint(py), pyh = __double2hiint(py);
    int32_t sxl = __double2loint(sx), sxh = __double2hiint(sx), syl = __double2loint(sy), syh = __double2hiint(sy);
    if constexpr (DEEP) {
        if constexpr (COMPAT) BH64_WALK(BH64_POP_DEEP, BH64_COMPAT_ON, BH64_PUSHCHK, BH64_HI_STUBS);
        else BH64_WALK(BH64_POP_DEEP, BH64_COMPAT_OFF, BH64_PUSHCHK, BH64_HI_STUBS);
    } else {
        if constexpr (COMPAT) BH64_WALK(BH64_POP_FAST, BH64_COMPAT_ON, BH64_NOCHK, "");
        else BH64_WALK(BH64_POP_FAST, BH64_COMPAT_OFF, BH64_NOCHK, "");
    }
    sx = w64_f64(sxl, sxh);
    sy = w64_f64(syl, syh);
}

// DEEP: trees deeper than 21 levels need more than 64 stack entries (3 * (max_depth - 1) + 1): a second register-lane
// tier, and a test on every push and pop that the usual depth does without.
// ASM: the hand-written loop (no counters); otherwise the C++ statement of the same machine.
struct WalkF64Args {
    const NodeD *gd;
    const LinkD *ld;
    const uint32_t *perm;
    double2 *pos, *vel;
    const double *mass;
    double2 *force_out;
    int64_t lo, hi;
    double G, dt;
    int32_t integrate, pad0;
    TreeCounters *ctr;
    uint32_t *body_counts;         // counting variant: accepted force evaluations per body, may be null
    double *slots;                 // bh_bounds.hpp: bounds records the new positions fold into (next root box), may be null
    int32_t bpw, pad1;             // bodies per wavefront, a power of two <= 64 (see walk_exact_kernel): few bodies, short chains
    double eps2;                   // Plummer softening: eps * eps; read by walk_f64_soft_kernel only
};

// SOFT (Plummer softening, bh_set_softening): an accepted term is taken at s2 = d2 + eps2 -- one fp64 add, then the same
// sequence on s2: y = 1 / sqrt(s2) by v_rsq_f64 and the Newton step, 1 / s2 = y^2, 1 / d = y - 1e-15 y^2 (the offset stays:
// eps -> 0 is continuous with the unsoftened walk).  Every decision -- the cut-off, the occupant test, thr < d2 -- stays on the
// geometric d2, so the term set does not depend on eps.  The body is one text, bh_walk_f64_body.hpp, compiled into two
// kernels: walk_f64_kernel (SOFT = false: instruction for instruction the code it was before) and walk_f64_soft_kernel.
template <bool COMPAT, bool STATS, bool DEEP = false, bool ASM = false>
__global__ __launch_bounds__(kF64Block) void walk_f64_kernel(WalkF64Args a)
{
    constexpr bool SOFT = false;
#include "bh_walk_f64_body.hpp"
}

template <bool COMPAT, bool STATS, bool DEEP = false, bool ASM = false>
__global__ __launch_bounds__(kF64Block) void walk_f64_soft_kernel(WalkF64Args a)
{
    constexpr bool SOFT = true;
#include "bh_walk_f64_body.hpp"
}

}  // namespace bh
