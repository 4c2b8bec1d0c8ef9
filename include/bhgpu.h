/*
 * bhgpu.h -- C-ABI of libbhgpu.so, the MI355X-native Barnes-Hut step.
 *
 * The reference (DavidSevic/gpu-nbody-simulation) has NO library interface: its three
 * programs are configured by -D macros and by editing source (README.md:9-18), and the only
 * stable contract is file level.  This header is therefore the boundary a
 * maintainer would bind instead of calling runSimulationGpu() (project.cu:918-1024): each
 * entry point cites the reference function(s) it replaces.  Paths are relative to
 * /root/reference/implementation/.  INTEGRATION.md shows the ctypes stub and the three-line
 * change to a C++ main().
 *
 * Conventions
 *   - plain C types only; every call returns 0 on success or a negative bh_status;
 *     bh_last_error(ctx) gives the text.  No exceptions cross the boundary.
 *   - the caller owns every host buffer; the library owns all device memory.
 *   - host arrays use the reference's layout: positions/velocities AoS double[n][2],
 *     masses double[n] (project.cu:38-43).  Body order is the caller's order on every
 *     download, whatever order the device keeps internally.
 *   - one context per device; a context is not thread-safe; there are no globals.
 */
#ifndef BHGPU_H
#define BHGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BHGPU_ABI_VERSION 4   /* 2: bh_stats_t carries per-kernel-group times and algorithmic bytes;
                                 3: bh_get_interaction_counts, bh_build_info, bh_step_times,
                                    bh_stats_t.let_*_ms;
                                 4: bh_stats_t.wave_accepts, .walk_launches (the struct grew) */

typedef enum bh_status {
    BH_OK = 0,
    BH_ERR_ARG = -1,         /* bad argument (null pointer, n > capacity, ...)            */
    BH_ERR_DEVICE = -2,      /* HIP runtime error; text in bh_last_error                  */
    BH_ERR_NO_DEVICE = -3,   /* no usable GPU: the product has no CPU fallback            */
    BH_ERR_CAPACITY = -4,    /* tree needs more nodes than node_capacity                  */
    BH_ERR_STATE = -5,       /* call order (e.g. step before upload)                      */
    BH_ERR_IO = -6           /* cannot open/write a file                                  */
} bh_status;

typedef enum bh_precision {
    /* fp64 state, fp64 arithmetic in the reference's operation order, no FMA contraction:
     * results are bit-identical to the reference CPU path (project.cu:865-916). */
    BH_PRECISION_F64_EXACT = 0,
    /* fp32 state and arithmetic (BASELINE config "fp32"): the throughput mode. */
    BH_PRECISION_F32 = 1,
    /* fp64 state, fp32 forces (BASELINE config "fp64 positions / fp32 forces"): positions,
     * velocities and masses are kept and integrated in fp64, the tree keys and the centres of mass
     * are computed from the fp64 positions, the theta-walk runs in fp32 on rounded copies exactly
     * as in BH_PRECISION_F32.  For runs where a step's displacement is below the fp32 resolution
     * of the coordinates.  Single-GPU step and the LET distributed step; not the replicated one. */
    BH_PRECISION_MIXED = 2,
    /* fp64 end to end like the reference (project.cu:38-65) at THROUGHPUT: the tree is the exact mode's, node
     * for node bitwise the reference's; the walk takes the fp32 kernel's design (a hand-written gfx950 loop, four sibling
     * nodes per scalar load, free visiting order, the acceptance criterion of project.cu:643 as one compare on d^2, 1/d by
     * v_rsq_f64 + ONE Newton step instead of sqrt and three divisions).  Forces agree
     * with the reference CPU path to summation rounding (<= 1e-12 relative, same per-body interaction counts), not
     * bit for bit; trajectories therefore diverge from it as fast as the dynamics amplify 1e-15.  reference_compat,
     * max_depth and the empty-node cut-off mean what they mean in BH_PRECISION_F64_EXACT.  Single GPU. */
    BH_PRECISION_F64 = 3
} bh_precision;

/* bh_config.flags */
#define BH_FLAG_WALK_STATS   (1u << 0)  /* count visits/interactions in the walk (slower)   */
#define BH_FLAG_LDS_STACK    (1u << 1)  /* fp32 walk: LDS traversal stack instead of the
                                           register-lane stack (A/B switch)  */
#define BH_FLAG_WALK_NO_SPLIT (1u << 2) /* fp32 walk: always one wavefront per 64 bodies.  By
                                           default a launch of few bodies (<= ~100k: small N, or
                                           one rank's share) lets 4 or 8 wavefronts share each
                                           64-body group, level by level; same nodes, same
                                           per-body criterion, but another order of the fp32
                                           sums, so a body's last bits then depend on how many
                                           bodies its launch walks (still reproducible run to
                                           run).  Set this to rule that out.  BH_PRECISION_F64 likewise:
                                           launches of few bodies give a wavefront fewer than 64 of them
                                           (shorter walks), which changes the order of a body's fp64 sum;
                                           the flag pins 64.  (The bit-exact mode does the same and needs no
                                           flag: its order is the reference's whoever shares the wave.)   */

#define BH_FLAG_WALK_PORTABLE (1u << 3) /* fp32 and BH_PRECISION_F64 walks: the C++ traversal loop instead of the
                                           hand-scheduled gfx950 assembly loop.  Same operations
                                           in the same order -- results are bit-identical; kept
                                           as the readable statement of the loop and for tests.
                                           BH_PRECISION_F64_EXACT: the walk written as the reference
                                           writes it (sqrt, size / d < theta, three divisions per
                                           term; the nodes then carry sizes instead of exact d2
                                           thresholds) -- bit-identical again.                  */

/* Replaces the compile-time configuration of project.cu:1-11, 27-35, 60-62. */
typedef struct bh_config {
    int64_t  capacity;          /* max bodies (N_BODIES, project.cu:1-3)                    */
    double   theta;             /* THETA, project.cu:60 (0.5)                               */
    double   G;                 /* project.cu:27 (6.67e-11)                                 */
    double   dt;                /* DELTA_T, project.cu:29 (1.0)                             */
    int32_t  max_depth;         /* QUADTREE_MAX_DEPTH, project.cu:61 (10); root is depth 1;
                                   1..32                                                    */
    int32_t  precision;         /* bh_precision                                             */
    int32_t  reference_compat;  /* 1: depth-cap aggregation and the `occ+2 == -i` self skip
                                   exactly as project.cu:360-382, 646 (self-interaction
                                   artefact included).  0: F64_EXACT keeps the aggregation but
                                   uses main_approach_2.cpp's `occ == i` skip only (with
                                   max_depth 32 this is the uncapped tree of ma2.cpp); F32
                                   sums a depth-cap cell holding several (<= 1024) bodies body
                                   by body (bucket leaf), so no body interacts with its own
                                   cell; larger cells (degenerate inputs) are aggregated.     */
    int32_t  device;            /* HIP device ordinal                                       */
    int32_t  n_threads;         /* N_THREADS, project.cu:5-7, 703: at most this many bodies are walked
                                   at a time (rounded up to whole 256-thread workgroups; the passes run
                                   one after the other, as the reference's threads stride over the bodies).
                                   0 = all at once.  The launch SHAPE within a pass is CDNA4's, not the
                                   reference's (a12 is replaced, not kept).                              */
    uint32_t flags;             /* BH_FLAG_*                                                */
    int64_t  node_capacity;     /* 0 = automatic (8*capacity + 1024 nodes)                  */
} bh_config;

/* The reference's 12-double `Quadrant` (project.cu:46-65), as exported by bh_export_tree.
 * child[k] is an index INTO THE EXPORTED ARRAY (DFS pre-order), or -1. */
typedef struct bh_tree_node {
    double child[4];
    double comx, comy, mass;
    double xmin, xmax, ymin, ymax;
    double particle;
} bh_tree_node;

typedef struct bh_stats_t {
    int64_t  n_bodies;
    int64_t  n_nodes;            /* nodes of the last tree built                            */
    int64_t  n_internal;         /* subdivided cells of the last tree                       */
    int64_t  steps_done;
    uint64_t visits;             /* BH_FLAG_WALK_STATS: body-node visits of the last walk   */
    uint64_t interactions;       /* BH_FLAG_WALK_STATS: accepted force evaluations          */
    uint64_t wave_nodes;         /* BH_FLAG_WALK_STATS: nodes evaluated, counted once per
                                    wavefront (= distinct nodes per 64-body group)           */
    double   last_step_ms;       /* HIP-event time of the last bh_step call / nsteps        */
    double   build_ms;           /* bounds+keys+sort+nodes+COM of the last timed step       */
    double   walk_ms;            /* walk+integrate kernel of the last timed step            */
    uint64_t device_bytes;       /* device memory held by the context                       */
    /* per kernel group of the last timed step (HIP events on the context's stream):
     * the reference times "GPU parallel computation" as a whole (project.cu:957, 1008)          */
    double   keys_ms;            /* root box + keys (bounds_partial, keys_kernel)            */
    double   sort_ms;            /* radix passes (+ the state re-ordering when it ran)       */
    double   scan_ms;            /* cell counts, sorted copies, ranks, prefix sums           */
    double   nodes_ms;           /* node records (+ the bottom-up mass pass in exact mode)   */
    /* algorithmic bytes of that step: what each kernel must read and write once            */
    uint64_t build_bytes;        /* keys + sort passes + scan + nodes                        */
    uint64_t walk_bytes;         /* walk + integrate: 44 B per body + 20 B per node a
                                    wavefront evaluates (needs BH_FLAG_WALK_STATS, else 0)    */
    uint64_t wave_quads;         /* BH_FLAG_WALK_STATS: sibling quads loaded, counted once per
                                    wavefront (the walk's memory round trips)                 */
    uint64_t sort_spill_buckets; /* buckets of the bucket sort that did not fit on chip and were sorted
                                    through memory, since bh_create (0 in steady motion)      */
    /* the last bh_let_build (distributed step), HIP events on the context's stream (ABI 3)  */
    double   let_tree_ms;        /* global box + the local tree under it                     */
    double   let_pack_ms;        /* marking, numbering and packing the peers' LETs           */
    uint64_t sort_rerun_buckets; /* buckets of the bucket sort whose short sort (the top 24 bits of the keys' span, then
                                    runs of equal top bits by counting) met a run of more than 8 keys and was repeated
                                    with all byte passes, since bh_create (0 unless bodies pile up)          */
    /* ABI 4 */
    uint64_t wave_accepts;       /* BH_FLAG_WALK_STATS, the fp64 precisions: nodes some lane of the wavefront took a term from, counted once
                                    per wavefront -- the nodes that pay the reciprocal square root and the force (the
                                    others stop at the compare); 0 in the other precisions                          */
    uint64_t walk_launches;      /* walk kernel launches of the last bh_step / bh_compute_forces step: 1, or the passes
                                    of n_threads (project.cu:703)                                              */
} bh_stats_t;

typedef struct bh_ctx bh_ctx;

/* --- lifetime ---------------------------------------------------------------------------
 * Replaces the cudaMalloc block of runSimulationGpu (project.cu:932-940) and its cudaFree
 * block (:1014-1019).  Fails with BH_ERR_NO_DEVICE when no GPU is present. */
int bh_create(const bh_config *cfg, bh_ctx **out);
void bh_destroy(bh_ctx *ctx);
/* ctx may be NULL: then the text of the last failed bh_create on this thread. */
const char *bh_last_error(const bh_ctx *ctx);
int bh_abi_version(void);
/* What this binary was built from: "digest=<16 hex digits of the device sources> flags=<extra compiler flags>",
 * stamped by the build (gpu_nbody_simulation_amd/build.py, scripts/build_variants.sh).  bench.py prints it, so a
 * line measured on an A/B variant or a stale library says so (the reference has no counterpart: project.cu is
 * rebuilt by nvcc for every run, first_scaling_script.sh:30). */
const char *bh_build_info(void);

/* --- state ------------------------------------------------------------------------------
 * bh_upload replaces the three cudaMemcpy H2D of project.cu:943-945 (and, on the caller's
 * side, the arrays filled by loadSimulationDataFromText, project.cu:103-161).
 * bh_download replaces the per-step D2H of positions (project.cu:1010) and additionally
 * returns velocities, which the reference never exposes.  vel may be NULL.
 * Masses: BH_PRECISION_F64_EXACT reproduces the reference bit for bit for POSITIVE masses (however small).  A mass of
 * exactly 0.0 is accepted, but QuadInsert takes a leaf whose mass is 0.0 for empty (project.cu:395-397): a massless
 * body is overwritten by a later arrival and subdivides an earlier one, an insertion-order-dependent tree that
 * this build does not reproduce -- here a massless body occupies its leaf like any other (and pulls nobody).
 * BH_PRECISION_F32 / BH_PRECISION_MIXED: the mass and the moments of a tree cell of two or more bodies are differences
 * of fp64 prefix sums over ALL sorted bodies, so they carry an ABSOLUTE error of the order of H * 2^-53 times the total
 * mass and the total moments sum |m x|, sum |m y| of the system (H ~ 44 additions between a term and a prefix sum; above
 * 2,048 scan tiles 36 + one per 256 tiles).  That is far below the fp32 rounding of an ordinary cell's record; a cell
 * LIGHTER than that relative to the whole system is not resolved -- its mass is that noise, its centre arbitrary, and
 * whether the 1e-15f cut-off (project.cu:617) drops it is decided by the noise.  One-body cells take the body's own values. */
int bh_upload(bh_ctx *ctx, const double *pos, const double *vel, const double *mass, int64_t n);
int bh_download(bh_ctx *ctx, double *pos, double *vel);

/* bh_initialize replaces initializeGpu (project.cu:304-341): bodies are generated on the device
 * by a counter-based generator, reproducible for a given (seed, n).  kind 0 = the reference's box
 * distribution: masses in [lower_m, higher_m], positions in [lower_p, higher_p]^2, velocities in
 * [lower_v, higher_v]^2, each range log-uniform when both bounds are positive and linear otherwise
 * (generateRandomGpu, project.cu:84-97).  kind 1 = projected Plummer sphere (BASELINE config 3):
 * scale lower_p, truncation radius higher_p, equal masses higher_m, zero velocities.
 *
 * The generator is Philox-4x32-10 with the counter [i_lo, i_hi, stream, 0x9E3779B9] and the key [seed_lo, seed_hi]: body i is
 * a function of (seed, i) alone -- not of n, the capacity or the launch.  kind 0 takes the mass and x from stream 0, y and vx
 * from stream 1, vy from stream 2 (53 bits each); a linear range is u * (upper - lower) + lower in two roundings.
 *
 * kind 1, the rejection rule: the THREE-dimensional radius is drawn by inverting M(r) = r^3 / (r^2 + a^2)^(3/2) and drawn
 * again, from stream 16 + t for try t, while it lies beyond higher_p.  Up to 64 draws are made; AFTER THE 64TH THE LAST ONE
 * STANDS, beyond higher_p though it is.  A body ends that way with probability (1 - M(higher_p))^64: below 1e-12 for
 * higher_p >= a, about 0.2 at higher_p = 0.3 a.  (The truncation is of the sphere: the projected radius of every other
 * body is <= higher_p, with the law 1 - a^2 / (R^2 + a^2) (1 - R^2 / higher_p^2)^(3/2).)
 * kind 1 returns BH_ERR_ARG unless lower_p is finite and > 0, higher_p is > 0 (+inf: no truncation) and higher_m is finite;
 * lower_m, lower_v and higher_v are ignored.  kind 0 takes any ranges, as the reference does.
 * bh_download_masses returns the masses (the caller supplied them in bh_upload otherwise). */
int bh_initialize(bh_ctx *ctx, int64_t n, uint64_t seed, int32_t kind, double lower_m, double higher_m,
                  double lower_p, double higher_p, double lower_v, double higher_v);
int bh_download_masses(bh_ctx *ctx, double *mass);

/* --- the hot path -----------------------------------------------------------------------
 * bh_step: nsteps x { buildTree (project.cu:575-591), computeForcesGpu (:679-793),
 * updateAccVelPos (:819-836) }, i.e. the body of the step loop project.cu:955-1011, with
 * the tree built on the device instead of the host.  Asynchronous on the context's stream;
 * bh_sync / bh_download / bh_stats wait for it. */
int bh_step(bh_ctx *ctx, int32_t nsteps);
int bh_sync(bh_ctx *ctx);

/* The same three stages one at a time, for per-stage parity checks:
 * bh_build_tree   = buildTree            (project.cu:575-591)
 * bh_compute_forces = buildTree + computeForces/computeForcesGpu (project.cu:593-675, 679-793);
 *                   state is not advanced
 * bh_get_forces   -> forces[n][2], FORCE with m_i included as in the reference's `forces`
 * bh_get_accel    -> forces / m_i (updateAccelerations, project.cu:795-801)               */
int bh_build_tree(bh_ctx *ctx);
int bh_compute_forces(bh_ctx *ctx);
int bh_get_forces(bh_ctx *ctx, double *forces);
int bh_get_accel(bh_ctx *ctx, double *accel);

/* Per-body count of accepted force evaluations of the last walk -- the reference's walk has no such output; it is
 * the `inter++`-per-body of computeForces (project.cu:651-658 executed once per accepted node), which the parity
 * tests compare with the oracle's body by body: equal counts = the same acceptance decisions (project.cu:643).
 * Needs BH_FLAG_WALK_STATS; fp32, mixed precision and BH_PRECISION_F64; caller order. */
int bh_get_interaction_counts(bh_ctx *ctx, uint32_t *counts);

/* --- diagnostics: potential, energy, momentum --------------------------------------------
 * The reference has NO potential or energy at all (project.cu computes forces only); these entry points are new.
 * phi_i = -G sum_j M_j / d_ij over exactly the terms the precision's force walk takes for body i -- the term set of
 * computeForces (project.cu:617-658): the `mass <= 1e-15` cut-off, the same acceptance decisions, the self skip
 * (`occ == i`, and `occ + 2 == -i` under reference_compat), depth-cap aggregates, fp32 bucket leaves body by body.
 * d is the force walk's distance: sqrt(d2) + 1e-15 in the fp64 precisions (project.cu:630-634), the fp32 walk's
 * 1 / rsq(d2) in BH_PRECISION_F32 / MIXED (fp32 terms, fp64 sums).  Single GPU: a context in LET mode or with
 * world > 1 gets BH_ERR_STATE (LET mode has bh_let_potential / bh_let_energy, below).
 * The diagnostics do not perturb the run: a following bh_step computes the trajectory bit for bit as it would have
 * without them, in every precision.  They build their own tree of the current state (which bh_export_tree then
 * exports) but leave the forces, interaction counts, step timings and walk_launches of the last force walk as they
 * were: bh_get_forces still returns the forces of the last bh_step / bh_compute_forces.  The device buffers are
 * allocated on first use (bh_stats.device_bytes grows then, not before). */
typedef struct bh_energy_t {
    double kinetic, potential, total;   /* 1/2 sum m |v|^2, 1/2 sum m_i phi_i, their sum        */
    double momentum[2];                 /* sum m v                                              */
    double angular_momentum;            /* sum m (x v_y - y v_x), about the origin              */
    double com[2];                      /* sum m x / sum m                                      */
    double mass;                        /* sum m                                                */
    int64_t n_bodies;
} bh_energy_t;

/* Builds the tree of the CURRENT state and runs the potential walk (one launch over all bodies, whatever
 * n_threads); the state is not advanced. */
int bh_compute_potential(bh_ctx *ctx);
/* phi[n] (per unit mass) and, if counts != NULL, the terms summed per body -- equal to the force walk's per-body
 * interaction counts (project.cu:651-658 once per accepted node); caller order.  BH_ERR_STATE unless the last
 * bh_compute_potential / bh_energy saw the current state. */
int bh_get_potential(bh_ctx *ctx, double *phi, uint32_t *counts);
/* Runs bh_compute_potential unless the potential is current, then deterministic fp64 reductions on the device
 * (fixed-shape partials, Neumaier-compensated, folded in a fixed order: two calls on the same state return the
 * same bits).  Only the final sums reach the host. */
int bh_energy(bh_ctx *ctx, bh_energy_t *out);

/* --- exact forces and the Barnes-Hut force error ------------------------------------------
 * bh_direct_forces: fp64 direct-sum forces of the CURRENT state, computeForces of main_approach_1.cpp:53-75 bit for
 * bit (in BH_PRECISION_F32 of the fp32 state widened exactly): for each target i, the sum over j = 0 .. n-1 in caller
 * order, j != i, of ((G m_i) m_j) / (d2 d) * (dx, dy) with IEEE sqrt and division, in every precision.  targets:
 * caller indices (any order, repeats allowed), or NULL for all n bodies in caller order (then n_targets must be n);
 * forces[n_targets][2], FORCE with m_i included.  Reads the state only: no tree, nothing of the run changes.
 * Coincident bodies give inf / NaN as in the reference (NaN payloads are not part of the contract).
 * bh_force_check: tree[k][2] are the precision's Barnes-Hut forces of the current state -- a tree built as the
 * diagnostics build theirs and the force walk bh_compute_forces would run (n_threads applies), accelerations times m_i
 * in BH_PRECISION_F32 / MIXED -- and direct[k][2] the bh_direct_forces of the same targets.  A following bh_step is
 * bit for bit unchanged, and bh_get_forces, bh_get_interaction_counts, bh_stats (walk_launches, the walk counters) and
 * the ORB weights still describe the last real force walk.
 * Both: BH_ERR_ARG for a null output array, n_targets < 0 or a target outside [0, n); BH_ERR_STATE before upload and in
 * LET mode or with world > 1.  n_targets = 0 is valid.  Device buffers are allocated on first use. */
int bh_direct_forces(bh_ctx *ctx, const int64_t *targets, int64_t n_targets, double *forces);
int bh_force_check(bh_ctx *ctx, const int64_t *targets, int64_t n_targets, double *tree, double *direct);

/* --- the field at arbitrary points ----------------------------------------------------------
 * bh_field_at: what the precision's Barnes-Hut walk of the CURRENT state gives at caller coordinates that are nobody's.
 * points[n_points][2]; accel[n_points][2] the acceleration (force per unit mass, G included), phi[n_points] the potential
 * per unit mass over the same terms, counts[n_points] the number of terms taken; any output may be NULL, but not all
 * three.  Results are in the order of `points`.
 * Term set: exactly the terms the precision's force walk would take for a body standing at the point -- the
 * `mass <= 1e-15` cut-off, the force walk's acceptance decisions (read from the node data it compares against),
 * depth-cap aggregates as point masses, fp32 bucket leaves body by body -- without any self skip: a point is no body.
 *   BH_PRECISION_F64_EXACT / F64: d = sqrt(d2) + 1e-15, a += ((G M) / d2) * (dx / d), phi -= (G M) / d
 *     (project.cu:630-658 with m_i = 1), IEEE sqrt and division.  A point that COINCIDES with a body gets what that
 *     expression gives there: inf * 0, a non-finite acceleration (the potential stays finite: -G M / 1e-15).
 *   BH_PRECISION_F32 / MIXED: the point is rounded to fp32 on the device; the fp32 walk's terms (ri = rsq(d2),
 *     w = m ri ri ri; w dx, w dy, m ri) in fp32, summed in fp64, times G in fp64.  A node or bucket body at d2 == 0
 *     contributes nothing, as in the fp32 walk.
 * A point's result does not depend on the other points of the call, their order or their number (the points are
 * Morton-sorted on the device and walked 64 to a wavefront, up to 2^20 per launch; every lane adds its own terms in a
 * fixed order).  Points outside the root box are valid.  With no bodies the field is 0 and the counts are 0.
 * Like the diagnostics, the call builds its own tree of the current state and does not perturb the run: a following
 * bh_step is bit for bit what it would have been, and bh_get_forces, bh_get_interaction_counts, bh_stats (the walk
 * counters, walk_launches), the step timings and the ORB weights still describe the last real force walk.
 * BH_ERR_ARG: n_points < 0, points == NULL with n_points > 0, all outputs NULL, a non-finite coordinate (checked
 * before anything is enqueued).  BH_ERR_STATE before upload, in LET mode or with world > 1.  n_points = 0 is valid.
 * Device buffers for one launch are allocated on first use (bh_stats.device_bytes grows then). */
int bh_field_at(bh_ctx *ctx, const double *points, int64_t n_points, double *accel, double *phi, uint32_t *counts);

/* --- Plummer softening (opt-in; additive entry points, the ABI version stays 4) -----------------------
 * bh_set_softening: a softening length eps >= 0 for every term the context evaluates from then on; 0 (the default) is
 * the reference's unsoftened law, and every launch then takes the kernels it has always taken.  With d2 = dx^2 + dy^2
 * the geometric squared distance a walk computes and s2 = d2 + eps^2:
 *   decisions stay on d2 -- the acceptance compare, the fp32 leaf test d2 > 0 (the body itself or an exactly coincident
 *     body contributes nothing), the `mass <= 1e-15` cut-off, the self skip by index.  The term set, and so every
 *     per-body interaction and term count, is the same for any eps on the same state;
 *   only the magnitude of an accepted term uses s2: force G m_i M (dx, dy) / s2^(3/2), potential -G M / sqrt(s2).
 *   BH_PRECISION_F32 / MIXED (force walk, bucket leaves body by body, forest walk, potential, field): eps2 =
 *     (float)(eps * eps), the product formed in fp64; ri = rsq(d2 + eps2), one fp32 add, then w = m ri ri ri, w dx, w dy,
 *     m ri as before.  An eps2 that rounds to 0.f runs the unsoftened kernels.
 *   BH_PRECISION_F64 (force walk): s2 = d2 + eps * eps, one fp64 add, then the walk's sequence on s2: y = 1 / sqrt(s2) by
 *     the reciprocal square root and one Newton step, 1 / s2 = y^2, 1 / d = y - 1e-15 y^2 (the 1e-15 offset stays, so
 *     eps -> 0 is continuous with the unsoftened walk).
 *   fp64 potential and field: d = sqrt(s2) + 1e-15, a += ((G M) / s2) * (dx / d), phi -= (G M) / d, IEEE sqrt and
 *     division (BH_FLAG_WALK_PORTABLE nodes: size / d < theta keeps the geometric d).
 *   bh_direct_forces, and so bh_force_check: d = sqrt(s2), ((G m_i) m_j) / (s2 d), same order, j == i skipped by index;
 *     distinct coincident bodies give a finite zero force.
 *   BH_PRECISION_F64_EXACT: its contract is the reference's bits and the reference has no softening -- eps != 0 is
 *     BH_ERR_ARG there (eps = 0 is accepted).
 * May be called at any time between calls and takes effect at the next walk; it marks the potential as not current
 * (bh_get_potential / bh_let_get_potential return BH_ERR_STATE until it is recomputed).  In a distributed run eps is a
 * property of the run: the caller gives every rank's context the same value.
 * BH_ERR_ARG: eps negative or not finite, or eps != 0 in BH_PRECISION_F64_EXACT.
 * bh_get_softening: the length last set (0 by default). */
int bh_set_softening(bh_ctx *ctx, double eps);
int bh_get_softening(bh_ctx *ctx, double *eps);

/* --- kick, drift, a time-step criterion and the KDK leapfrog (opt-in; additive entry points, the ABI version stays 4) ---
 * bh_step advances the state by the reference's fused kick-drift at cfg.dt (updateAccVelPos, project.cu:819-836:
 * v += a dt; p += v dt, symplectic Euler): first order, and the velocities a download returns sit half a step away from the
 * positions.  These entry points advance velocities and positions SEPARATELY, from the forces the device already holds.
 * "The forces are current" below means: the force buffer holds the accelerations of the current positions of all bodies.
 *   That is so after a completed bh_compute_forces (whatever n_threads) and after bh_step_kdk.  It stops being so at any
 *   integrating walk (bh_step, bh_step_local), bh_drift, bh_upload, bh_initialize, bh_migrate_unpack, a bh_set_softening
 *   that changes the length, and bh_build_tree (a build that may re-order the state without a force walk after it).
 *   bh_kick keeps it (the positions do not move), and so do the diagnostics -- bh_energy, bh_compute_potential,
 *   bh_field_at, bh_direct_forces, bh_force_check: they leave the force buffer and the device order alone.
 * bh_kick: v += a h for every body, a the acceleration in the force buffer.  One lane per device slot.
 *   BH_PRECISION_F32:       v' = fma32(a, (float)h, v), a the fp32 acceleration the walk wrote.
 *   BH_PRECISION_MIXED:     v' = fma64((double)a32, h, v), the fp64 h unrounded.
 *   BH_PRECISION_F64:       a = F / m_i, one IEEE division (the buffer holds the force (G m_i) * sum), v' = fma64(a, h, v).
 *   BH_PRECISION_F64_EXACT: a = F / m_i, v' = v + a * h, unfused: updateAccelerations and updateVelocities
 *                           (project.cu:795-809) in their order.
 *   In the two fp64 precisions a body of mass exactly 0 gets a = 0 / 0, a NaN velocity, as in the reference.
 *   The potential stays current (it does not depend on the velocities).
 * bh_drift: p += v h.  F32: p' = fma32(v, (float)h, p); MIXED and F64: p' = fma64(v, h, p); F64_EXACT: p' = p + v * h,
 *   unfused.  The forces and the potential stop being current, the tree is invalid until the next build, and that build
 *   takes its root box from a pass over the positions (the drift folds no bounds).
 * Both: any finite h is valid, negative included; h = 0 launches nothing and leaves the arrays bit for bit as they were
 *   (bh_drift's state rules apply all the same).  The arithmetic is per body and does not depend on the device
 *   order.  bh_compute_forces, bh_kick(dt), bh_drift(dt) is bit for bit bh_step(1) in F32,
 *   MIXED and F64_EXACT; in F64 the fused step uses a = G * sum where the kick divides (G m_i) * sum by m_i (equal when
 *   the division is exact, e.g. masses that are powers of two).
 * bh_timestep: the criterion dt = eta * sqrt(length / a_max) over the same accelerations, reduced on the device.  Per body
 *   a2 = ax^2 + ay^2 in fp64 (fp32 accelerations widened first; fp64 precisions: a = F / m_i); a_max = sqrt(max a2); worst =
 *   the caller index of the maximum, the smallest such index on a tie.  length <= 0: the softening length (BH_ERR_ARG if
 *   that is 0 too).  A non-finite a2 (coincident bodies, a massless body in an fp64 precision) gives a_max = +inf, dt = 0 and
 *   worst = the smallest caller index with a non-finite a2; a_max == 0 gives dt = +inf; no bodies: a_max = 0, dt = +inf,
 *   worst = -1.  The maximum does not depend on the order of the reduction: two calls return the same bits.  Only the result
 *   words reach the host; the call waits for the stream.
 * bh_step_kdk: nsteps kick-drift-kick (leapfrog) steps at cfg.dt, asynchronous like bh_step:
 *     forces of the current state (skipped when they are current), bh_kick(dt/2), bh_drift(dt);
 *     nsteps - 1 fused steps -- the body of bh_step, the same kernels in the same batch: between two drifts the two half
 *       kicks are one whole kick on the same forces;
 *     forces, bh_kick(dt/2).
 *   On return velocities and positions are at the same time, so bh_energy is second order in dt; the forces are current,
 *   so a following bh_step_kdk costs nsteps walks, not nsteps + 1; steps_done advances by nsteps; bh_stats' step timings
 *   describe the call (last_step_ms = the whole call / nsteps, the per-step records end at each force walk).  nsteps = 0 is a
 *   no-op.  All four precisions; in BH_PRECISION_F64_EXACT every operation is the reference's, but the reference has no
 *   leapfrog, so there are no reference bits to match.  A tree that outgrows node_capacity is reported by bh_sync, as
 *   for bh_step.
 * Errors: BH_ERR_ARG for a null context or output, a non-finite h or eta, nsteps < 0.  BH_ERR_STATE before upload, in LET
 *   mode and with world > 1 (all four), and for bh_kick / bh_timestep when the forces are not current.  n = 0 is valid. */
typedef struct bh_timestep_t {
    double  dt;          /* eta * sqrt(length / a_max)                                       */
    double  a_max;       /* the largest |a|                                                  */
    int64_t worst;       /* caller index of the body that has it (-1: no bodies)             */
    int64_t n_bodies;
} bh_timestep_t;
int bh_kick(bh_ctx *ctx, double h);
int bh_drift(bh_ctx *ctx, double h);
int bh_timestep(bh_ctx *ctx, double eta, double length, bh_timestep_t *out);
int bh_step_kdk(bh_ctx *ctx, int32_t nsteps);
/* bh_forces_current: *current = 1 when the force buffer holds the accelerations of the current positions of all bodies under the
 * current law -- when bh_kick, bh_timestep and bh_rotation_curve would accept it --, else 0 (before any upload too).  It asks
 * the host's record only: no launch, no wait.  BH_ERR_ARG for a null pointer. */
int bh_forces_current(bh_ctx *ctx, int32_t *current);

/* --- moment maps: where the mass is, how it streams, how hot it is ----------------------------------------------------
 * The reference draws its pictures on the host from the downloaded state (plot_2d.py); these deposit on the device, so a
 * distributed run can map a system no rank holds.  Four moments of every body, each formed in fp64 in the written order
 * (an fp32 state is widened first, exactly), on nx x ny cells over box = {xmin, xmax, ymin, ymax}, half open:
 *     plane 0: m      plane 1: m * vx      plane 2: m * vy      plane 3: m * (vx * vx + vy * vy)
 * With sx = nx / (xmax - xmin) (one division), and likewise in y:
 *   BH_MAP_NGP: tx = (x - xmin) * sx; the whole body goes to cell (floor(tx), floor(ty)) when 0 <= tx < nx and x < xmax
 *     (and the same in y), else nowhere.  A body exactly at xmax is outside.
 *   BH_MAP_CIC: tx = (x - xmin) * sx - 0.5, ix = floor(tx), fx = tx - ix; the corners (ix, 1 - fx) and (ix + 1, fx), the
 *     same in y, a corner's weight wx * wy.  Corners outside the grid are dropped, the others kept: a body within half a
 *     cell of the box is partly inside.
 *   Inside and outside are decided on the fp64 tx: a body at 1e300 converts to no index.
 * Fixed point.  A first pass takes max |q_p| of every plane over the bodies; E_p is its frexp exponent (max < 2^E_p),
 * L = ceil(log2(max(n, 1))) for the n bodies of the WHOLE system, and the plane's exponent is 62 - E_p - L (0 when the
 * maximum is 0).  A contribution is (int64) rint(ldexp(q_p * (wx * wy), exponent)) (NGP: q_p itself), added with integer
 * atomics: the sums cannot leave int64 (n contributions of at most 2^(62 - L)), and, integer addition being associative,
 * they do not depend on the order of the bodies, the launch or the number of contexts whose grids are added -- the same
 * system gives the same bits.  Every contribution is rounded once: a cell is off by at most half a unit of 2^-exponent
 * per contribution it received.  value = planes * 2^-exponent.
 * bh_moment_map: both passes and the download.  planes: 4 * ny * nx, plane-major, y the outer axis of a plane.
 *   *n_deposited: the bodies with at least one corner inside.
 * bh_moment_map_max: the first pass alone, maxabs[p] = max |q_p| over this context's bodies (0 without bodies).
 * bh_moment_map_deposit: the second pass alone with the caller's exponents -- for a distributed map: the MAX of the
 *   ranks' maxima and the SUM of their body counts give every rank the same exponents -- and the grid left on the device:
 *   *planes_dev points at 4 * ny * nx int64, valid until the next moment-map call or bh_destroy.  Exponents too large for
 *   this context's own maxima and body count are refused.
 * Valid any time after bh_upload / bh_initialize / bh_migrate_unpack, in every precision, in LET mode too (the context's own
 * bodies); they read the state arrays bh_download reads, build no tree and change nothing a step reads: the steps around
 * them run bit for bit as they would have.  They wait for the stream.
 * Errors: BH_ERR_ARG for a null pointer, nx or ny < 1, nx * ny > BH_MAP_MAX_CELLS, an unknown scheme, a box that is empty or
 *   not finite (or whose extent overflows), and -- with a message that says so -- a body whose position, velocity or mass is
 *   not finite or whose moment overflows fp64.  BH_ERR_STATE before any upload. */
#define BH_MAP_NGP 0
#define BH_MAP_CIC 1
#define BH_MAP_MAX_CELLS 16777216
int bh_moment_map(bh_ctx *ctx, const double box[4], int32_t nx, int32_t ny, int32_t scheme,
                  int64_t *planes, int32_t exponents[4], int64_t *n_deposited);
int bh_moment_map_max(bh_ctx *ctx, double maxabs[4]);
int bh_moment_map_deposit(bh_ctx *ctx, const double box[4], int32_t nx, int32_t ny, int32_t scheme,
                          const int32_t exponents[4], void **planes_dev, int64_t *n_deposited);

/* --- radial profiles and Lagrangian radii: how the mass is arranged about a centre -----------------------------------------
 * The radial counterpart of the moment maps, on the device, so that a distributed run can profile a system no rank holds.
 * centre = {cx, cy}; centre_vel = {ucx, ucy} (NULL: 0).  Per body of the CURRENT state, in fp64 in the written order with
 * nothing fused (an fp32 state is widened first, exactly):
 *     dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy
 *     ux = vx - ucx;  uy = vy - ucy;  a = dx * ux + dy * uy;  b = dx * uy - dy * ux
 *     r2 >= 2^-1022:  r = sqrt(r2);  vr = a / r;  vt = b / r        r2 < 2^-1022 (zero or subnormal): vr = vt = 0
 *     q0 = m   q1 = m * vr   q2 = m * vt   q3 = m * (vr * vr)   q4 = m * (vt * vt)
 * Bins.  edges[nb + 1], 1 <= nb <= BH_RADIAL_MAX_BINS, finite, edges[0] >= 0, strictly ascending, and so are their squares
 *   e2[k] = edges[k] * edges[k] (formed once in fp64 on the host).  nb + 2 slots, decided on r2 alone: slot 0: r2 < e2[0];
 *   slot k + 1: e2[k] <= r2 < e2[k + 1]; slot nb + 1: r2 >= e2[nb].  A body exactly on an edge belongs to the bin above it.
 * Planes.  planes[6][nb + 2], plane-major.  Planes 0-4 are the sums of q0-q4 in the fixed point of the moment maps: a first
 *   pass takes max |q_p| over the bodies, E_p is its frexp exponent, L = ceil(log2(max(n, 1))) for the n bodies of the WHOLE
 *   system, the plane's exponent is 62 - E_p - L (0 when the maximum is 0), a contribution is (int64) rint(ldexp(q_p,
 *   exponent)), added with 64-bit integer atomics.  Plane 5 is the body count.  value = planes * 2^-exponent.  The planes are
 *   a pure function of the set of bodies -- no order, launch shape or number of contexts enters -- and plane 0 summed over the
 *   slots is the sum of w_i = rint(ldexp(m_i, exponent 0)) exactly.
 * bh_radial_profile: both passes and the download.
 * bh_radial_max: the first pass alone, maxabs[p] = max |q_p| over this context's bodies (0 without bodies).
 * bh_radial_deposit: the second pass alone with the caller's exponents (a distributed profile: the MAX of the ranks' maxima
 *   and the SUM of their body counts give every rank the same exponents), the planes left on the device: *planes_dev points
 *   at 6 * (nb + 2) int64, valid until the next radial call or bh_destroy.  Exponents too large for this context's own
 *   maxima and body count are refused.
 * Lagrangian radii.  w_i = rint(ldexp(m_i, e0)), e0 the exponent of plane 0, W = sum w_i; every mass must be >= 0.  For a
 *   fraction f, finite, 0 < f <= 1:  T_f = min(W, max(1, (int64) ceil(f * (double) W)));  R2_f = the smallest r2_i such that
 *   the sum of w_j over r2_j <= r2_i is at least T_f.  r2[f] = R2_f, count[f] = the bodies with r2_i <= R2_f, mass[f] = the
 *   sum of their w_i (bodies tied in r2 are all inside: no index order enters).  Up to BH_RADIAL_MAX_FRACTIONS fractions, in
 *   any order, repeats allowed, results in the caller's order.  W = 0: r2 = NaN, count = mass = 0.  The velocities are not read.
 * bh_lagrangian_radii: the first pass, then a radix select over the bit pattern of r2: 8 rounds of BH_RADIAL_DIGIT_BITS = 8
 *   bits from the top, one pass over the bodies each; between two rounds every fraction picks, on the host, the digit at
 *   which its running sum first reaches T_f.  *exponent = e0.
 * bh_radial_select: one round alone with the caller's e0: the primitive of a distributed selection.  round 0 .. 7; prefixes[np],
 *   1 <= np <= BH_RADIAL_MAX_FRACTIONS, distinct: the 8 * round bits already decided above this round's digit (round 0: the
 *   one prefix 0).  *hist_dev points at np * 256 * 2 int64, hist[k][digit] = {sum w, count} over this context's bodies whose
 *   higher bits equal prefixes[k], valid until the next radial call or bh_destroy.  Summed over the ranks the histograms are
 *   those of the whole system.  An exponent too large for this context's masses and body count is refused.
 * bh_radial_times: HIP-event times of the last of these calls: the first pass; the deposit, or the select rounds together;
 *   rounds_ms[8] (may be NULL): every round of the last bh_lagrangian_radii / bh_radial_select (0 for a round not run).
 * Valid any time after bh_upload / bh_initialize / bh_migrate_unpack, in every precision, in LET mode too (the context's own
 * bodies); they read the state arrays bh_download reads, build no tree and change nothing a step reads: the steps around
 * them run bit for bit as they would have.  They wait for the stream.
 * Errors: BH_ERR_ARG for a null pointer (centre_vel and rounds_ms excepted), a centre or centre velocity that is not finite,
 *   nb < 1 or > BH_RADIAL_MAX_BINS, edges that are not finite, negative or not strictly ascending (they or their squares), nf or
 *   np < 1 or > BH_RADIAL_MAX_FRACTIONS, a fraction that is not finite or outside (0, 1], a round outside 0 .. 7, prefixes that
 *   repeat or have more digits than the round, and -- with a message that says so -- a body whose position, velocity (not the
 *   radii) or mass is not finite or whose r2 or moment overflows fp64, and for the radii a negative mass.  BH_ERR_STATE before
 *   any upload. */
#define BH_RADIAL_MAX_BINS 4096
#define BH_RADIAL_MAX_FRACTIONS 32
#define BH_RADIAL_DIGIT_BITS 8
int bh_radial_profile(bh_ctx *ctx, const double centre[2], const double centre_vel[2], const double *edges, int32_t nb,
                      int64_t *planes, int32_t exponents[5]);
int bh_radial_max(bh_ctx *ctx, const double centre[2], const double centre_vel[2], double maxabs[5]);
int bh_radial_deposit(bh_ctx *ctx, const double centre[2], const double centre_vel[2], const double *edges, int32_t nb,
                      const int32_t exponents[5], void **planes_dev);
int bh_lagrangian_radii(bh_ctx *ctx, const double centre[2], const double *fractions, int32_t nf, double *r2, int64_t *count,
                        int64_t *mass, int32_t *exponent);
int bh_radial_select(bh_ctx *ctx, const double centre[2], int32_t exponent, int32_t round, const uint64_t *prefixes, int32_t np,
                     void **hist_dev);
int bh_radial_times(bh_ctx *ctx, double *max_ms, double *main_ms, double rounds_ms[8]);

/* --- azimuthal Fourier modes: bar strength, phase and pattern speed of a disc ------------------------------------------------
 * What a radial profile loses by construction: A_k(bin) = sum over the bin's bodies of m exp(i k phi), k = 0 .. M, and with
 * rates D_k(bin) = sum m w exp(i k phi), w the angular velocity of the body about the centre.  |A_k| / A_0 is the relative
 * amplitude (k = 2: the bar strength), arg(A_k) / k the phase, Re(D_k / A_k) the instantaneous pattern speed.
 * centre = {cx, cy}; centre_vel = {ucx, ucy} (NULL: 0).  Per body of the CURRENT state, in fp64 in the written order with
 * nothing fused (an fp32 state is widened first, exactly):
 *     dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy
 *     r2 >= 2^-1022:  r = sqrt(r2);  c1 = dx / r;  s1 = dy / r
 *     c_0 = 1;  s_0 = 0;  k = 1 .. M:  c_k = c_{k-1} * c1 - s_{k-1} * s1;  s_k = s_{k-1} * c1 + c_{k-1} * s1
 *     r2 < 2^-1022 (zero or subnormal, no direction):  c_k = s_k = 0 for k >= 1, w = 0
 *     rates:  ux = vx - ucx;  uy = vy - ucy;  b = dx * uy - dy * ux;  w = b / r2;  mw = m * w
 *   The recurrence -- a complex multiplication by (c1 + i s1) -- IS the definition of cos k phi and sin k phi here: no
 *   trigonometric function is called and nothing is renormalised, so the planes are a pure function of the set of bodies.
 * Bins.  edges[nb + 1] under the rules of the radial profiles with BH_MODES_MAX_BINS; the same nb + 2 slots on r2.
 * Planes.  planes[P][nb + 2], plane-major, P = (rates ? 2 : 1) * (1 + 2 M) + 1:
 *     A-planes: m c_0, then m c_k, m s_k for k = 1 .. M;   D-planes (rates only): mw c_0, then mw c_k, mw s_k;   last: the count.
 *   Fixed point of the moment maps with TWO exponents: a first pass runs the same recurrence and takes maxA, the largest
 *   |m c_k| or |m s_k| over all bodies and all k (k = 0 gives |m|), and with rates maxD, the same with mw; exponents[0] = 62 -
 *   E(maxA) - L for the A-planes, exponents[1] likewise from maxD for the D-planes (E the frexp exponent, L = ceil(log2(max(n,
 *   1))) for the n bodies of the WHOLE system, 0 for a zero maximum; exponents[1] = 0 without rates).  A contribution is
 *   (int64) rint(ldexp(q, exponent)), added with 64-bit integer atomics.  value = planes * 2^-exponent.
 * 0 <= M <= BH_MODES_MAX_M; M = 0 is a mass profile.  Without rates the velocities are not read.
 * bh_azimuthal_modes: both passes and the download.
 * bh_modes_max: the first pass alone, maxabs = {maxA, maxD} over this context's bodies (0 without bodies or rates).
 * bh_modes_deposit: the second pass alone with the caller's two exponents (a distributed call: the MAX of the ranks' maxima and
 *   the SUM of their body counts give every rank the same exponents), the planes left on the device: *planes_dev points at
 *   P * (nb + 2) int64, valid until the next modes call or bh_destroy.  Exponents too large for this context's own maxima and
 *   body count are refused.
 * bh_modes_times: HIP-event times of the last of these calls: the first pass, the deposit.
 * Valid whenever the radial calls are: any time after bh_upload / bh_initialize / bh_migrate_unpack, in every precision, in
 * LET mode too (the context's own bodies); they read the state only, build no tree and change nothing a step reads.  They
 * wait for the stream.  The buffers are allocated on the first call.
 * Errors: BH_ERR_ARG for a null pointer (centre_vel excepted), a centre or centre velocity that is not finite, M outside
 *   0 .. BH_MODES_MAX_M, nb < 1 or > BH_MODES_MAX_BINS, bad edges (as the radial calls), and -- found by the first pass, with a
 *   message that says so -- a body whose position, mass, velocity (with rates), r2 or any contribution is not finite (w
 *   overflowing for a tiny r2 included).  Negative masses are allowed.  BH_ERR_STATE before any upload. */
#define BH_MODES_MAX_M 16
#define BH_MODES_MAX_BINS 4096
int bh_azimuthal_modes(bh_ctx *ctx, const double centre[2], const double centre_vel[2], const double *edges, int32_t nb, int32_t M,
                       int32_t rates, int64_t *planes, int32_t exponents[2]);
int bh_modes_max(bh_ctx *ctx, const double centre[2], const double centre_vel[2], int32_t M, int32_t rates, double maxabs[2]);
int bh_modes_deposit(bh_ctx *ctx, const double centre[2], const double centre_vel[2], const double *edges, int32_t nb, int32_t M,
                     int32_t rates, const int32_t exponents[2], void **planes_dev);
int bh_modes_times(bh_ctx *ctx, double *max_ms, double *deposit_ms);

/* --- a disc: initial conditions, the rotation curve of the engine's own forces, velocities about a radial table ---------------
 * Everything below is written down operation by operation in fp64 with nothing fused and goes through no mathematical
 * library beyond the correctly rounded sqrt: a twin in numpy gives the same bits (tests/disc_ref.py).
 * bh_initialize_disc: n bodies of a Kuzmin-Toomre disc, surface density mass * scale / (2 pi (R^2 + scale^2)^(3/2)) cut at
 *   r_max (+inf: no cut), every mass mass / n (one host division), velocities zero.  Body i is a function of (seed, i):
 *     F = 1 - scale / sqrt(r_max^2 + scale^2) on the host (1 without a cut)
 *     stream 96:       u = u01(w0, w1) * F;  t = u * (2 - u);  R = (scale * sqrt(t)) / (1 - u)
 *     stream 128 + k:  p = 2 u01(w0, w1) - 1;  q = 2 u01(w2, w3) - 1;  s = p * p + q * q;  taken when 2^-1022 <= s <= 1, else
 *                      the next stream, 64 at most; the 64th stands whatever its s ((1, 0) when its s < 2^-1022)
 *     x = R * (p / sqrt(s));  y = R * (q / sqrt(s)), rounded to the state type
 *   (u01: the 53-bit uniform of bh_initialize; its streams 0-2 and 16-79 are not used here.)  It fires the events of
 *   bh_initialize: a new body set in caller order, nothing current.  It does not wait for the stream.
 *   Errors: BH_ERR_ARG for n < 0 or n > capacity (the message of bh_initialize), scale not finite or <= 0, r_max not > 0, mass
 *   not finite.
 * bh_rotation_curve: per body of the CURRENT state, with centre = {cx, cy} and (ax, ay) the acceleration in the force buffer
 *   -- widened from fp32, or Fx / m, Fy / m by one division each with an fp64 tree: what bh_get_accel returns --
 *     dx = x - cx;  dy = y - cy;  r2 = dx * dx + dy * dy;  r = sqrt(r2)
 *     q0 = m   q1 = m * r   q2 = m * (dx * ax + dy * ay)   q3 = m * (dx * ay - dy * ax)
 *   summed over the nb + 2 slots of the radial profiles (decided on r2 against the squared edges; a body on an edge belongs to
 *   the bin above it) into planes[5][nb + 2], plane-major: planes 0-3 in the fixed point of the moment maps with
 *   exponents[p] = 62 - E(max |q_p|) - L from a first pass over the whole system, plane 4 the body count.
 *   value = planes * 2^-exponent.  -q2 / q0 of a bin is its squared circular speed, q1 / q0 its mean radius, q3 the torque on it.
 *   nb <= BH_DISC_MAX_BINS.  It needs the forces of the current positions (bh_compute_forces, bh_step_kdk; bh_kick keeps them),
 *   reads the state and the force buffer only and changes nothing a step reads.  It waits for the stream.
 *   Errors: BH_ERR_ARG for a null pointer, a centre that is not finite, nb < 1 or > BH_DISC_MAX_BINS, bad edges (as the radial
 *   calls), and -- found by the first pass -- a body whose position, mass, acceleration, r2 or contribution is not finite (a
 *   massless body with an fp64 tree: 0 / 0).  BH_ERR_STATE before any upload, in LET mode or with world > 1, and when the forces
 *   are not current.
 * bh_set_disc_velocities: the velocity of every body from k ascending radii and three tables over them -- the mean tangential
 *   speed vt and the radial and tangential dispersions --, about centre with the velocity centre_vel = {ucx, ucy} (NULL: 0).
 *   Per body with caller index i (dx, dy, r2 as above):
 *     r2 < 2^-1022:  v = (ucx, ucy)
 *     r = sqrt(r2);  j = the number of radii with radii[.]^2 <= r2
 *     j = 0: f = y[0];  j = k: f = y[k-1];  else t = (r - radii[j-1]) / (radii[j] - radii[j-1]);  f = y[j-1] + t * (y[j] - y[j-1])
 *     g1 = ((int64) sum of the twelve 32-bit words of streams 192 .. 194 of (seed, i)  -  6 (2^32 - 1)) * 2^-32;  g2: 195 .. 197
 *     vr = sr * g1;  vtt = vt + st * g2;  vx = ucx + (vr * dx - vtt * dy) / r;  vy = ucy + (vr * dy + vtt * dx) / r
 *   rounded to the state type.  g is a sum of twelve uniforms (Irwin-Hall): mean 0 exactly, variance 1 - 2^-64, |g| <= 6, exact.
 *   Only the velocities are written: positions, masses, the force buffer and what is current stay, as after bh_kick.  It waits
 *   for the stream.
 *   Errors: BH_ERR_ARG for a null table, a centre or centre velocity that is not finite, k outside 1 .. BH_DISC_MAX_TABLE, radii
 *   (or squares) not finite, negative or not strictly ascending, a table entry that is not finite, a negative dispersion.
 *   BH_ERR_STATE before any upload, in LET mode or with world > 1.
 * bh_disc_times: HIP-event times of the last bh_initialize_disc (it waits for the stream when that has not been read yet), of
 *   the two passes of the last bh_rotation_curve, and of the last bh_set_disc_velocities. */
#define BH_DISC_MAX_BINS 1022
#define BH_DISC_MAX_TABLE 1024
int bh_initialize_disc(bh_ctx *ctx, int64_t n, uint64_t seed, double mass, double scale, double r_max);
int bh_rotation_curve(bh_ctx *ctx, const double centre[2], const double *edges, int32_t nb, int64_t *planes, int32_t exponents[4]);
int bh_set_disc_velocities(bh_ctx *ctx, const double centre[2], const double centre_vel[2], const double *radii, const double *vt,
                           const double *sigma_r, const double *sigma_t, int32_t k, uint64_t seed);
int bh_disc_times(bh_ctx *ctx, double *init_ms, double *curve_max_ms, double *curve_deposit_ms, double *velocities_ms);

/* --- neighbours: which bodies are next to a body or a point, and how far away ------------------------------------------
 * Queries.  points == NULL: the queries are the n bodies in caller order and n_points must be n; body i is left out of its
 *   own answer by index -- another body at the same place is not: it is a neighbour at d2 = 0.  Otherwise points[n_points][2]
 *   are coordinates that are nobody's: a point exactly on a body has that body as a neighbour at d2 = 0.
 * Distance.  For query q and body j of the CURRENT state: dx = x_j - q.x; dy = y_j - q.y; d2 = dx * dx + dy * dy, in fp64 with
 *   nothing fused, in every precision (an fp32 state is widened first, exactly).
 * bh_neighbours: the first k bodies in the total order (d2, caller index j), ascending: idx[n_points][k] their caller indices,
 *   d2[n_points][k] the distances; with fewer than k candidates the remaining slots are idx = -1, d2 = +inf.  Either output
 *   may be NULL, not both.  evals (may be NULL): the number of bodies whose d2 the search computed for the query, seeds
 *   included -- deterministic for a given state and call, a measure of the work and no part of the answer.
 * bh_count_within: counts[n_points] = the bodies with d2 <= radius * radius (the product formed once in fp64 on the host),
 *   the same self-exclusion.
 * A query's result does not depend on the other queries of the call, their order or their number.  The search (a bounding-box
 * hierarchy over the Morton-sorted bodies, rebuilt on every call) prunes with bounds that rounding cannot invert, so the
 * results are those of the brute-force definition above, bit for bit.
 * bh_neighbours_times: HIP-event times of the last of these calls: the structure's build (bounds, sort, boxes) and the
 *   queries (a point launch's own sort included), downloads excluded.
 * They read the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.  They wait for the stream.
 * Errors: BH_ERR_ARG for k < 1 or k > BH_NEIGHBOURS_MAX_K, n_points < 0, a null output, points == NULL with n_points != n, a
 *   non-finite query coordinate (checked before anything is enqueued), a negative or non-finite radius, and -- found by the
 *   bounds pass, with a message that says so -- a non-finite body position in the state.  BH_ERR_CAPACITY for more than 2^24
 *   bodies (their indices share a key word).  BH_ERR_STATE before any upload, in LET mode and with world > 1 (a neighbour can
 *   live on another rank).  n_points = 0 returns at once; without bodies every idx is -1, every d2 +inf, every count 0. */
#define BH_NEIGHBOURS_MAX_K 32
int bh_neighbours(bh_ctx *ctx, const double *points, int64_t n_points, int32_t k, int64_t *idx, double *d2, uint32_t *evals);
int bh_count_within(bh_ctx *ctx, const double *points, int64_t n_points, double radius, uint32_t *counts);
int bh_neighbours_times(bh_ctx *ctx, double *build_ms, double *query_ms);

/* --- neighbour lists: WHICH bodies lie within a radius of a body or a point, every one of them ---------------------------------
 * Queries, distance and self-exclusion: those of bh_count_within above.  points == NULL: the queries are the n bodies in caller
 *   order, n_points must be n, and body i is left out of its own row by index only.  Otherwise points[n_points][2], nobody is
 *   left out, and a point that lies on a body lists that body with d2 = 0.
 * Row r holds the bodies j with d2 <= radius_r * radius_r (the product formed once in fp64 on the host; the edge inclusive),
 *   ascending in the order (d2, caller index j).  radius_r is radii[0] when n_radii == 1, else radii[r]; every radius is finite
 *   and >= 0.
 * Outputs.  offsets[n_points + 1]: the exclusive prefix of the row lengths in caller order, offsets[n_points] = *n_entries.
 *   Row r is idx[offsets[r] .. offsets[r + 1]) -- caller indices -- with the matching d2.  idx and d2 hold max_entries each.
 * Count-only call: idx == NULL and d2 == NULL.  offsets and *n_entries are written and the call returns BH_OK whatever
 *   max_entries is; it costs about a bh_count_within.
 * Too little room: with idx and d2 given and *n_entries > max_entries the call returns BH_ERR_CAPACITY; offsets and *n_entries
 *   are still written (the message carries the number too) and nothing is written to idx or d2.
 * A row depends on its own query only -- not on the other queries of the call, their order or their number -- and equals the
 *   brute-force definition bit for bit in all four precisions (an fp32 state is widened first, exactly).
 * stats (may be NULL): {distances computed by the fill pass, nodes opened by it (summed over the queries), entries, longest
 *   row} -- deterministic for a given state and call, a measure of the work and no part of the answer.  A count-only or refused
 *   call leaves the first two 0.  bh_neighbour_lists_evals: the distances the fill pass of the last call computed, per query.
 * How.  Two traversals of the neighbours' search structure: one counts (taking whole nodes where it can), the row lengths are
 *   scanned to write cursors on the device, one fills; rows are sorted on the device.  The entries of a launch are bounded by
 *   BH_LISTS_ENTRIES (environment, read at bh_create; at least the longest row), BH_LISTS_SORT_LDS is the longest row sorted in
 *   LDS alone.  Should the two traversals ever disagree, the call fails with BH_ERR_DEVICE and says how; it never writes past a row.
 * bh_neighbour_lists_times: HIP-event times of the last call: the structure's build, the count pass (a point launch's own sort
 *   included), scan and fill, and the row sorts; downloads excluded.
 * It reads the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.  It waits for the stream.  Its buffers only grow; bh_destroy frees them.
 * Errors: BH_ERR_ARG for a negative or non-finite radius (checked before anything is enqueued), n_radii not 1 or n_points,
 *   n_points < 0, null offsets, n_entries or radii, exactly one of idx and d2 null, max_entries < 0, points == NULL with
 *   n_points != n, a non-finite point, and -- found by the bounds pass, with a message that says so -- a non-finite body
 *   position.  BH_ERR_CAPACITY for more than 2^24 bodies.  BH_ERR_STATE before any upload, in LET mode and with world > 1.
 *   n_points = 0 gives offsets[0] = 0 and *n_entries = 0; without bodies every row is empty. */
int bh_neighbour_lists(bh_ctx *ctx, const double *points, int64_t n_points,
                       const double *radii, int64_t n_radii,          /* 1, or n_points */
                       int64_t max_entries, int64_t *offsets /* n_points + 1 */,
                       int64_t *idx, double *d2,                      /* max_entries each, or both NULL */
                       int64_t *n_entries, uint64_t stats[4]);
int bh_neighbour_lists_times(bh_ctx *ctx, double *build_ms, double *count_ms, double *fill_ms, double *sort_ms);
int bh_neighbour_lists_evals(bh_ctx *ctx, int64_t n_points, uint32_t *evals);

/* --- pair counts: how many pairs lie at each separation (DD(r), the raw material of the two-point correlation) ----------------
 * Distance.  For a body j and a query q of the CURRENT state: dx = x_j - q.x; dy = y_j - q.y; d2 = dx * dx + dy * dy, in fp64
 *   with nothing fused, in every precision (an fp32 state is widened first, exactly): the d2 of bh_count_within.  It is
 *   symmetric in (i, j), bit for bit.
 * Edges.  edges[nb + 1] must be finite, >= 0 and strictly ascending, 1 <= nb <= BH_PAIR_MAX_BINS.  e2_k = edges[k] * edges[k]
 *   is formed once in fp64 on the host; the e2 must be finite and strictly ascending too.
 * Bins.  counts[nb + 2]: counts[0] ("below") the pairs with d2 <= e2_0; counts[k + 1] those with e2_k < d2 <= e2_{k+1};
 *   counts[nb + 1] ("beyond") those with d2 > e2_nb -- the bin index is the number of e2_k < d2.  The upper edge is inclusive,
 *   as in bh_count_within and bh_groups, so coincident distinct bodies (d2 = 0) are always "below", even with edges[0] = 0.
 * Auto mode (points == NULL, n_points must be n): every unordered pair i != j of the n bodies is counted exactly once; the
 *   counts sum to n (n - 1) / 2.
 * Cross mode (points[n_points][2], finite coordinates that are nobody's): every (point, body) combination is counted once,
 *   nobody is left out; the counts sum to n_points * n.  A point on a body gives d2 = 0, which is "below".
 * evals (may be NULL): the number of d2 the call computed -- deterministic for a given state and call, a measure of the work
 *   and no part of the answer.  The search (the index of the neighbour queries, rebuilt on every call) takes a node whole when
 *   both of its distance bounds fall in one bin; rounding cannot invert the bounds, so the counts are those of the brute-force
 *   definition above, bit for bit.
 * bh_pair_counts_times: HIP-event times of the last bh_pair_counts: the structure's build (bounds, sort, boxes) and the
 *   traversals (a point launch's own sort included), the download excluded.
 * It reads the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.  It waits for the stream.
 * Unlike bh_count_within it is allowed in LET mode and with world > 1: it then counts THIS CONTEXT'S OWN bodies (all of the
 *   bodies this context holds); the pairs across ranks are the caller's to add, as cross counts of another rank's positions.
 * Errors: BH_ERR_ARG for nb or edges outside the rules above, a null edges or counts, n_points < 0, points == NULL with
 *   n_points != n, a non-finite point (checked before anything is enqueued), and -- found by the bounds pass, with a message
 *   that says so -- a non-finite body position in the state.  BH_ERR_STATE before any upload.  BH_ERR_CAPACITY for more than
 *   2^24 bodies.  With n = 0 or n_points = 0 all counts are zero; n = 1 in auto mode gives all zeros. */
#define BH_PAIR_MAX_BINS 1024
int bh_pair_counts(bh_ctx *ctx, const double *points, int64_t n_points, const double *edges, int32_t nb, int64_t *counts,
                   int64_t *evals);
int bh_pair_counts_times(bh_ctx *ctx, double *build_ms, double *query_ms);

/* --- groups: which bodies belong together (friends of friends), and a catalogue of the groups ---------------------------------
 * Distance.  For bodies i != j of the CURRENT state: dx = x_j - x_i; dy = y_j - y_i; d2 = dx * dx + dy * dy, in fp64 with nothing
 *   fused, in every precision (an fp32 state is widened first, exactly): the d2 of bh_count_within.  It is symmetric in (i, j).
 * Friends.  i and j are friends when d2 <= b2, b2 = linking_length * linking_length (the product formed once in fp64 on the host).
 * Groups.  A group is a connected component of the friendship graph over all n bodies; a body without friends is a group of one.
 * Label.  label[i] (n of them, caller order; may be NULL) is the smallest caller index in the group of body i.  The labels are a
 *   pure function of the state and the linking length: no launch shape, traversal order or race decides any of them.
 * Catalogue.  Every group with at least min_members (>= 1) bodies has a record: its label, its member count and the five sums
 *     plane 0: m      plane 1: m * x      plane 2: m * y      plane 3: m * vx      plane 4: m * vy
 *   over its members, each moment one fp64 product, summed in the fixed point of the moment maps: a first pass takes max |q_p|
 *   of every plane over ALL bodies, E_p is its frexp exponent, L = ceil(log2(max(n, 1))), the plane's exponent is 62 - E_p - L
 *   (0 when the maximum is 0), a contribution is (int64) rint(ldexp(q_p, exponent)), added with 64-bit integer atomics: no
 *   overflow, the same bits in any order, every contribution rounded once by at most half a unit.  value = sum * 2^-exponent.
 *   The records are ordered by (count descending, label ascending).
 * bh_groups: builds the index of the neighbour queries, links, labels and reduces; waits for the stream.  *n_groups: all
 *   components, whatever min_members.  n_catalogue may be NULL: then no catalogue is made (and masses and velocities are not
 *   read); else *n_catalogue is the number of records.  stats (may be NULL) = {distances computed, friend pairs found, unions
 *   that joined two trees}: deterministic for a given state and call; the third is n - *n_groups; a measure of the work and no
 *   part of the answer.
 * bh_groups_catalogue: copies out the catalogue of the last bh_groups call -- that call's result, valid until the next bh_groups
 *   or bh_destroy whatever the run does in between.  labels[g], counts[g], sums[g][5], exponents[5]; any of them may be NULL.
 *   *n_out receives the number of records even when max_records is too small (then BH_ERR_CAPACITY and nothing else is copied
 *   but the exponents).
 * bh_groups_times: HIP-event times of the last bh_groups: the index's build; init, link, flatten and label; the catalogue.
 * They read the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.
 * Errors: BH_ERR_ARG for a negative or non-finite linking length, min_members < 1, a null n_groups, and -- found by the bounds
 *   pass, with a message that says so -- a non-finite body position; with a catalogue also for a non-finite mass or velocity (or
 *   a moment that overflows fp64).  BH_ERR_CAPACITY for more than 2^24 bodies.  BH_ERR_STATE before any upload, in LET mode and
 *   with world > 1 (a group can span ranks).  Without bodies *n_groups = 0 and the catalogue is empty. */
int bh_groups(bh_ctx *ctx, double linking_length, int64_t min_members, int64_t *label, int64_t *n_groups, int64_t *n_catalogue,
              uint64_t stats[3]);
int bh_groups_catalogue(bh_ctx *ctx, int64_t max_records, int64_t *labels, int64_t *counts, int64_t *sums, int32_t exponents[5],
                        int64_t *n_out);
int bh_groups_times(bh_ctx *ctx, double *build_ms, double *link_ms, double *catalogue_ms);

/* --- spanning trees: the clustering at every linking length at once, and the trees of small subsets ------------------------------
 * Distance.  d2(i, j) is the d2 of bh_count_within and bh_groups: dx = x_j - x_i; dy = y_j - y_i; d2 = dx * dx + dy * dy, in fp64
 *   with nothing fused, in every precision (an fp32 state is widened first, exactly).  It is symmetric in (i, j), bit for bit.
 * Edge order.  The edges of the complete graph over the bodies are ordered by the triple (d2, lo, hi), lo < hi the CALLER indices
 *   of the two ends.  That is a strict total order, so the minimum spanning tree is UNIQUE -- with coincident bodies and on a
 *   lattice too: there is exactly one right answer, and no launch shape, traversal order or race decides any of it.
 * bh_spanning_tree: the n - 1 edges of that tree over all bodies of the current state (none for n <= 1) as lo[], hi[], d2[], each
 *   with room for n - 1 entries, ASCENDING in the edge order.  The friends-of-friends groups of bh_groups at linking length b are
 *   the connected components of the edges with d2 <= b * b, and their number is n minus the number of such edges.  It builds the
 *   index of the neighbour queries, runs Boruvka rounds on it (at most ceil(log2 n); BH_ERR_DEVICE with a message should 25 not
 *   do) and sorts the edges by d2 on the device (the host orders edges of equal d2); it waits for the stream.
 *   stats (may be NULL) = {rounds, distances computed, nodes skipped because all their bodies lay in the lane's own component,
 *   edges (= n - 1)}: deterministic for a given state; a measure of the work and no part of the answer.
 * bh_spanning_tree_subsets: for each of n_sets rows of k caller indices in members[n_sets][k], the k - 1 edges of the minimum
 *   spanning tree of THOSE k BODIES ALONE under the same edge order, into row r of lo, hi, d2 ([n_sets][k - 1]), each row
 *   ascending.  2 <= k <= BH_MST_SUBSET_MAX, n_sets >= 0.  One wavefront per row (Prim's algorithm in LDS); rows may share
 *   bodies.  It reads the positions of the members only.
 * bh_spanning_tree_times: of the last of the two calls.  bh_spanning_tree: HIP-event times of the index's build, of the rounds
 *   and of the final sort (the host's ordering of equal d2 added).  bh_spanning_tree_subsets: 0, the HIP-event time of the
 *   kernels, and the host's time for sorting the rows.
 * They read the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.
 * Errors: BH_ERR_ARG for a null lo, hi or d2 (bh_spanning_tree_subsets: with n_sets > 0, members too), for k or n_sets outside
 *   the rules above, for an index outside [0, n) or an index twice in one row (checked on the host before anything is
 *   enqueued), and for a non-finite body position (bh_spanning_tree: found by the bounds pass, with a message that says so;
 *   bh_spanning_tree_subsets: of a member).  BH_ERR_CAPACITY for more than 2^24 bodies.  BH_ERR_STATE before any upload, in LET
 *   mode and with world > 1 (the tree spans ranks). */
#define BH_MST_SUBSET_MAX 512
int bh_spanning_tree(bh_ctx *ctx, int64_t *lo, int64_t *hi, double *d2, uint64_t stats[4]);
int bh_spanning_tree_subsets(bh_ctx *ctx, const int64_t *members, int64_t n_sets, int32_t k, int64_t *lo, int64_t *hi, double *d2);
int bh_spanning_tree_times(bh_ctx *ctx, double *build_ms, double *rounds_ms, double *sort_ms);

/* --- binaries: which bodies are bound pairs, and a catalogue of their Keplerian elements -----------------------------------------
 * Energy.  For bodies i != j of the CURRENT state, in fp64 with nothing fused, sqrt and / correctly rounded, in every precision
 *   (an fp32 state is widened first, exactly), G the context's:
 *     dx = x_j - x_i; dy = y_j - y_i; d2 = dx * dx + dy * dy                     (the d2 of bh_count_within)
 *     ux = vx_j - vx_i; uy = vy_j - vy_i; v2 = ux * ux + uy * uy
 *     M = m_i + m_j;  eps_ij = 0.5 * v2 - (G * M) / sqrt(d2)                     (two-body energy per unit reduced mass)
 *   eps_ij and eps_ji are the same bits.  The softening of the configuration does NOT enter: the elements are Keplerian.  The
 *   state is read as it is: after bh_step the velocities lie half a step from the positions; synchronised elements want the
 *   state of bh_step_kdk.
 * Candidates of i, for max_separation R (R2 = R * R, formed once on the host): all j != i with 0 < d2 <= R2 and eps_ij < 0.  The
 *   upper edge is inclusive, as in bh_count_within; coincident bodies are never candidates of each other.  A NaN velocity or
 *   mass follows the formulas: every comparison is false, such a body is nobody's candidate and has none.
 * Partner.  partner[i] (n of them, caller order; may be NULL) is the candidate first in the strict total order (eps_ij, caller
 *   index j), with eps[i] = that eps_ij (may be NULL); -1 with eps = +inf when there is no candidate.  A pure function of the
 *   state and R: no launch shape, traversal order or race decides any of it.
 * Binary.  A pair lo < hi (caller indices) with partner[lo] == hi and partner[hi] == lo.  The catalogue lists them ASCENDING in lo;
 *   record k is lo[k], hi[k] and records[k][11], computed on the device in this order with i = lo, j = hi:
 *     mu = G * M;  r = sqrt(d2);  eps as above
 *     a = mu / (-2.0 * eps)                                                       semi-major axis
 *     h = dx * uy - dy * ux
 *     e = sqrt(max(1.0 + ((2.0 * eps) * (h * h)) / (mu * mu), 0.0))               eccentricity (max(x, 0) is x > 0 ? x : 0)
 *     period = 6.283185307179586 * sqrt(((a * a) * a) / mu)
 *     binding = -(((m_i * m_j) / M) * eps)                                        > 0
 *     com = ((m_i * x_i + m_j * x_j) / M, same in y);  velocity likewise
 *   records[k] = {r, eps, a, e, period, binding, M, com x, com y, velocity x, velocity y}.
 * bh_binaries: builds the index of the neighbour queries and, beside it, the sorted velocities and masses and the largest mass
 *   under every node; searches (a lane drops a node only on a lower bound of its distances or of its energies that rounding
 *   cannot invert: DESIGN.md section 27); finds the mutual pairs and their elements; waits for the stream.  R must be > 0 and not
 *   NaN; +inf means no cut -- a body that is bound to nobody then searches every body.  *n_pairs: the records of the catalogue.
 *   stats (may be NULL) = {energies computed, the most by one body, nodes opened, pairs}: deterministic for a given state and
 *   call; a measure of the work and no part of the answer.
 * bh_binaries_catalogue: copies out the catalogue of the last bh_binaries call -- that call's result, valid until the next
 *   bh_binaries or bh_destroy whatever the run does in between.  lo[g], hi[g], records[g][11]; any of them may be NULL.  With
 *   max_records below the *n_pairs of that call: BH_ERR_CAPACITY and nothing is copied.
 * bh_binaries_times: HIP-event times of the last bh_binaries: the index's build with the sorted copies and mass bounds; the
 *   search; the pairs and their elements (the host's ordering of the records added).
 * They read the state only: no force tree is built, nothing a step, bh_stats or another diagnostic reads is touched, and a
 * following bh_step is bit for bit what it would have been.
 * Errors: BH_ERR_ARG for R <= 0 or NaN, G <= 0, a null n_pairs, max_records < 0 and -- found by the bounds pass, with a message
 *   that says so -- a non-finite body position.  BH_ERR_CAPACITY for more than 2^24 bodies.  BH_ERR_STATE before any upload, in LET
 *   mode and with world > 1 (a pair can span ranks).  Without bodies *n_pairs = 0 and the catalogue is empty. */
int bh_binaries(bh_ctx *ctx, double max_separation, int64_t *partner, double *eps, int64_t *n_pairs, uint64_t stats[4]);
int bh_binaries_catalogue(bh_ctx *ctx, int64_t max_records, int64_t *lo, int64_t *hi, double *records /* n x 11 */);
int bh_binaries_times(bh_ctx *ctx, double *build_ms, double *search_ms, double *catalogue_ms);

/* --- tree output ------------------------------------------------------------------------
 * bh_export_tree: the tree of the last bh_build_tree/bh_compute_forces/bh_step in DFS
 * pre-order with children in index order -- the visiting order of TraverseTreeToFile
 * (project.cu:504-534).  depth may be NULL.  *n_nodes receives the node count even when cap
 * is too small (then BH_ERR_CAPACITY).
 * bh_write_quadtree_file: TraverseTreeToFile itself (same text format, project.cu:509-526);
 * for occupant indices <= -2, where the reference reads out of bounds, the body's true
 * position is printed. */
int bh_export_tree(bh_ctx *ctx, bh_tree_node *nodes, int32_t *depth, int64_t cap,
                   int64_t *n_nodes);
int bh_write_quadtree_file(bh_ctx *ctx, const char *path);

/* --- measurement (replaces the std::chrono timers of project.cu:985-1007) ----------------*/
int bh_stats(bh_ctx *ctx, bh_stats_t *out);
/* Per step of the last bh_step call (at most 4,096 of them): step_ms[s] = end of step s-1's walk (or the start of
 * the call) to the end of step s's walk, walk_ms[s] = that step's walk + integrate kernel -- HIP events on the
 * context's stream.  The reference accumulates one total per run (project.cu:985-1007); a spread needs the steps.
 * *n_out receives the number of steps available even when cap is too small; step_ms / walk_ms may be NULL. */
int bh_step_times(bh_ctx *ctx, double *step_ms, double *walk_ms, int32_t cap, int32_t *n_out);
/* What the sort of the most recent tree build (of a step, bh_build_tree, or a diagnostic's quiet build) was given, decided and
 * wrote -- for tests of the bucket sort's direct input.  Waits for the stream, then plain copies: no
 * launch, nothing a step or bh_stats reads is touched, a following bh_step is bit for bit what it would have been.
 * info = {offered, n, nb, L, T, room of one list, lists, counter words that follow word 0 (64)}: offered = 1 when direct input was
 *   offered to that build (the device then decided per its counters); n bodies in nb buckets, bucket b the range [b L, (b + 1) L).
 * Every array may be NULL.  keys_sorted[n], perm[n]: the sort's output as the later kernels read it (a build that was offered
 *   direct input: the 40 key bits, and the slot each came from).  Only when offered = 1, untouched otherwise:
 *   decision[65]: word 0 (non-zero: the counting pass was ordered outright) and the 64 list counters of the block that build
 *     counted into; range_keys[nb]; list[lists * room]: list s at s * room; keys_in[n]: the packed keys in state order,
 *     key | slot << 40, as keys_kernel left them.
 * Call it with NULL arrays first to learn the sizes.
 * Errors: BH_ERR_STATE without a valid tree (before the first build, after bh_upload, bh_drift, bh_migrate_pack) and in LET mode,
 *   where bh_migrate_pack reuses the buffers. */
int bh_sort_snapshot(bh_ctx *ctx, int64_t info[8], uint32_t *decision, uint64_t *range_keys, uint64_t *list, uint64_t *keys_in,
                     uint64_t *keys_sorted, uint32_t *perm);

/* How the buckets of the bucket sort's in-LDS sort ended, cumulative since bh_create:
 * out[0] buckets finished by placement -- nearly ordered input, every key written straight to its rank, no byte pass; tried
 *   for single-bucket launches and for the ranges of a direct build in which no body changed bucket
 *   (BH_SORT_PLACE=0 at bh_create turns that path off: out[0] stays 0);
 * out[1] buckets that went through byte passes (those counted in bh_stats_t.sort_rerun_buckets among them).
 * A bucket of equal keys with placement off, and a bucket sorted through memory (sort_spill_buckets), count in neither.
 * Waits for the stream; no launch. */
int bh_sort_paths(bh_ctx *ctx, uint64_t out[2]);

/* --- multi-GPU plumbing -----------------------------------------------------------------
 * The reference is single-GPU.  One process per GPU owns a contiguous range [lo, hi) of
 * the sorted (space-filling-curve order) bodies: bh_step then walks and integrates only that range, and the
 * host exchanges the updated ranges (torch.distributed all_gather over RCCL) through the
 * device pointers below.  The exchange buffers stay valid until bh_destroy; element types follow
 * the context's precision (double2/double or float2/float).  bh_device_state exposes the state
 * arrays as the device holds them: in exact mode that is the caller's order; in fp32 / mixed mode
 * the engine re-orders the bodies into sorted order every 16th tree build (so that its gathers
 * stay local) and swaps buffers when it does -- ask again after stepping, and use bh_download for
 * the caller's order. */
int bh_set_owned_fraction(bh_ctx *ctx, int32_t rank, int32_t world);
int bh_device_state(bh_ctx *ctx, void **pos, void **vel, void **mass, int64_t *n,
                    int32_t *elem_bytes);
int bh_owned_range(bh_ctx *ctx, int64_t *lo, int64_t *hi);
/* Sorted-order view used by the exchange: ONE buffer of {x, y, vx, vy} (4 floats) per sorted body.
 * After bh_step_local the owned slice holds the new state; after ONE all_gather of the slices
 * bh_scatter_sorted writes the whole buffer back to caller order. */
int bh_step_local(bh_ctx *ctx);
int bh_device_sorted(bh_ctx *ctx, void **sorted_state);
int bh_scatter_sorted(bh_ctx *ctx);
/* Distributed step with locally-essential trees (LET).  Unlike the replicated scheme above, a
 * context in LET mode holds ONLY ITS OWN bodies (bh_upload its subset; a contiguous range of a
 * space-filling-curve order of the bodies keeps the exchanged trees small).  Per step:
 *   bh_let_bounds   -> B = boxes_per_rank bounding boxes of consecutive slices of the local bodies
 *                      in a device buffer (B x 4 doubles: xmin, xmax, ymin, ymax; unpadded)
 *   [host: all_gather the W x B x 4 doubles into the all_bounds buffer]
 *   bh_let_build    -> global root box, local tree under it, and for every peer a compact LET
 *                      (the quads that some body inside one of the peer's boxes can open) packed
 *                      in the send buffer, W fixed-size blocks of let_cap quads, child links
 *                      already expressed in the receiver's index space
 *   [host: all_to_all of the blocks, send buffer -> recv buffer]
 *   bh_let_walk     -> every local body walks its own tree and the W-1 received LETs, integrate
 * bh_let_pointers exposes the device buffers for the two collectives; block_bytes is the size of
 * one per-peer block (the pointers change when let_cap does).  bh_let_counts waits for the stream and
 * returns, per peer, the LARGEST LET of any build since the previous bh_let_counts (or
 * bh_let_configure), and whether any of those builds overflowed: with overflow == NULL it fails with
 * BH_ERR_CAPACITY if one exceeded let_cap, otherwise it reports that in *overflow and returns BH_OK.
 * The flag is sticky over the interval (a check every N steps sees an overflow of ANY step in
 * between) and is also raised when the LOCAL tree outgrew node_capacity, because the send blocks are
 * then left as they were; reading the counters starts a new interval.  An overflowing LET is
 * truncated safely (links past the block are cut), so the step completes but its forces are wrong:
 * check the counts before trusting a run.  bh_let_configure may be called again with the same
 * rank/world and a new let_cap (size the blocks from measured counts).  bh_let_forces =
 * bh_let_walk without the integration.  fp32 and mixed precision. */
/* forest_base: where the received blocks start in a context's quad array.  A sender writes the child
 * links of a LET in the RECEIVER's index space, so this must be ONE number on all ranks: the largest
 * bh_let_local_quads of any rank (all_reduce MAX it once; contexts of equal capacity agree anyway). */
int bh_let_local_quads(bh_ctx *ctx, int64_t *local_quads);
int bh_let_configure(bh_ctx *ctx, int32_t rank, int32_t world, int64_t let_cap, int64_t forest_base);
int bh_let_bounds(bh_ctx *ctx);
int bh_let_pointers(bh_ctx *ctx, void **lbounds, void **all_bounds, void **send, void **recv,
                    int64_t *block_bytes, int32_t *boxes_per_rank);
int bh_let_build(bh_ctx *ctx);
int bh_let_walk(bh_ctx *ctx);
int bh_let_forces(bh_ctx *ctx);
/* bh_let_walk in two launches, so that the all_to_all can overlap the first: bh_let_walk_local walks
 * the local tree only (needs bh_let_build, not the received blocks); bh_let_walk_remote adds the
 * received LETs and finishes the step (integrate != 0) or only the forces.  Same sums in the same
 * order as bh_let_walk when the launch runs one wavefront per 64 bodies. */
int bh_let_walk_local(bh_ctx *ctx);
int bh_let_walk_remote(bh_ctx *ctx, int32_t integrate);
int bh_let_counts(bh_ctx *ctx, uint32_t *counts, int32_t *overflow);
/* --- diagnostics of the distributed step: potential and energy sums of a rank ---------------------
 * The single-context diagnostics above refuse a context in LET mode; these are their forest forms (fp32 and mixed
 * precision, as LET mode itself).  No rank ever holds more than its own bodies: a rank computes the potential of ITS
 * bodies over the forest it holds, and its share of the eight sums; the host combines the ranks' shares.
 * bh_let_potential: phi_i = -G sum M / d over exactly the terms the forest force walk takes for body i -- the own tree
 *   from quad 0 (fp32 acceptance, own depth-cap buckets body by body, a body at d2 == 0 gives nothing), then the
 *   received LET of every peer in rank order, the own rank skipped (remote buckets are aggregates) -- with the fp32
 *   walk's term m * rsq(d2) in fp32, summed per body in fp64 in that fixed order: two calls on the same forest return
 *   the same bits.  It walks the forest of the last bh_let_build, completed by the caller with the peers' blocks: the
 *   preconditions of bh_let_forces.  BH_ERR_STATE outside LET mode (so in every precision without LET), before
 *   bh_let_build, and when an integrating walk has moved the bodies since that build.  One wavefront per 64 bodies in
 *   one launch, whatever shape the force walk takes.  It writes the potential and its own term counts only: forces,
 *   interaction counts, group costs (the ORB weights), the bounds records, bh_stats' walk counters and the timings stay
 *   the last force walk's.  A truncated block (bh_let_counts reports the overflow) is walked as safely as the force
 *   walk walks it -- links past the block are cut -- and is as wrong.  The buffers are allocated on first use
 *   (bh_stats.device_bytes grows then, not before).
 * bh_let_get_potential: phi[n_local] (per unit mass) and, if counts != NULL, the terms summed per body -- equal to the
 *   forest force walk's bh_get_interaction_counts -- in the rank's caller order (the order of bh_download / bh_get_ids).
 *   BH_ERR_STATE unless a bh_let_potential of the current state exists: the potential stops being current at
 *   bh_let_walk, bh_let_walk_remote with integrate, bh_upload, bh_initialize and bh_migrate_unpack.
 * bh_let_energy: runs bh_let_potential unless the potential is current, then this rank's share of
 *   sums[8] = sum m, sum m x, sum m y, sum m vx, sum m vy, sum m (x vy - y vx), sum m |v|^2, sum m phi
 *   by the deterministic two-pass reduction of bh_energy -- RAW sums, nothing halved or divided: the caller adds the
 *   ranks' shares (in a fixed order, compensated, if every rank is to get the same bits) and only then forms
 *   kinetic = 1/2 sum m |v|^2, potential = 1/2 sum m phi, com = sum m x / sum m.  A rank without bodies returns zeros.
 * bh_let_bounds_quiet / bh_let_build_quiet: bh_let_bounds and bh_let_build for a diagnostic between two steps -- same
 *   boxes, tree, LETs and LET size counters, but everything a later step reads from an earlier one is put back: the
 *   walk's bounds records stay for the next bh_let_bounds, the state is never re-ordered, the build count (re-order
 *   cadence) and the sort's sample state are restored, bh_stats' walk counters and bh_let_build timings are left alone,
 *   and bh_orb_histogram keeps weighting every body by the cost of its group in the last FORCE walk.  The steps that
 *   follow compute bit for bit the trajectory they would have computed without the diagnostic. */
int bh_let_bounds_quiet(bh_ctx *ctx);
int bh_let_build_quiet(bh_ctx *ctx);
int bh_let_potential(bh_ctx *ctx);
int bh_let_get_potential(bh_ctx *ctx, double *phi, uint32_t *counts);
int bh_let_energy(bh_ctx *ctx, double sums[8]);
/* --- device-side body migration and re-balancing for the LET scheme -------
 * The reference is single-GPU (project.cu:918-1024 keeps every body on one device); this is new design.
 * Ownership is defined by an orthogonal-recursive-bisection cut tree over the global root box: the node
 * that splits the ranks [r0, r0 + nr) (nr > 1) into nl = nr / 2 and nr - nl sends a body with
 * coordinate[axis] < value to the left.  Cuts are stored in pre-order: the left subtree's cuts follow
 * their parent directly (nl - 1 of them), the right subtree's come after those.
 *   bh_orb_histogram : for every region of depth `level` of the cut tree (cuts above it already fixed),
 *                      a histogram of this rank's bodies over BH_ORB_BINS bins across the ROOT box along
 *                      the region's axis (bin edges = depth-12 lines of the tree grid, so a cut taken
 *                      from it is a grid line), each body weighted by the cost of its 64-body group in the
 *                      last walk (1 before the first walk).  *hist = device pointer to n_cuts x
 *                      BH_ORB_BINS uint64 (row k = the region whose cut is k): the caller all-reduces it.
 *   bh_migrate_pack  : classify every local body by the cut tree, group the bodies by destination rank
 *                      (stable) into the send buffer -- 6 doubles per body: x, y, vx, vy, mass, id -- and
 *                      return the W counts (host; waits for the stream).
 *   [host: all_to_all of the counts, then ONE all_to_all of the records on the device pointers of
 *    bh_migrate_pointers with those splits; a rank's own group travels with the rest]
 *   bh_migrate_unpack: the received records become the local state (n_new bodies, arrival order =
 *                      caller order from here on); the tree is invalid until the next build.
 * bh_set_ids / bh_get_ids: a 64-bit identifier per body in caller order (default: the upload index);
 * it travels with the body. */
#define BH_ORB_BINS 4096
#define BH_ORB_MAX_CUTS 63
typedef struct bh_orb_cuts {
    int32_t world, n_cuts;           /* n_cuts = world - 1                                       */
    double  box[4];                  /* global root box: xmin, xmax, ymin, ymax                  */
    int32_t axis[BH_ORB_MAX_CUTS];   /* 0 = x, 1 = y                                             */
    int32_t pad;
    double  value[BH_ORB_MAX_CUTS];
} bh_orb_cuts;
int bh_set_ids(bh_ctx *ctx, const int64_t *ids);
int bh_get_ids(bh_ctx *ctx, int64_t *ids);
int bh_orb_histogram(bh_ctx *ctx, const bh_orb_cuts *cuts, int32_t level, void **hist, int64_t *n_words);
int bh_migrate_pack(bh_ctx *ctx, const bh_orb_cuts *cuts, int64_t *send_counts);
int bh_migrate_pointers(bh_ctx *ctx, void **send, void **recv, int64_t *capacity_records);
int bh_migrate_unpack(bh_ctx *ctx, int64_t n_new);
/* Run on an external HIP stream (e.g. torch's current stream), passed as void*. */
int bh_set_stream(bh_ctx *ctx, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* BHGPU_H */
