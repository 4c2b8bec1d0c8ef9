// bh_engine.hip -- libbhgpu.so: the C-ABI of include/bhgpu.h.  In this file: the context and its helpers, the tree build, the
// walks' launchers, the step and the split operators, the diagnostics, direct sums and force check, tree export, the
// locally-essential trees and migration, and of the disc what writes the state (initial conditions, velocities).  The analysis
// queries' host code -- moment maps, radial profiles, azimuthal modes, the rotation curve, field at points, neighbours, pair counts,
// groups, spanning trees -- is bh_queries_host.hpp, included below as part of this unit.
// Compiled with -ffp-contract=off (tree build + exact walk must not fuse multiply-adds; the fp32
// walk lives in bh_walk_fast.hip, compiled separately).  gfx950 only, no CPU fallback.
#include "../../include/bhgpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "bh_tree.hpp"
#include "bh_walk_exact.hpp"
#include "bh_walk_f64.hpp"
#include "bh_diag.hpp"
#include "bh_direct.hpp"
#include "bh_field.hpp"
#include "bh_init.hpp"
#include "bh_let.hpp"
#include "bh_migrate.hpp"
#include "bh_split.hpp"
#include "bh_moments.hpp"
#include "bh_radial.hpp"
#include "bh_modes.hpp"
#include "bh_disc.hpp"
#include "bh_neighbours.hpp"
#include "bh_neighbour_lists.hpp"
#include "bh_pairs.hpp"
#include "bh_groups.hpp"
#include "bh_mst.hpp"
#include "bh_binaries.hpp"
#include "bh_walk_fast.h"
#include "bh_run_state.hpp"
#include "bh_queries_state.hpp"

using namespace bh;

// The one place the product translation unit knows about A/B builds: -DBHGPU_EXPERIMENTS (scripts/build_variants.sh) swaps the
// empty hook object for scripts/experiments/bh_engine_hooks.hpp (the per-wave timeline and clock stamps of the walk).
#ifdef BHGPU_EXPERIMENTS
#include "../../scripts/experiments/bh_engine_hooks.hpp"
#else
struct ExpHooks {
    hipError_t create(int64_t) { return hipSuccess; }
    void walk_args(WalkFastArgs &) const {}
    void destroy(int64_t) {}
};
#endif

static thread_local std::string g_create_error;

struct bh_ctx : RunState {   // (is / carry / last and their events: bh_run_state.hpp)
    bh_config cfg{};
    int Dm = 0;
    // cfg.precision: BH_PRECISION_F64_EXACT, BH_PRECISION_F64 (the exact mode's tree and state, the throughput walk of
    // bh_walk_f64.hpp), BH_PRECISION_MIXED, BH_PRECISION_F32
    enum class Mode { Exact, F64, Mixed, F32 };
    Mode mode = Mode::Exact;
    // fp64 NodeD / LinkD tree, fp64 forces, state in caller order (else: QuadF tree, accelerations, device order)
    bool tree64() const { return mode == Mode::Exact || mode == Mode::F64; }
    bool state64() const { return mode != Mode::F32; }    // fp64 state arrays
    bool compat = true;
    // Plummer softening (bh_set_softening; 0 = none, and always 0 in Mode::Exact): the length, its square for the fp64
    // kernels, and (float)eps2 for the fp32 walks -- 0.f there selects the unsoftened kernels
    double eps = 0.0, eps2 = 0.0;
    float eps2f = 0.f;
    bool exact_thresholds = false; // Mode::Exact: nodes carry exact d2 thresholds for the walk's acceptance test (off: BH_FLAG_WALK_PORTABLE)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0;
    int64_t internal_cap = 0, node_cap = 0;
    int64_t bfs_max = 12288;       // bit-exact walk: one wavefront per body (walk_exact_bfs_kernel) for launches up to here (BH_EXACT_BFS_MAX;
                                   // walk ms against the cooperative walk: 0.021 / 0.072 at N = 1,024, 0.042 / 0.108 at 4,096, 0.126 / 0.223
                                   // at 8,192, 0.180 / 0.221 at 12,288, 0.241 / 0.212 at 16,384)
    int exact_bpw = 0;             // BH_EXACT_BPW: bodies per wavefront in the fp64 walks (0 = by launch size; 64 = rounds 1-3)
    int walk_split = 0;            // 0 = automatic
    bool walk_asm = true;          // BH_WALK_ASM=0: the C++ loop everywhere (A/B)
    int sort_bucket = 1;           // 1: bucket sort when the previous build's sorted positions are this body set's
                                   // (BH_SORT_BUCKET=0: always the LSD passes; 2: always the bucket sort, tests)
    uint64_t *splitters = nullptr;
    uint16_t *sort_dig = nullptr;  // bucket of every key (written by the histogram, read by the scatter)
    // direct input of the bucket sort (bh_sort.hpp; fp32-tree builds): 1 = when at most sort_direct_max bodies changed bucket
    // (BH_SORT_DIRECT=0: never; 2: whatever their number -- the list holds every body --, tests; BH_SORT_DIRECT_MAX: the threshold)
    int sort_direct = 1;
    int64_t sort_direct_max = kSortDirectMax;
    uint64_t *keys_scatter = nullptr;     // the counting pass's own output array, so that both inputs end in keys[1] / vals[1]
    uint64_t *direct_list = nullptr, *direct_range_keys = nullptr;
    uint32_t *direct_count = nullptr;     // two counters: a build counts into one and clears the other for the next
    uint32_t direct_cap = 0, direct_subcap = 0;
    int direct_nsub = 1;
    int direct_slot = 0;                  // the counter the next build counts into (zero by then)
    bool sort_place = true;               // bucket_sort_kernel finishes a nearly ordered bucket by placement (BH_SORT_PLACE=0 disables, A/B)
    uint32_t *sort_paths = nullptr;       // [2][kBucketsBig] per bucket number: times placed, times through the passes (bh_sort_paths)
    // what the last build's sort was given (bh_sort_snapshot): direct_slot has been flipped by the time anybody asks.
    // offered: direct input was offered, and `count` is the block that build counted into; the output is keys_sorted / perm
    struct SortRecord {
        bool valid = false, offered = false;
        int64_t n = 0;
        int nb = 0, nsub = 0;
        uint32_t len = 0, cap = 0, subcap = 0;
        const uint32_t *count = nullptr;
    } sort_rec;
    int build_items = 0;          // 0 = automatic, else keys per thread in the sort / scan kernels (2, 4, 8)
    bool hilbert = false;                // fp32 mode: Hilbert-ordered keys (BH_HILBERT=0 disables, A/B)
    bool chain_collapse = true;          // fp32 step build: slots link past single-child cell chains (BH_CHAIN_COLLAPSE=0 disables, A/B)
    double *bslots = nullptr;      // kBoundSlots running bounds records (bh_bounds.hpp)

    // state (double2/double or float2/float).  Exact mode: caller order.  fp32 / mixed: DEVICE order --
    // every reorder_every-th build the bodies are physically permuted into that build's sorted order
    // (the gathers through `perm` in prep and in the walk's epilogue then touch neighbouring lines),
    // and orig[slot] remembers the caller's index; every host-facing call translates back.
    void *pos = nullptr, *vel = nullptr, *mass = nullptr, *force = nullptr;
    void *pos2 = nullptr, *vel2 = nullptr, *mass2 = nullptr, *force2 = nullptr;
    uint32_t *orig = nullptr, *orig2 = nullptr;
    int reorder_every = 16;        // BH_REORDER_EVERY; 0 = never
    // sorted-order copies (fp32 mode)
    float2 *spos = nullptr;
    float4 *sstate = nullptr;      // sorted-order {x, y, vx, vy}: the replicated scheme's one exchange buffer
    float *smass = nullptr;
    // sort
    uint64_t *keys[2] = {nullptr, nullptr};
    uint32_t *vals[2] = {nullptr, nullptr};
    uint64_t *keys_sorted = nullptr;
    uint32_t *perm = nullptr;
    uint32_t *radix_counts = nullptr, *bsum_sort = nullptr, *bsum_u32 = nullptr, *cnt = nullptr;
    uint64_t *coarse = nullptr;          // fp32: every 256th sorted key
    uint32_t *cell_first = nullptr;      // fp32: rank of a subdivided cell -> its first sorted body
    d3 *terms = nullptr, *bsum_d3 = nullptr;
    double *partial = nullptr, *box = nullptr;
    // tree
    NodeD *gd = nullptr;
    LinkD *ld = nullptr;
    QuadF *qf = nullptr;
    NodeAux *aux = nullptr;
    int32_t *self_node = nullptr, *cell_depth = nullptr;
    uint32_t *com_pending = nullptr;   // exact mode: subdivided children per cell still to be summed
    TreeCounters *ctr = nullptr;

    // ownership (multi-GPU): sorted range [lo, hi) = rank's share
    int rank = 0, world = 1;
    // distributed step with locally-essential trees (bh_let_*): this context holds only its own bodies
    bool let_mode = false, external_box = false;
    int64_t let_cap = 0, quads_local = 0;
    int64_t forest_base = 0;       // first quad of the received blocks: THE SAME ON EVERY RANK (>= quads_local)
    uint64_t *needmask = nullptr;
    uint32_t *let_tsum = nullptr, *let_outidx = nullptr;
    QuadF *let_send = nullptr;
    double *lbounds = nullptr, *all_bounds = nullptr;
    float2 *acc_part = nullptr;    // LET mode: raw sums of the local-tree walk (bh_let_walk_local)
    LetCounters *let_ctr = nullptr;
    // migration / re-balancing (bh_migrate.hpp)
    int64_t *gid = nullptr;             // 64-bit id per body, caller order
    uint32_t *group_cost = nullptr;     // cost of every 64-body group in the last walk (sorted order)
    const void **walk_consts = nullptr; // device block {aux, spos, smass, 0} for the assembly walk's bucket path
    uint32_t *body_counts = nullptr;    // BH_FLAG_WALK_STATS: accepted force evaluations per body (device slot order)
    // diagnostics (bh_diag.hpp), allocated on first use: potential and terms per body (state order), reduction records
    double *phi = nullptr;
    uint32_t *phi_counts = nullptr;
    double *diag_part = nullptr, *diag_out = nullptr;
    // the split operators (bh_split.hpp; is.forces_current): the records of bh_timestep are allocated on first use
    TsRecord *ts_part = nullptr, *ts_out = nullptr;
    // the analysis queries (bh_queries_host.hpp; one struct per family, bh_queries_state.hpp), all allocated on first use
    MapState map;
    RadState rad;
    ModState mod;
    DiscState disc;
    FieldState field;
    NbState nb;
    PairState pair;
    FofState fof;
    MstState mst;
    BinState bin;
    NblState nbl;
    // the quiet scope's device-side copies (quietly), allocated on first use; perm_save: the last force walk's permutation
    double *slots_save = nullptr;
    TreeCounters *ctr_save = nullptr;
    uint32_t *perm_save = nullptr;
    // direct sums and the force check (bh_direct.hpp), allocated on first use: caller index -> slot, one launch's targets and
    // results (capacity of them), and the check walk's own force / count / group-cost outputs
    uint32_t *slot_of = nullptr;
    int64_t *direct_targets = nullptr;
    double2 *direct_out = nullptr;
    void *check_force = nullptr;
    uint32_t *check_counts = nullptr, *check_cost = nullptr;
    bool sort_pack = true;              // BH_SORT_PACK=0: separate key and index arrays in every pass (A/B)
    unsigned long long *orb_hist = nullptr;
    double *mig_send = nullptr, *mig_recv = nullptr;
    ExpHooks exp;                       // A/B builds only (-DBHGPU_EXPERIMENTS); an empty struct in the product

    // measurement
    std::vector<hipEvent_t> ev;        // pairs around the walk kernel, one pair per step
    hipEvent_t ev_step[2] = {nullptr, nullptr}, ev_build[2] = {nullptr, nullptr};
    hipEvent_t ev_grp[3] = {nullptr, nullptr, nullptr};   // after keys / sort / scan of the last timed build
    hipEvent_t ev_let[3] = {nullptr, nullptr, nullptr};   // bh_let_build: start, local tree built, LETs packed
    bool let_timed = false;
    int64_t steps_done = 0;
    int32_t last_nsteps = 0;
    int timed_pairs = 0;
    bool step_timed = false;

    std::vector<void *> allocs;
    uint64_t device_bytes = 0;
    std::string err;
};

using Mode = bh_ctx::Mode;

namespace {

int fail(bh_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define BH_HIP(c, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), BH_ERR_DEVICE,                                                     \
                        std::string(#call) + ": " + hipGetErrorString(e_));                     \
    } while (0)

template <typename T>
int dev_alloc(bh_ctx *c, T **out, size_t count)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return fail(c, BH_ERR_DEVICE, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    c->allocs.push_back(p);
    c->device_bytes += bytes;
    *out = static_cast<T *>(p);
    return BH_OK;
}

inline void dev_free(bh_ctx *c, void *p)
{
    if (!p) return;
    auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
    if (it != c->allocs.end()) { c->allocs.erase(it); (void)hipFree(p); }
}

inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// f(std::bool_constant<b>{}...) for runtime bools b...: every combination is instantiated
template <typename F>
void dispatch(F &&f) { f(); }
template <typename F, typename... B>
void dispatch(F &&f, bool b, B... rest)
{
    if (b) dispatch([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else dispatch([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// f(double2{}) or f(float2{}): the vector type of the state arrays (its scalar type is decltype(Real2{}.x))
template <typename F>
void with_state(const bh_ctx *c, F &&f)
{
    if (c->state64()) f(double2{}); else f(float2{});
}

// bytes of a walk's output for n bodies: forces (fp64 tree) or accelerations (fp32 / mixed)
inline size_t force_bytes(const bh_ctx *c, int64_t n)
{
    return (size_t)std::max<int64_t>(n, 1) * 2 * (c->tree64() ? sizeof(double) : sizeof(float));
}

// node kernels and the mass pass: one thread per subdivided cell; I <= (n-1)*Dm and <= internal_cap (at least one
// thread: the root-only case)
inline int64_t cell_span(const bh_ctx *c)
{
    return std::max<int64_t>(1, std::min<int64_t>(c->internal_cap, std::max<int64_t>(c->n - 1, 0) * (int64_t)std::max(1, c->Dm)));
}

void owned_range(const bh_ctx *c, int64_t *lo, int64_t *hi)
{
    if (c->let_mode) { *lo = 0; *hi = c->n; return; }     // a LET context holds only its own bodies
    // equal chunks of ceil(n/world) sorted slots rounded up to the workgroup size (the last ranks
    // may own fewer, or none): every rank then forms exactly the wavefronts the single-GPU run
    // forms, so per-body summation order -- and therefore every bit of the result -- does not
    // depend on the number of GPUs; and the all_gather moves one fixed-size block per rank
    const int64_t per = (c->n + c->world - 1) / c->world;
    const int64_t chunk = (per + kBlock - 1) / kBlock * kBlock;
    *lo = std::min<int64_t>(c->n, chunk * c->rank);
    *hi = std::min<int64_t>(c->n, chunk * (c->rank + 1));
}

constexpr int64_t kComClimbMaxBodies = 32768;     // exact mode: single-launch bottom-up mass pass up to here
constexpr int64_t kSmallBuildBodies = 327680;    // up to here: tiles of 512 instead of 2,048 (measured)
constexpr int64_t kMediumBuildBodies = 786432;   // up to here: tiles of 1,024
constexpr int kSmallItems = 2;

// Physically permute the state into the sorted order of the build that has just produced `perm`
// (sorted index -> slot); afterwards slot == sorted index, so perm becomes the identity.
template <typename Real2, typename Real>
__global__ __launch_bounds__(kBlock) void reorder_state_kernel(uint32_t *__restrict__ perm, const Real2 *__restrict__ pos,
                                                                const Real2 *__restrict__ vel, const Real *__restrict__ mass,
                                                                const float2 *__restrict__ acc, const uint32_t *__restrict__ orig,
                                                                Real2 *__restrict__ pos2, Real2 *__restrict__ vel2,
                                                                Real *__restrict__ mass2, float2 *__restrict__ acc2,
                                                                uint32_t *__restrict__ orig2, int64_t n)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t b = perm[s];
    pos2[s] = pos[b]; vel2[s] = vel[b]; mass2[s] = mass[b]; acc2[s] = acc[b];
    orig2[s] = orig ? orig[b] : b;                            // orig == nullptr: slots still are caller indices
    perm[s] = (uint32_t)s;
}

// fp32 node kernel.  full_aux: also the {first body, count} record of every node (the host export needs them;
// a step only needs those of bucket leaves).  Inputs are what the build left on the device, so it can be run
// again after the build (export_tree_host).  The step build of a single-GPU context links past single-child cell chains
// (nodes_fast_kernel, COLLAPSE); the export keeps the reference's tree -- every link -- and so does a LET context that has
// peers, whose extraction marks and packs quads by index (bh_let.hpp: a quad's need mask is written through the link to it).
// A LET context of world 1 has nobody to extract for -- every need mask it writes is zero, and the masks start out zero
// (bh_let_configure) -- so it takes the single context's links and stays that context's walk bit for bit.
static void launch_nodes_fast(bh_ctx *c, bool full_aux, hipStream_t st)
{
    dispatch([&](auto compat, auto full, auto chains) {
        constexpr bool kCollapse = decltype(chains)::value && !decltype(full)::value;
        hipLaunchKernelGGL((nodes_fast_kernel<decltype(compat)::value, decltype(full)::value, kCollapse>),
                           dim3(blocks_for(cell_span(c), kBlock)),
                           dim3(kBlock), 0, st, c->keys_sorted, c->coarse, c->cnt, c->cell_first, c->spos, c->smass, c->box,
                           c->terms, c->n, c->Dm, c->cfg.theta, c->internal_cap, c->qf, c->aux, c->ctr);
    }, c->compat, full_aux, c->chain_collapse && !(c->let_mode && c->world > 1));
}

// before the bounds are folded into the slot records (bh_bounds.hpp): every record +-inf
void clean_slots(bh_ctx *c) { if (c->carry.slots_dirty) hipLaunchKernelGGL(bounds_slots_reset, dim3(1), dim3(kWave), 0, c->stream, c->bslots); }

// Stable LSD radix sort of n keys over key bits [0, bits): kSortBits-wide digits, wave-private ranking, digit-sorted
// write-out, tiles of kBlock * SI keys.  Pass p reads keys[cur] / vals[cur] and writes keys[cur ^ 1] / vals[cur ^ 1], cur = 0
// first; returns the cur that holds the result.  packed: the index travels in the key word, no pass reads a value array (the
// kernels get a null input) and only the last writes one: the unpacked {key, index} pair.
template <int SI>
int enqueue_lsd_passes(hipStream_t st, uint64_t *const keys[2], uint32_t *const vals[2], uint32_t *counts, uint32_t *rows, int64_t n,
                       int bits, bool packed)
{
    constexpr int SB = kSortBits;
    const unsigned nbl = blocks_for(n, kBlock * SI);
    const int passes = (bits + SB - 1) / SB;
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = p * SB;
        auto scatter = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(nbl), dim3(kBlock), 0, st, keys[cur], packed ? nullptr : vals[cur], keys[cur ^ 1],
                               vals[cur ^ 1], counts, rows, n, shift, (int)nbl, nullptr, nullptr, nullptr, 0u, 0u, 1);
        };
        hipLaunchKernelGGL((radix_hist<SI, SB>), dim3(nbl), dim3(kBlock), 0, st, keys[cur], counts, n, shift, (int)nbl);
        hipLaunchKernelGGL(radix_rowscan, dim3(1 << SB), dim3(kBlock), 0, st, counts, rows, (int)nbl);
        if (!packed) scatter(radix_scatter_w<SI, SB>);
        else if (p + 1 == passes) scatter(radix_scatter_w<SI, SB, 2>);
        else scatter(radix_scatter_w<SI, SB, 1>);
        cur ^= 1;
    }
    return cur;
}

template <bool TREE64, bool STATE64 = TREE64, int ITEMS = kItems>
int enqueue_build_t(bh_ctx *c, bool may_reorder, bool time_groups)
{
    constexpr int TILE = kBlock * ITEMS;
    static_assert(!TREE64 || STATE64, "an fp64 tree is built from fp64 state");
    using Real2 = typename std::conditional<STATE64, double2, float2>::type;   // the state
    using Real = typename std::conditional<STATE64, double, float>::type;
    const int64_t n = c->n;
    const int Dm = c->Dm;
    hipStream_t st = c->stream;
    const Real2 *pos = static_cast<const Real2 *>(c->pos);     // (re-read after a reorder)
    const Real *mass = static_cast<const Real *>(c->mass);

    // 1. root box (ComputeRootBounds, project.cu:536-573): the min/max of the positions is in the bounds slot records
    //    (bh_bounds.hpp) -- folded by the previous step's walk, or here by bounds_partial when no walk has left it --
    //    and keys_kernel reduces and pads it (LET mode: let_box_kernel has set the global box and cleared the counters)
    const bool from_walk = c->carry.slots_valid;
    double *slots = c->external_box ? nullptr : c->bslots;
    if (slots) {
        if (!from_walk) {
            const unsigned nbb = std::max(1u, std::min(1024u, blocks_for(n, kBlock)));
            clean_slots(c);
            hipLaunchKernelGGL((bounds_partial<Real2>), dim3(nbb), dim3(kBlock), 0, st, pos, n, slots);
        }
    }
    BuildDone done{n, slots != nullptr, false, false, false, false};

    if (n > 0) {
        // 2. keys by fp64 bisection, 3. stable radix sort
        // keys of <= 40 bits for <= 2^24 bodies carry the body index in the key word through the sort
        const bool pack = Dm >= 1 && 2 * Dm <= kPackShift && n <= ((int64_t)1 << (64 - kPackShift))
                          && c->sort_pack;
        // bucket sort (bh_sort.hpp): one counting pass by splitters from the previous build + one in-LDS sort per bucket
        // (exact modes and BH_HILBERT=0 too since round 3: the splitters only have to be sorted, whatever curve the keys follow)
        // a launch of up to 4,096 keys is ONE bucket: no splitters, no counting pass (three launches of ~5 us less), the first build
        // included.  (One workgroup's LDS holds 12,288 keys, but at twelve keys per thread its chain of passes is longer than the
        // counting pass it saves: N = 12,288 measured 0.100 ms per build this way against 0.090 at N = 16,384 the other way.
        // BH_SORT_BUCKET=2 keeps the splitter path at every size, for the tests that compare it with the LSD passes.)
        const bool single = pack && n >= 2 && n <= 4 * kBsThreads && c->sort_bucket == 1;
        const bool bucket = !single && pack && n >= 2 && n <= kBucketMaxNBig && (c->sort_bucket == 2 || (c->sort_bucket == 1 && c->carry.samples_n == n));
        const int nb = (n <= kBucketMaxN) ? kBuckets : kBucketsBig;
        // sample positions behind the splitters: two per bucket where the key workgroups run long enough to hide the
        // sample workgroups (256 buckets: above 262k bodies; 1,024 buckets: above 3M), one per bucket otherwise
        const int ns = (nb == kBuckets) ? ((n > (int64_t)1 << 18) ? 2 * kBuckets : kBuckets)
                                        : ((n > (int64_t)3 << 20) ? kMaxSplitSamples : kBucketsBig);
        static_assert(kBucketMaxN == (int64_t)1 << 20 && kBucketMaxNBig == (int64_t)1 << 22, "BASELINE configs 3 and 4 fit");
        done.sort_bucket = bucket || single; done.sort_packed = pack;
        // direct input (bh_sort.hpp): the state is in the sorted order of a recent build of these bodies, so the keys come out
        // sorted but for the bodies that changed bucket; the device decides per build whether the counting pass has to run
        const bool direct = bucket && !TREE64 && c->sort_direct != 0 && c->carry.samples_n == n;
        SortDirect sd;
        BucketDirect bd;
        if (direct) {
            const uint32_t len = (uint32_t)((n + nb - 1) / nb);
            sd.count = c->direct_count + c->direct_slot * kDirectCounterWords;
            sd.count_next = c->direct_count + (c->direct_slot ^ 1) * kDirectCounterWords;
            sd.list = c->direct_list; sd.range_keys = c->direct_range_keys; sd.cap = c->direct_cap; sd.subcap = c->direct_subcap;
            sd.len = len; sd.nsub = c->direct_nsub;
            bd.count = sd.count; bd.list = sd.list; bd.range_keys = sd.range_keys; bd.keys = c->keys[0]; bd.scratch = c->keys_scatter;
            bd.n = n; bd.cap = sd.cap; bd.subcap = sd.subcap; bd.len = len; bd.nb = nb; bd.nsub = sd.nsub;
            c->direct_slot ^= 1;
        }
        {
            const unsigned nkb = blocks_for(n, kBlock);
            auto keys_launch = [&](auto fs, auto pk, auto hil) {
                constexpr bool H = decltype(hil)::value, P = decltype(pk)::value, F = decltype(fs)::value;
                const bool smp = P && bucket;                       // (the splitter workgroups go with the packed keys)
                // samples: the previous build's sorted positions -- the fp32 walk's copy, or through the previous perm in the exact modes
                hipLaunchKernelGGL((keys_kernel<Real2, H, P, F>), dim3(nkb + (smp ? ns / kWave : 0)), dim3(kBlock), 0, st, pos, c->box,
                                   c->keys[0], c->vals[0], n, Dm, (smp && !TREE64) ? (const float2 *)c->spos : nullptr, c->splitters, nb, ns,
                                   slots, c->ctr, smp ? c->bsum_sort : nullptr, smp ? nb : 0, (smp && TREE64) ? c->perm : nullptr,
                                   from_walk ? 1 : 0, smp ? sd : SortDirect{});
            };
            // (exact mode and BH_HILBERT=0: child-index keys, packed all the same)
            dispatch(keys_launch, slots != nullptr, pack, c->hilbert);
        }
        if (time_groups) (void)hipEventRecord(c->ev_grp[0], st);
        const unsigned nbl = blocks_for(n, ITEMS == kItems ? kSortTile : TILE);
        int cur = 0;
        if (single) {
            hipLaunchKernelGGL(bucket_sort_kernel, dim3(1), dim3(kBsThreads), 0, st, c->keys[0], c->keys[1], c->vals[1],
                               nullptr, nullptr, &c->ctr->sort_spills, &c->ctr->sort_reruns, (int)n, BucketDirect{}, c->sort_paths,
                               c->sort_place ? 1 : 0);
            cur = 1;
        } else if (bucket) {
            constexpr int SI = (ITEMS == kItems ? kSortItems : ITEMS);
            auto pass = [&](auto bits_tag) {
                constexpr int NBITS = decltype(bits_tag)::value;
                if constexpr (TREE64) {                               // (state in caller order: the pass with its row scan, see radix_scatter_w)
                    hipLaunchKernelGGL((radix_hist<SI, NBITS, true>), dim3(nbl), dim3(kBlock), 0, st, c->keys[0], c->radix_counts, n,
                                       0, (int)nbl, c->splitters, c->sort_dig, nullptr);
                    hipLaunchKernelGGL(radix_rowscan, dim3(1 << NBITS), dim3(kBlock), 0, st, c->radix_counts, c->bsum_sort, (int)nbl);
                    hipLaunchKernelGGL((radix_scatter_w<SI, NBITS, 1, true, false>), dim3(nbl), dim3(kBlock), 0, st, c->keys[0], c->vals[0],
                                       c->keys[1], c->vals[1], c->radix_counts, c->bsum_sort, n, 0, (int)nbl, c->sort_dig,
                                       c->bsum_sort + kBucketStartOffset);
                } else {
                    // (direct: both kernels return at once unless the device took the decision for the counting pass, and the
                    // scatter writes an array of its own -- the sort's output is keys[1] / vals[1] whichever input it had)
                    hipLaunchKernelGGL((radix_hist<SI, NBITS, true>), dim3(nbl), dim3(kBlock), 0, st, c->keys[0], c->radix_counts, n,
                                       0, (int)nbl, c->splitters, c->sort_dig, c->bsum_sort, sd.count, sd.cap, sd.subcap, sd.nsub);
                    hipLaunchKernelGGL((radix_scatter_w<SI, NBITS, 1, true>), dim3(nbl), dim3(kBlock), 0, st, c->keys[0], c->vals[0],
                                       direct ? c->keys_scatter : c->keys[1], c->vals[1], c->radix_counts, c->bsum_sort, n, 0, (int)nbl,
                                       c->sort_dig, c->bsum_sort + kBucketStartOffset, sd.count, sd.cap, sd.subcap, sd.nsub);
                }
            };
            if (nb == kBuckets) pass(std::integral_constant<int, 8>{}); else pass(std::integral_constant<int, 10>{});
            if (direct) {
                hipLaunchKernelGGL(bucket_sort_kernel, dim3(nb), dim3(kBsThreads), 0, st, c->keys_scatter, c->keys[1], c->vals[1],
                                   c->bsum_sort, c->bsum_sort + kBucketStartOffset, &c->ctr->sort_spills, &c->ctr->sort_reruns, 0, bd,
                                   c->sort_paths, c->sort_place ? 1 : 0);
                cur = 1;
            } else {
                hipLaunchKernelGGL(bucket_sort_kernel, dim3(nb), dim3(kBsThreads), 0, st, c->keys[1], c->keys[0], c->vals[0],
                                   c->bsum_sort, c->bsum_sort + kBucketStartOffset, &c->ctr->sort_spills, &c->ctr->sort_reruns, 0,
                                   BucketDirect{}, c->sort_paths, c->sort_place ? 1 : 0);
                cur = 0;
            }
        } else {
            constexpr int SI = (ITEMS == kItems ? kSortItems : ITEMS);
            cur = enqueue_lsd_passes<SI>(st, c->keys, c->vals, c->radix_counts, c->bsum_sort, n, 2 * Dm, pack);
        }
        c->keys_sorted = c->keys[cur];
        c->perm = c->vals[cur];
        c->sort_rec = bh_ctx::SortRecord{true, direct, n, nb, direct ? sd.nsub : 0, sd.len, sd.cap, sd.subcap, sd.count};
        if constexpr (!TREE64) {
            if (may_reorder && c->reorder_every > 0 && c->carry.builds % c->reorder_every == 0) {
                hipLaunchKernelGGL((reorder_state_kernel<Real2, Real>), dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, st,
                                   c->perm, pos, static_cast<const Real2 *>(c->vel), mass,
                                   static_cast<const float2 *>(c->force), c->is.orig_identity ? nullptr : c->orig,
                                   static_cast<Real2 *>(c->pos2), static_cast<Real2 *>(c->vel2),
                                   static_cast<Real *>(c->mass2), static_cast<float2 *>(c->force2), c->orig2, n);
                std::swap(c->pos, c->pos2); std::swap(c->vel, c->vel2); std::swap(c->mass, c->mass2);
                std::swap(c->force, c->force2); std::swap(c->orig, c->orig2);
                done.reordered = true;
                pos = static_cast<const Real2 *>(c->pos);
                mass = static_cast<const Real *>(c->mass);
            }
        }
        if (time_groups) (void)hipEventRecord(c->ev_grp[1], st);

        // 4. cells owned by each sorted neighbour pair (+ fp32: sorted copies and prefix-sum terms),
        // 5. their ranks / the prefix sums
        using SReal2 = typename std::conditional<TREE64, double2, float2>::type;    // what the walk reads
        using SReal = typename std::conditional<TREE64, double, float>::type;
        // elements per thread in prep / scan_apply2: the sort's tile size, except that between 768k and
        // 2M bodies tiles of 1,024 are still the better choice for these two (a workgroup's rows are a
        // chain of load -> scan -> store; measured at N = 1M: 42.5 -> 33 us for the pair)
        auto scan_part = [&](auto si_tag) {
            constexpr int SI = decltype(si_tag)::value;
            const unsigned nbs = blocks_for(n + 1, kBlock * SI);
            hipLaunchKernelGGL((prep_kernel<TREE64, SI, Real2, Real, SReal2, SReal>), dim3(nbs), dim3(kBlock), 0, st,
                               c->keys_sorted, c->perm, pos, mass, c->cnt, c->bsum_u32, (SReal2 *)c->spos,
                               (SReal *)c->smass, c->terms, c->bsum_d3, c->coarse, n, Dm, slots);
            constexpr bool TSRC = !TREE64 && std::is_same<Real2, SReal2>::value;   // fp32 state: terms from the sorted copies
            if (nbs <= 8u * kBlock) {
                // few tiles: every workgroup sums the tile totals before it itself (no scan_top2 launch)
                hipLaunchKernelGGL((scan_apply2<TREE64, SI, true, TSRC>), dim3(nbs), dim3(kBlock), 0, st, c->cnt, c->bsum_u32,
                                   c->terms, c->bsum_d3, (int)nbs, n, c->cell_first, c->internal_cap, c->ctr,
                                   (const float2 *)c->spos, (const float *)c->smass);
            } else {
                hipLaunchKernelGGL(scan_top2, dim3(TREE64 ? 1 : 2), dim3(kBlock), 0, st, c->bsum_u32, c->bsum_d3,
                                   (int)nbs, c->ctr);
                hipLaunchKernelGGL((scan_apply2<TREE64, SI, false, TSRC>), dim3(nbs), dim3(kBlock), 0, st, c->cnt, c->bsum_u32,
                                   c->terms, c->bsum_d3, (int)nbs, n, c->cell_first, c->internal_cap, c->ctr,
                                   (const float2 *)c->spos, (const float *)c->smass);
            }
        };
        if (ITEMS == kItems && n <= (int64_t)1 << 21) scan_part(std::integral_constant<int, 4>{});
        else scan_part(std::integral_constant<int, ITEMS>{});
        if (time_groups) (void)hipEventRecord(c->ev_grp[2], st);
    } else {
        if (slots)          // no keys: one workgroup still writes the box and clears the counters
            hipLaunchKernelGGL((keys_kernel<Real2, false, false, true>), dim3(1), dim3(kBlock), 0, st, pos, c->box, c->keys[0],
                               c->vals[0], n, Dm, nullptr, nullptr, 0, 0, slots, c->ctr);
        c->keys_sorted = c->keys[0];
        c->perm = c->vals[0];
        c->sort_rec = bh_ctx::SortRecord{};
        c->sort_rec.valid = true;
        if (time_groups) for (auto e : c->ev_grp) (void)hipEventRecord(e, st);
    }

    // 6. nodes (thread 0 writes the root when nothing is subdivided)
    if constexpr (TREE64) {
        hipLaunchKernelGGL(nodes_exact_kernel, dim3(blocks_for(cell_span(c), kBlock)), dim3(kBlock), 0, st, c->keys_sorted, c->perm,
                           c->cnt, c->cell_first, pos, mass, c->box, n, Dm, c->internal_cap, c->gd, c->ld, c->self_node,
                           c->cell_depth, c->com_pending, c->ctr, (c->mode == Mode::F64 || c->exact_thresholds) ? c->cfg.theta : 0.0,
                           c->exact_thresholds ? 1 : 0);
    } else {
        launch_nodes_fast(c, false, st);
    }
    // 7. exact bottom-up mass pass (ComputeMass, project.cu:473-502): ONE launch for small trees (the climb of
    //    com_up_kernel), one launch per depth for large ones, where the climb's coherence traffic costs more
    //    than the launches (measured cross-over ~65k bodies; see com_level_kernel).  Bitwise the same sums.
    if (TREE64 && n > 1 && c->internal_cap > 0) {
        const int64_t span = cell_span(c);
        if (n <= kComClimbMaxBodies) {
            hipLaunchKernelGGL(com_up_kernel, dim3(blocks_for(span, kBlock)), dim3(kBlock), 0, st, c->gd, c->ld,
                               c->self_node, c->com_pending, c->ctr, c->internal_cap);
        } else {
            for (int d = Dm - 1; d >= 0; --d)
                hipLaunchKernelGGL(com_level_kernel, dim3(blocks_for(span, kBlock)), dim3(kBlock), 0, st, c->gd,
                                   c->self_node, c->cell_depth, c->ctr, c->internal_cap, d);
        }
    }
    const hipError_t err = hipGetLastError();
    done.launched = err == hipSuccess;
    c->build_completed(done);
    BH_HIP(c, err);
    return BH_OK;
}

template <int ITEMS>
static int enqueue_build_items(bh_ctx *c, bool may_reorder, bool time_groups)
{
    if (c->tree64()) return enqueue_build_t<true, true, ITEMS>(c, may_reorder, time_groups);
    return c->state64() ? enqueue_build_t<false, true, ITEMS>(c, may_reorder, time_groups)
                        : enqueue_build_t<false, false, ITEMS>(c, may_reorder, time_groups);
}

// may_reorder = false: a quiet build never permutes the state; time_groups: bh_step's last build records ev_grp
int enqueue_build(bh_ctx *c, bool may_reorder = true, bool time_groups = false)
{
    // keys per thread in the sort / scan kernels: launches of few bodies take smaller tiles (more
    // workgroups, fewer sequential rounds in each); BH_BUILD_ITEMS = 2, 4 or 8 overrides
    int items = c->build_items;
    if (items == 0) items = c->n <= kSmallBuildBodies ? 2 : c->n <= kMediumBuildBodies ? 4 : 8;
    if (c->n > (1 << 22)) items = 8;         // (scratch for small tiles is sized for 4M bodies)
    switch (items) {
    case 2: return enqueue_build_items<2>(c, may_reorder, time_groups);
    case 4: return enqueue_build_items<4>(c, may_reorder, time_groups);
    default: return enqueue_build_items<kItems>(c, may_reorder, time_groups);
    }
}

// fp64 walks (exact and throughput): bodies per wavefront for a launch of `cnt` bodies.  A wave's walk is one dependent chain
// over the union of its bodies' walks (~900 node visits for 64 bodies, ~150 for one), and up to ~130k bodies the launch cannot
// fill the GPU's 8,192 wave slots with 64-body waves anyway.  Measured (scripts/bpw_ab.py, profiles/r04_f64/bpw_sweep.txt): the
// best number of waves is ~4,096 for the throughput walk: the smallest power of two that stays below that.  The bit-exact walk
// (round 4's assembly loop, ~50 vector instructions per visit; scripts/bpw_ab.py -> profiles/r04_exact/bpw_sweep.txt): one body
// per wave up to 4,096 bodies, from there 16 bodies per wave or what keeps the launch within ~2,048 waves (more waves than that
// cost more vector work than the shorter chains return).  BH_EXACT_BPW sets it for both walks.  The bit-exact mode's results do
// not depend on it, bit for bit.
static int fp64_bodies_per_wave(const bh_ctx *c, int64_t cnt)
{
    // (the throughput walk adds a lane's terms in the order its WAVE meets them: its last bits depend on who shares the wave, like
    // the fp32 split walk's -- BH_FLAG_WALK_NO_SPLIT pins 64 bodies per wave for callers that need launch-size independence)
    if (c->mode == Mode::F64 && (c->cfg.flags & BH_FLAG_WALK_NO_SPLIT)) return kWave;
    int b = 1;
    if (c->exact_bpw > 0) b = c->exact_bpw;
    else if (c->mode == Mode::F64) {
        while (b < kWave && (int64_t)b * 4096 < cnt) b <<= 1;
    } else if (cnt > 4096) {
        b = 16;
        while (b < kWave && (int64_t)b * 2048 < cnt) b <<= 1;
    }
    return b;
}

// What the launches of one enqueue_walk share
struct WalkRange {
    int64_t lo, hi;            // the owned sorted range
    int64_t pass;              // bodies per launch (hi - lo: one launch)
    bool integrate, to_sorted, stats;
    int part;                  // LET mode: 1 = local tree only, 2 = received trees only, 0 = both
    double *partial;           // LET mode, fp32 walk: per-workgroup min/max of the new positions (bh_let_bounds), may be null
    double *slots;             // bounds slot records for the next keys_kernel (bh_bounds.hpp), may be null
};

enum class WalkKind { F64, ExactBfs, Exact, F32 };

struct WalkChoice {
    WalkKind kind;
    bool use_asm;              // the hand-written loop instead of the C++ statement of the same walk
    int bpw;                   // fp64 cooperative walks: bodies per wavefront
};

// Which walk a launch of this context runs
WalkChoice choose_walk(const bh_ctx *c, const WalkRange &w)
{
    const bool portable = (c->cfg.flags & BH_FLAG_WALK_PORTABLE) != 0;
    // the fp64 hand-written loops and the breadth-first walk address the node array with 32-bit byte offsets
    const bool nodes32 = c->node_cap * (int64_t)sizeof(NodeD) < (1ll << 32);
    const int64_t cnt = std::min(w.pass, w.hi - w.lo);
    switch (c->mode) {
    case Mode::F64:
        // hand-written loop (walk64_asm); the counting variant and BH_FLAG_WALK_PORTABLE run the C++ statement of the same
        // loop (same operations, same order, same bits)
        return {WalkKind::F64, c->walk_asm && !w.stats && !portable && nodes32, fp64_bodies_per_wave(c, cnt)};
    case Mode::Exact:
        // launches of a few thousand bodies: one wavefront per BODY, its tree breadth-first (walk_exact_bfs_kernel) -- the same
        // bits as the cooperative walk, which an explicit BH_EXACT_BPW, the counting variant and the portable walk keep using
        if (c->exact_thresholds && !w.stats && c->exact_bpw == 0 && w.pass == w.hi - w.lo && w.hi - w.lo <= c->bfs_max && nodes32)
            return {WalkKind::ExactBfs, false, 0};
        // (the node kernel stored what the cooperative walk reads in the size slot: exact thresholds, or the sizes for the
        // portable walk; the hand-written loop carries no counters)
        return {WalkKind::Exact, c->exact_thresholds && !w.stats && nodes32, fp64_bodies_per_wave(c, cnt)};
    default: {
        // hand-scheduled loop: byte offsets into the quad array and the sorted bodies are 32-bit there, and the SGPR
        // offset of s_load is an UNSIGNED 32-bit value on gfx950 (scripts/calib/soffset_calib.hip, profiles/r03_final/
        // soffset_calib.txt: offsets up to 0xf0000100 read base + offset): 4 GiB of quads = 53.6 M.  (Round 2 stopped at
        // 2 GiB, so BASELINE config 5 -- capacity 33.5 M quads -- ran the C++ loop.)
        const int64_t forest_quads = c->let_mode ? c->forest_base + (int64_t)c->world * c->let_cap : c->internal_cap + 1;
        return {WalkKind::F32, c->walk_asm && !portable && forest_quads * (int64_t)sizeof(QuadF) < (1ll << 32) && c->n < (1ll << 28), 0};
    }
    }
}

// The launchers, one per walk family: each returns BH_OK or a BH_ERR_* code.

// One launch per pass of w.pass bodies: launch(lo, hi, workgroups of per_group bodies) returns BH_OK or a BH_ERR_* code
template <typename Launch>
int each_pass(bh_ctx *c, const WalkRange &w, int per_group, Launch launch)
{
    for (int64_t plo = w.lo; plo < w.hi; plo += w.pass) {
        const int64_t phi = std::min(w.hi, plo + w.pass);
        if (int rc = launch(plo, phi, blocks_for(phi - plo, per_group))) return rc;
        c->walk_launched();
    }
    return BH_OK;
}

int launch_walk_f64(bh_ctx *c, const WalkRange &w, const WalkChoice &k)
{
    const bool deep = 3 * c->Dm + 1 > kWave;                 // (deeper than 21 levels: the two-tier stack)
    return each_pass(c, w, (kF64Block / kWave) * k.bpw, [&](int64_t plo, int64_t phi, unsigned grid) {
        WalkF64Args wa{};
        wa.gd = c->gd; wa.ld = c->ld; wa.perm = c->perm; wa.pos = (double2 *)c->pos; wa.vel = (double2 *)c->vel;
        wa.mass = (const double *)c->mass; wa.force_out = (double2 *)c->force; wa.lo = plo; wa.hi = phi;
        wa.G = c->cfg.G; wa.dt = c->cfg.dt; wa.integrate = w.integrate ? 1 : 0; wa.ctr = c->ctr;
        wa.body_counts = w.stats ? c->body_counts : nullptr; wa.slots = w.slots; wa.bpw = k.bpw;
        wa.eps2 = c->eps2;
        dispatch([&](auto compat, auto deep_stack) {
            constexpr bool CP = decltype(compat)::value, DP = decltype(deep_stack)::value;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kF64Block), 0, c->stream, wa); };
            if (c->eps2 != 0.0) {                                    // softened terms: the same loops with one v_add_f64
                if (w.stats) go(walk_f64_soft_kernel<CP, true, DP, false>);
                else if (k.use_asm) go(walk_f64_soft_kernel<CP, false, DP, true>);
                else go(walk_f64_soft_kernel<CP, false, DP, false>);
            }
            else if (w.stats) go(walk_f64_kernel<CP, true, DP, false>);
            else if (k.use_asm) go(walk_f64_kernel<CP, false, DP, true>);
            else go(walk_f64_kernel<CP, false, DP, false>);
        }, c->compat, deep);
        return BH_OK;
    });
}

// a workgroup = four wavefronts, each taking bodies (turn * grid + workgroup) * 4 + wave one after the other; at most
// max(1,024, capacity / 64) workgroups, every wave at most 64 bodies
int launch_walk_exact_bfs(bh_ctx *c, const WalkRange &w)
{
    const int64_t cnt = w.hi - w.lo;
    const int64_t max_groups = std::max<int64_t>(1024, (c->cfg.capacity + kWave - 1) / kWave);
    const int64_t grid = std::max<int64_t>(std::min<int64_t>(blocks_for(cnt, kWavesPerBlock), max_groups),
                                           blocks_for(cnt, kWavesPerBlock * kBfsBodiesPerWave));
    // (more interactions per body in larger trees: 384 terms per walk -- 52 KB of LDS per workgroup, three per CU; 512 would leave two)
    dispatch([&](auto compat, auto big) {
        hipLaunchKernelGGL((walk_exact_bfs_kernel<decltype(compat)::value, decltype(big)::value ? 384 : 256>), dim3((unsigned)grid),
                           dim3(kBlock), 0, c->stream, c->gd, c->ld, c->perm, (double2 *)c->pos, (double2 *)c->vel,
                           (const double *)c->mass, (double2 *)c->force, w.lo, w.hi, c->cfg.G, c->cfg.dt, w.integrate ? 1 : 0,
                           c->ctr, w.slots, c->box);
    }, c->compat, cnt > 4096);
    c->walk_launched();
    return BH_OK;
}

int launch_walk_exact(bh_ctx *c, const WalkRange &w, const WalkChoice &k)
{
    return each_pass(c, w, kWavesPerBlock * k.bpw, [&](int64_t plo, int64_t phi, unsigned grid) {
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, c->stream, c->gd, c->ld, c->perm, (double2 *)c->pos,
                               (double2 *)c->vel, (const double *)c->mass, (double2 *)c->force, plo, phi, c->cfg.theta, c->cfg.G,
                               c->cfg.dt, w.integrate ? 1 : 0, c->ctr, w.slots, k.bpw, c->box);
        };
        dispatch([&](auto compat) {
            constexpr bool CP = decltype(compat)::value;
            if (!c->exact_thresholds) { if (w.stats) go(walk_exact_kernel<CP, true, false, false>); else go(walk_exact_kernel<CP, false, false, false>); }
            else if (w.stats) go(walk_exact_kernel<CP, true, true, false>);
            else if (k.use_asm) go(walk_exact_kernel<CP, false, true, true>);
            else go(walk_exact_kernel<CP, false, true, false>);
        }, c->compat);
        return BH_OK;
    });
}

int launch_walk_f32(bh_ctx *c, const WalkRange &w, const WalkChoice &k)
{
    WalkFastArgs a{};
    a.quads = c->qf; a.aux = c->aux; a.partial = w.partial; a.spos = c->spos; a.smass = c->smass; a.perm = c->perm;
    a.pos = (float2 *)c->pos; a.vel = (float2 *)c->vel;
    a.state64 = c->state64() ? 1 : 0;             // mixed precision: pos/vel point at double2 arrays
    a.sstate = c->sstate;
    a.acc_out = (float2 *)c->force; a.ctr = c->ctr;
    a.lo = w.lo; a.hi = w.hi; a.G = (float)c->cfg.G; a.dt = (float)c->cfg.dt; a.dt64 = c->cfg.dt;
    a.integrate = w.integrate ? 1 : 0; a.to_sorted = w.to_sorted ? 1 : 0;
    a.n_trees = c->let_mode ? c->world : 0; a.self_rank = c->let_mode ? c->rank : -1;
    a.part = w.part; a.acc_part = c->acc_part;
    a.forest_base = c->forest_base; a.let_cap = c->let_cap;
    a.eps2 = c->eps2f;
    c->exp.walk_args(a);
    a.group_cost = (w.lo == 0 && w.hi == c->n) ? c->group_cost : nullptr;
    a.bucket_consts = c->walk_consts;
    a.slots = w.slots;
    a.body_counts = w.stats ? c->body_counts : nullptr;
    // the register-lane stack holds 128 entries and pairs entries only while the bound of
    // walk_tree_asm allows it, so it serves every max_depth <= 32; the LDS stack is the flag's variant
    const bool lds = (c->cfg.flags & BH_FLAG_LDS_STACK) != 0;
    a.pair_limit = std::max(0, 116 - 3 * c->Dm);   // the stack bound of walk_tree_asm2 (bh_walk_fast.hip)
    // few bodies: several waves per 64-body group (bh_walk_fast.hip).  Measured best factor
    // (scripts/split_ab.sh): 8 up to 32k bodies per launch, 4 up to ~100k, one wave
    // per group -- the hand-scheduled loop with two quads in flight -- beyond (round 1's compiled loop
    // lost to the split walk up to 192k; at 131k: 0.097 against 0.102 ms).  BH_WALK_SPLIT overrides (1 = off).
    int split = (c->cfg.flags & BH_FLAG_WALK_NO_SPLIT) || c->cfg.n_threads > 0 ? 1 : c->walk_split;   // (n_threads: one thread per body)
    if (split <= 0) {
        const int64_t groups = (w.hi - w.lo + kWave - 1) / kWave;
        // (a forest walk keeps the split longer: the level-synchronous walk seeds its first frontier with
        // all the roots, the one-wave loop walks tree after tree -- 8 ranks x 135k bodies: 0.270 vs 0.293 ms;
        // 4 ranks x 268k: 0.346 vs 0.298)
        // (measured with the hand-scheduled chunk loop, Plummer, walk ms for split 1 / 2 / 4 / 8 --
        //  768 groups: .089 .061 .042 .040; 1,536: .094 .073 .059 .074; 2,048: .098 .074 .078 .100;
        //  3,072: .108 .115 .102 .136; 3,584: .115 .127 .118 .157; profiles/r02_final/split_sweep.txt)
        split = groups <= (c->let_mode ? 512 : 768) ? 8 : groups <= 3072 ? 4 : 1;
    }
    if (3 * c->Dm + 2 > kWave) split = 1;        // the level-synchronous walk's depth-first fallback has 64 entries
    const int per_record = walk_fast_split_effective(a, lds, split) ? kWave : kBlock;
    if (w.partial) c->partials_recorded((int)blocks_for(w.hi - w.lo, per_record));
    return each_pass(c, w, per_record, [&](int64_t plo, int64_t phi, unsigned) -> int {
        a.lo = plo; a.hi = phi; a.partial = w.partial ? w.partial + 4 * ((plo - w.lo) / per_record) : nullptr;
        BH_HIP(c, launch_walk_fast(a, lds, w.stats, split, k.use_asm, c->stream));
        return BH_OK;
    });
}

int enqueue_walk(bh_ctx *c, bool integrate, bool to_sorted, int part = 0)
{
    WalkRange w{};
    owned_range(c, &w.lo, &w.hi);
    if (w.hi <= w.lo) return BH_OK;
    w.integrate = integrate; w.to_sorted = to_sorted; w.part = part;
    w.stats = (c->cfg.flags & BH_FLAG_WALK_STATS) != 0;
    c->walk_begins(part == 2);
    // N_THREADS (project.cu:5-7, 703: `body_i += N_THREADS`): at most that many bodies are walked at a time -- the
    // range is taken in passes of n_threads bodies, rounded up to whole 256-thread workgroups, one launch after the
    // other on the stream, as the reference's threads take their bodies one after the other.  0 (the default):
    // one pass.  It gives the thread axis of the reference's first scaling experiment (first_scaling_script.sh:
    // 17-36) a meaning on this hardware: n_threads = 1 is one workgroup at a time.
    w.pass = c->cfg.n_threads > 0 ? ((int64_t)c->cfg.n_threads + kBlock - 1) / kBlock * kBlock : w.hi - w.lo;
    // a walk over all bodies that integrates also leaves the min/max of the NEW positions for the next build's root box: its
    // workgroups fold them into the slot records the next keys_kernel reduces (bh_bounds.hpp), in every pass.  LET mode: the
    // fp32 walk writes one `partial` record per workgroup instead, for bh_let_bounds.
    const bool full = integrate && !to_sorted && w.lo == 0 && w.hi == c->n;
    if (full && c->let_mode) w.partial = c->partial;
    const bool want_slots = full && part == 0 && !c->let_mode && !c->external_box && c->n >= 2;
    if (want_slots) { clean_slots(c); w.slots = c->bslots; }
    if (integrate) c->positions_moved_by_walk(want_slots);

    const WalkChoice k = choose_walk(c, w);
    if (w.stats && (k.kind == WalkKind::F64 || k.kind == WalkKind::F32)) {      // (the bit-exact walks count no bodies)
        if (!c->body_counts) { int rc = dev_alloc(c, &c->body_counts, (size_t)std::max<int64_t>(c->cfg.capacity, 1)); if (rc) return rc; }
        // (a launch writes the slots of the bodies it walks: an owned range smaller than n, or a walk that returned
        // early on an overflowed tree, must not leave the others uninitialised; part 2 adds to the counts of part 1)
        if (part != 2) BH_HIP(c, hipMemsetAsync(c->body_counts, 0, (size_t)std::max<int64_t>(c->n, 1) * sizeof(uint32_t), c->stream));
    }
    int rc = BH_OK;
    switch (k.kind) {
    case WalkKind::F64: rc = launch_walk_f64(c, w, k); break;
    case WalkKind::ExactBfs: rc = launch_walk_exact_bfs(c, w); break;
    case WalkKind::Exact: rc = launch_walk_exact(c, w, k); break;
    case WalkKind::F32: rc = launch_walk_f32(c, w, k); break;
    }
    if (rc) return rc;
    BH_HIP(c, hipGetLastError());
    if (!c->tree64() && w.lo == 0 && w.hi == c->n) c->group_costs_written();
    return BH_OK;
}

int check_overflow(bh_ctx *c)
{
    TreeCounters h{};
    BH_HIP(c, hipMemcpyAsync(&h, c->ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    if (h.overflow || (int64_t)h.n_internal > c->internal_cap)
        return fail(c, BH_ERR_CAPACITY, "tree needs " + std::to_string(1 + 4 * (int64_t)h.n_internal) +
                                        " nodes, node_capacity is " + std::to_string(c->node_cap));
    return BH_OK;
}

// bh_upload / bh_initialize: the state arrays hold n new bodies in caller order
int upload_done(bh_ctx *c, int64_t n)
{
    c->n = n;
    c->new_bodies();
    c->steps_done = 0;
    if (c->gid && n > 0) {
        hipLaunchKernelGGL(iota_i64_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, c->stream, c->gid, n);
        BH_HIP(c, hipGetLastError());
    }
    return BH_OK;
}

// a non-integrating walk of this context covers every body (one GPU; a LET context and a rank of the replicated scheme do not)
bool forces_cover_all(const bh_ctx *c) { return !c->let_mode && c->world == 1; }

// BH_ERR_STATE with the caller's text unless a body set has been uploaded
int need_upload(bh_ctx *c, const std::string &text) { return c->is.uploaded ? BH_OK : fail(c, BH_ERR_STATE, text); }

// uploaded, and one context holds every body: else BH_ERR_STATE, `what` + `why_single` for the second
int single_gpu_check(bh_ctx *c, const char *what, const char *why_single)
{
    if (int rc = need_upload(c, std::string(what) + " before bh_upload")) return rc;
    return forces_cover_all(c) ? BH_OK : fail(c, BH_ERR_STATE, std::string(what) + why_single);
}

// the diagnostics and the analysis queries that need a tree or every body
int diag_check(bh_ctx *c, const char *what)
{
    return single_gpu_check(c, what, ": single GPU only -- in LET mode bh_let_potential / bh_let_energy give the potential "
                                     "and the energy sums; the replicated scheme (world > 1) and the other diagnostics have no distributed form");
}

// the split operators and the disc: uploaded, one context, and -- need_forces -- forces of the positions as they are
int split_check(bh_ctx *c, const char *what) { return single_gpu_check(c, what, ": single GPU only (not in LET mode or with world > 1)"); }

int need_forces(bh_ctx *c, const char *what)
{
    if (c->is.forces_current) return BH_OK;
    return fail(c, BH_ERR_STATE, std::string(what) + ": the force buffer does not hold the accelerations of the current positions "
                                 "(bh_compute_forces first; a step, bh_drift, bh_upload, bh_build_tree and a new softening length outdate them)");
}

// the LET calls' preconditions (c may be null): configured, and on demand bodies or a tree in the buffers
enum LetNeed { kLetConfigured, kLetBodies, kLetTree };
int let_check(bh_ctx *c, const char *who, LetNeed need)
{
    if (!c || !c->let_mode) return fail(c, BH_ERR_STATE, std::string(who) + ": call bh_let_configure first");
    if (need == kLetBodies) return need_upload(c, std::string(who) + " before bh_upload");
    return need == kLetTree && !c->is.tree_valid ? fail(c, BH_ERR_STATE, std::string(who) + " before bh_let_build") : BH_OK;
}

// host array with `per` values per body, read from the device in DEVICE order -> caller order (an fp64 tree never re-orders its
// state: orig_identity holds there)
template <typename T>
int to_caller_order(bh_ctx *c, T *host, int per)
{
    if (c->is.orig_identity || c->n == 0) return BH_OK;
    const int64_t n = c->n;
    std::vector<uint32_t> o(n);
    BH_HIP(c, hipMemcpy(o.data(), c->orig, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<T> t(host, host + (size_t)per * n);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < per; ++k) host[(size_t)per * o[i] + k] = t[(size_t)per * i + k];
    return BH_OK;
}

// The quiet scope: quietly(c, options, body) runs a diagnostic's builds and walks without perturbing the run.  A build inside is
// enqueue_build(c, false): it runs as a step's build would, except that it never re-orders the state.  Afterwards everything a
// later build reads from an earlier one and everything the last real build and walk report is put back -- BuildCarry and LastRun
// as whole structs (RunState::quiet_end), and the device-side copies the scope owns: always the bounds slot records the last walk
// folded, the rest by option.  What a build leaves otherwise -- the sorted copies and splitter samples of THIS state, the tree
// itself -- only changes the splitters of the next bucket sort, whose result is the same permutation whatever the splitters (the
// keys carry the body index, so there are no ties).
enum : unsigned {
    kQuietCounters = 1,    // the walk counters of bh_stats (from `visits` on; keys_kernel and let_box_kernel clear them) are kept
    kQuietOutputs = 2,     // a force walk runs inside: force, body_counts and group_cost are swapped for the check's buffers
    kQuietCostPerm = 4,    // the permutation the last force walk's group costs are indexed through is kept for bh_orb_histogram
};

void swap_walk_outputs(bh_ctx *c) { std::swap(c->force, c->check_force); std::swap(c->body_counts, c->check_counts); std::swap(c->group_cost, c->check_cost); }
template <typename Body>
int quietly(bh_ctx *c, unsigned opts, Body body)
{
    constexpr size_t off = offsetof(TreeCounters, visits), ctr_bytes = sizeof(TreeCounters) - off, slot_doubles = (size_t)4 * kBoundSlots;
    if ((opts & kQuietCounters) && !c->ctr_save) { if (int rc = dev_alloc(c, &c->ctr_save, 1)) return rc; }
    if (!c->slots_save) { if (int rc = dev_alloc(c, &c->slots_save, slot_doubles)) return rc; }
    RunState saved = *c;
    if ((opts & kQuietCostPerm) && c->last.group_cost_valid && c->is.tree_valid && !c->last.cost_perm && c->n > 0) {
        if (!c->perm_save) { if (int rc = dev_alloc(c, &c->perm_save, (size_t)std::max<int64_t>(c->cfg.capacity, 1))) return rc; }
        BH_HIP(c, hipMemcpyAsync(c->perm_save, c->perm, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        saved.costs_indexed_through(c->perm_save);
    }
    if (opts & kQuietCounters) BH_HIP(c, hipMemcpyAsync((char *)c->ctr_save + off, (char *)c->ctr + off, ctr_bytes, hipMemcpyDeviceToDevice, c->stream));
    BH_HIP(c, hipMemcpyAsync(c->slots_save, c->bslots, slot_doubles * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (opts & kQuietOutputs) swap_walk_outputs(c);
    const int rc = body();
    if (opts & kQuietOutputs) swap_walk_outputs(c);
    c->quiet_end(saved);
    BH_HIP(c, hipMemcpyAsync(c->bslots, c->slots_save, slot_doubles * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (opts & kQuietCounters) BH_HIP(c, hipMemcpyAsync((char *)c->ctr + off, (char *)c->ctr_save + off, ctr_bytes, hipMemcpyDeviceToDevice, c->stream));
    return rc;
}

}  // namespace

// the analysis queries: moment maps, radial profiles, azimuthal modes, the rotation curve, field at points, neighbours, pair counts,
// groups, spanning trees -- and the helpers they share, which the diagnostics and the disc below use as well
#include "bh_queries_host.hpp"

// ================================================================================================

extern "C" {

int bh_abi_version(void) { return BHGPU_ABI_VERSION; }

#ifndef BHGPU_BUILD_INFO
#define BHGPU_BUILD_INFO "digest=unknown flags=unknown"
#endif
const char *bh_build_info(void) { return BHGPU_BUILD_INFO; }

const char *bh_last_error(const bh_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int bh_create(const bh_config *cfg, bh_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, BH_ERR_ARG, "bh_create: null argument");
    *out = nullptr;
    if (cfg->capacity < 0 || cfg->capacity > 0x7fffffffLL - 8)
        return fail(nullptr, BH_ERR_ARG, "bh_create: capacity out of range");
    if (cfg->max_depth < 1 || cfg->max_depth > 32)
        return fail(nullptr, BH_ERR_ARG, "bh_create: max_depth must be 1..32");
    if (!(cfg->theta > 0.0)) return fail(nullptr, BH_ERR_ARG, "bh_create: theta must be > 0");
    if (cfg->precision != BH_PRECISION_F64_EXACT && cfg->precision != BH_PRECISION_F32 &&
        cfg->precision != BH_PRECISION_MIXED && cfg->precision != BH_PRECISION_F64)
        return fail(nullptr, BH_ERR_ARG, "bh_create: unknown precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, BH_ERR_NO_DEVICE, "bh_create: no HIP device (libbhgpu has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, BH_ERR_ARG, "bh_create: device ordinal out of range");

    bh_ctx *c = new bh_ctx();
    c->cfg = *cfg;
    c->Dm = cfg->max_depth - 1;
    c->mode = cfg->precision == BH_PRECISION_F64_EXACT ? Mode::Exact
            : cfg->precision == BH_PRECISION_F64       ? Mode::F64
            : cfg->precision == BH_PRECISION_MIXED     ? Mode::Mixed : Mode::F32;
    c->compat = cfg->reference_compat != 0;
    c->device = cfg->device;
    if (const char *e = std::getenv("BH_WALK_SPLIT")) c->walk_split = std::atoi(e);
    if (const char *e = std::getenv("BH_EXACT_BPW")) { const int b = std::atoi(e); c->exact_bpw = (b >= 1 && b <= kWave && (b & (b - 1)) == 0) ? b : 0; }
    if (const char *e = std::getenv("BH_WALK_ASM")) c->walk_asm = std::atoi(e) != 0;
    if (const char *e = std::getenv("BH_EXACT_BFS_MAX")) c->bfs_max = std::max(0, std::atoi(e));
    c->exact_thresholds = c->mode == Mode::Exact && c->walk_asm && !(cfg->flags & BH_FLAG_WALK_PORTABLE);
    if (const char *e = std::getenv("BH_SORT_PACK")) c->sort_pack = std::atoi(e) != 0;
    if (const char *e = std::getenv("BH_SORT_BUCKET")) c->sort_bucket = std::atoi(e);
    if (const char *e = std::getenv("BH_SORT_DIRECT")) { const int d = std::atoi(e); c->sort_direct = (d >= 0 && d <= 2) ? d : 1; }
    if (const char *e = std::getenv("BH_SORT_DIRECT_MAX")) c->sort_direct_max = std::max<long long>(0, std::atoll(e));
    if (c->tree64()) c->sort_direct = 0;
    if (const char *e = std::getenv("BH_BUILD_ITEMS")) c->build_items = std::atoi(e);
    if (const char *e = std::getenv("BH_REORDER_EVERY")) c->reorder_every = std::max(0, std::atoi(e));
    c->hilbert = !c->tree64();
    if (const char *e = std::getenv("BH_HILBERT")) c->hilbert = !c->tree64() && std::atoi(e) != 0;
    if (const char *e = std::getenv("BH_CHAIN_COLLAPSE")) c->chain_collapse = std::atoi(e) != 0;
    if (const char *e = std::getenv("BH_SORT_PLACE")) c->sort_place = std::atoi(e) != 0;
    if (const char *e = std::getenv("BH_RADIAL_BLOCKS")) { const int b = std::atoi(e); if (b >= 1 && b <= 65536) c->rad.blocks = b; }
    if (const char *e = std::getenv("BH_LISTS_ENTRIES")) { const long long b = std::atoll(e); if (b >= 1) c->nbl.budget = b; }
    if (const char *e = std::getenv("BH_LISTS_SORT_LDS")) { const int b = std::atoi(e); if (b >= 2 && b <= kNblMaxLds) c->nbl.sort_lds = b; }
    auto bail = [&](int rc) { g_create_error = c->err; bh_destroy(c); return rc; };

    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return bail(BH_ERR_DEVICE); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->err = "hipStreamCreate failed"; return bail(BH_ERR_DEVICE);
    }
    c->own_stream = true;

    const int64_t cap = std::max<int64_t>(cfg->capacity, 1);
    c->node_cap = cfg->node_capacity > 0 ? cfg->node_capacity : 8 * cap + 1024;
    // a depth-capped tree can never exceed the full tree (QUADTREE_MAX_SIZE, project.cu:62)
    if (c->Dm < 15) {
        int64_t full = 0, wdt = 1;
        for (int l = 0; l <= c->Dm; ++l) { full += wdt; wdt *= 4; }
        c->node_cap = std::min(c->node_cap, std::max<int64_t>(full, 1));
    }
    c->internal_cap = (c->node_cap - 1) / 4;

    const size_t rs = c->state64() ? sizeof(double) : sizeof(float);
    int rc = 0;
    auto A = [&](auto **pp, size_t count) { if (!rc) rc = dev_alloc(c, pp, count); };
    { char *t; A(&t, cap * 2 * rs); c->pos = t; }
    { char *t; A(&t, cap * 2 * rs); c->vel = t; }
    { char *t; A(&t, cap * rs); c->mass = t; }
    { char *t; A(&t, force_bytes(c, cap)); c->force = t; }
    if (!c->tree64()) {
        { char *t; A(&t, cap * 2 * rs); c->pos2 = t; }
        { char *t; A(&t, cap * 2 * rs); c->vel2 = t; }
        { char *t; A(&t, cap * rs); c->mass2 = t; }
        { char *t; A(&t, cap * 2 * sizeof(float)); c->force2 = t; }
        A(&c->orig, cap); A(&c->orig2, cap);
    }
    A(&c->keys[0], cap); A(&c->keys[1], cap); A(&c->vals[0], cap); A(&c->vals[1], cap);
    A(&c->cnt, cap + 1);
    { const size_t nbl = std::max<size_t>(blocks_for(cap, kSortTile), blocks_for(std::min<int64_t>(cap, 1 << 22), kBlock * kSmallItems));
      // (the bucket pass of launches above 1M bodies counts 1,024 buckets per tile; sized for the SMALLEST tile that
      // can reach it -- BH_BUILD_ITEMS=2 is honoured up to 4M bodies: 2 words per body, 32 MB at 4M -- ADVICE r2:
      // sized for kSortTile only, the 512-key tiles of that override wrote past the end between 1M and 4M bodies)
      const size_t big = (cap > kBucketMaxN) ? (size_t)kBucketsBig * blocks_for(std::min<int64_t>(cap, kBucketMaxNBig), kBlock * kSmallItems) : 0;
      A(&c->radix_counts, std::max<size_t>((size_t)(1 << kSortBits) * nbl, big));
      A(&c->bsum_sort, 2 * kBucketStartOffset);               // bucket totals, then bucket starts
      A(&c->splitters, kBucketsBig);
      A(&c->sort_dig, (size_t)std::min<int64_t>(cap, kBucketMaxNBig) + 16);
      A(&c->sort_paths, 2 * kBucketsBig);
      if (c->sort_direct) {
          const int64_t most = std::min<int64_t>(cap, kBucketMaxNBig);        // (larger launches take the LSD passes)
          c->direct_cap = (uint32_t)std::min<int64_t>(most, c->sort_direct == 2 ? most : c->sort_direct_max);
          // adaptive: kDirectSubs lists, each with room for four times its share of T (a power of two, at least 16 -- and so at
          // least T where T is small); every body listed: one list
          c->direct_nsub = c->sort_direct == 2 ? 1 : kDirectSubs;
          c->direct_subcap = c->direct_cap;
          if (c->sort_direct != 2) { c->direct_subcap = 16; while ((int64_t)c->direct_subcap * (kDirectSubs / 4) < c->direct_cap) c->direct_subcap *= 2; }
          A(&c->keys_scatter, (size_t)most);
          A(&c->direct_list, std::max<size_t>((size_t)c->direct_nsub * c->direct_subcap, 1));
          A(&c->direct_range_keys, kBucketsBig);
          A(&c->direct_count, 2 * kDirectCounterWords);
      }
    }
    // scan scratch (bsum_u32, bsum_d3): one record per scan tile, sized for the smallest tile
    const size_t scan_tiles = std::max<size_t>(blocks_for(cap + 1, kTile), blocks_for(std::min<int64_t>(cap, 1 << 22) + 1, kBlock * kSmallItems)) + 8;
    A(&c->bsum_u32, scan_tiles);
    A(&c->partial, 4 * (std::max<size_t>(1024, blocks_for(cap, kWave)) + 2));   // (LET mode only: the records of bh_let_bounds)
    A(&c->box, 8); A(&c->bslots, 4 * kBoundSlots);
    A(&c->ctr, 1);
    if (c->tree64()) {
        // (node 0 is the root, the four children of cell r are nodes 1 + 4 r ..: the arrays start three records into their
        // allocations, so that a sibling quad -- 128 bytes of NodeD, 32 of LinkD, what one visit of the fp64 walks loads -- is ONE
        // aligned 128-byte line and half a 64-byte line instead of straddling two and two: profiles/r04_f64/walk_traffic.json
        // read 1.85x the algorithmic bytes before)
        { NodeD *g0 = nullptr; LinkD *l0 = nullptr; A(&g0, c->node_cap + 4); A(&l0, c->node_cap + 4);
          if (!rc) { c->gd = g0 + 3; c->ld = l0 + 3; } }
        A(&c->self_node, c->internal_cap + 1); A(&c->com_pending, c->internal_cap + 1); A(&c->cell_depth, c->internal_cap + 1);
        A(&c->cell_first, c->internal_cap + 1);
    } else {
        A(&c->qf, c->internal_cap + 1); A(&c->aux, 4 * (c->internal_cap + 1));
        A(&c->cell_first, c->internal_cap + 1);
        A(&c->gid, cap); A(&c->group_cost, cap / kWave + 2); A(&c->walk_consts, 4);
        A(&c->coarse, cap / 256 + 2);
        A(&c->spos, cap); A(&c->sstate, cap + 64 * kBlock + 1024); A(&c->smass, cap);
        A(&c->terms, cap + 1); A(&c->bsum_d3, scan_tiles);
    }
    if (rc) return bail(rc);
    if (hipMemset(c->ctr, 0, sizeof(TreeCounters)) != hipSuccess) { c->err = "hipMemset failed"; return bail(BH_ERR_DEVICE); }
    if (hipMemset(c->sort_paths, 0, 2 * kBucketsBig * sizeof(uint32_t)) != hipSuccess) { c->err = "hipMemset failed"; return bail(BH_ERR_DEVICE); }
    if (c->direct_count && hipMemset(c->direct_count, 0, 2 * kDirectCounterWords * sizeof(uint32_t)) != hipSuccess) { c->err = "hipMemset failed"; return bail(BH_ERR_DEVICE); }
    if (!c->tree64()) {
        const void *wc[4] = {c->aux, c->spos, c->smass, nullptr};
        if (hipMemcpy(c->walk_consts, wc, sizeof(wc), hipMemcpyHostToDevice) != hipSuccess) { c->err = "hipMemcpy failed"; return bail(BH_ERR_DEVICE); }
    }
    if (!c->tree64() && c->exp.create(cap) != hipSuccess) { c->err = "experiment hooks: allocation failed"; return bail(BH_ERR_DEVICE); }
    auto create = [](auto &evs) { for (auto &e : evs) if (hipEventCreate(&e) != hipSuccess) return false; return true; };
    if (!create(c->ev_step) || !create(c->ev_build) || !create(c->ev_grp) || !create(c->ev_let)) {
        c->err = "hipEventCreate failed"; return bail(BH_ERR_DEVICE);
    }
    *out = c;
    return BH_OK;
}

void bh_destroy(bh_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->exp.destroy(c->n);
    for (void *p : c->allocs) (void)hipFree(p);
    auto destroy = [](auto &evs) { for (auto e : evs) if (e) (void)hipEventDestroy(e); };
    destroy(c->ev); destroy(c->ev_step); destroy(c->ev_build); destroy(c->ev_grp); destroy(c->ev_let); destroy(c->nb.ev);
    destroy(c->fof.ev); destroy(c->rad.ev); destroy(c->mod.ev); destroy(c->disc.ev); destroy(c->mst.ev); destroy(c->bin.ev); destroy(c->nbl.ev);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bh_set_softening(bh_ctx *c, double eps)
{
    if (!c) return BH_ERR_ARG;
    if (!(eps >= 0.0) || !std::isfinite(eps))
        return fail(c, BH_ERR_ARG, "bh_set_softening: the softening length must be finite and >= 0");
    if (eps != 0.0 && c->mode == Mode::Exact)
        return fail(c, BH_ERR_ARG, "bh_set_softening: BH_PRECISION_F64_EXACT reproduces the reference's results bit for bit and the "
                                   "reference has no softening -- use BH_PRECISION_F64, MIXED or F32 for a softened run");
    const double eps2 = eps * eps;
    if (!std::isfinite(eps2)) return fail(c, BH_ERR_ARG, "bh_set_softening: the square of the softening length overflows");
    c->law_changed(eps != c->eps);      // (phi holds the potential of another law until it is recomputed)
    c->eps = eps;
    c->eps2 = eps2;
    c->eps2f = (float)eps2;             // (0.f for a tiny eps: the fp32 walks then run their unsoftened kernels)
    return BH_OK;
}

int bh_get_softening(bh_ctx *c, double *eps)
{
    if (!c || !eps) return fail(c, BH_ERR_ARG, "bh_get_softening: null argument");
    *eps = c->eps;
    return BH_OK;
}

int bh_set_stream(bh_ctx *c, void *hip_stream)
{
    if (!c) return BH_ERR_ARG;
    BH_HIP(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = static_cast<hipStream_t>(hip_stream);
    c->own_stream = false;
    return BH_OK;
}

int bh_upload(bh_ctx *c, const double *pos, const double *vel, const double *mass, int64_t n)
{
    if (!c) return BH_ERR_ARG;
    if (n < 0 || (n > 0 && (!pos || !vel || !mass))) return fail(c, BH_ERR_ARG, "bh_upload: null array");
    if (n > c->cfg.capacity)
        return fail(c, BH_ERR_ARG, "Requested number of bodies exceeds N_BODIES.");   // project.cu:110-112
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    if (c->state64()) {
        BH_HIP(c, hipMemcpy(c->pos, pos, n * 2 * sizeof(double), hipMemcpyHostToDevice));
        BH_HIP(c, hipMemcpy(c->vel, vel, n * 2 * sizeof(double), hipMemcpyHostToDevice));
        BH_HIP(c, hipMemcpy(c->mass, mass, n * sizeof(double), hipMemcpyHostToDevice));
    } else {
        std::vector<float> t(std::max<int64_t>(2 * n, 1));
        for (int64_t i = 0; i < 2 * n; ++i) t[i] = (float)pos[i];
        BH_HIP(c, hipMemcpy(c->pos, t.data(), n * 2 * sizeof(float), hipMemcpyHostToDevice));
        for (int64_t i = 0; i < 2 * n; ++i) t[i] = (float)vel[i];
        BH_HIP(c, hipMemcpy(c->vel, t.data(), n * 2 * sizeof(float), hipMemcpyHostToDevice));
        for (int64_t i = 0; i < n; ++i) t[i] = (float)mass[i];
        BH_HIP(c, hipMemcpy(c->mass, t.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    BH_HIP(c, hipMemset(c->force, 0, force_bytes(c, n)));
    return upload_done(c, n);
}

static int download_pairs(bh_ctx *c, const void *dev, double *host, int64_t count, bool is64)
{
    if (is64) {
        BH_HIP(c, hipMemcpy(host, dev, count * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        std::vector<float> t(std::max<int64_t>(count, 1));
        BH_HIP(c, hipMemcpy(t.data(), dev, count * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < count; ++i) host[i] = (double)t[i];
    }
    return BH_OK;
}

// one uint32 per body, read from the device in DEVICE order -> out in caller order
static int counts_to_caller_order(bh_ctx *c, const uint32_t *dev_counts, uint32_t *out)
{
    BH_HIP(c, hipMemcpy(out, dev_counts, c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return to_caller_order(c, out, 1);
}

// a state array (`per` values per body) -> host, caller order
static int download_state(bh_ctx *c, const void *dev, double *host, int per)
{
    int rc = download_pairs(c, dev, host, per * c->n, c->state64());
    return rc ? rc : to_caller_order(c, host, per);
}

int bh_initialize(bh_ctx *c, int64_t n, uint64_t seed, int32_t kind, double lower_m, double higher_m,
                  double lower_p, double higher_p, double lower_v, double higher_v)
{
    if (!c) return BH_ERR_ARG;
    if (n < 0 || n > c->cfg.capacity)
        return fail(c, BH_ERR_ARG, "Requested number of bodies exceeds N_BODIES.");
    if (kind != 0 && kind != 1) return fail(c, BH_ERR_ARG, "bh_initialize: kind must be 0 (box) or 1 (plummer)");
    if (kind == 1) {               // kind 0 stays as permissive as generateRandomGpu; a Plummer sphere of these is NaN or garbage
        if (!(std::isfinite(lower_p) && lower_p > 0))
            return fail(c, BH_ERR_ARG, "bh_initialize: plummer scale lower_p must be finite and > 0");
        if (!(higher_p > 0))       // +inf: untruncated
            return fail(c, BH_ERR_ARG, "bh_initialize: plummer truncation radius higher_p must be > 0 (+inf: none)");
        if (!std::isfinite(higher_m)) return fail(c, BH_ERR_ARG, "bh_initialize: plummer mass higher_m must be finite");
    }
    BH_HIP(c, hipSetDevice(c->device));
    if (n > 0) {
        const unsigned g = blocks_for(n, kBlock);
        with_state(c, [&](auto r2) {
            using Real2 = decltype(r2);
            using Real = decltype(r2.x);
            hipLaunchKernelGGL((init_bodies_kernel<Real2, Real>), dim3(g), dim3(kBlock), 0, c->stream, (Real2 *)c->pos,
                               (Real2 *)c->vel, (Real *)c->mass, n, seed, kind, lower_m, higher_m, lower_p, higher_p, lower_v,
                               higher_v);
        });
        BH_HIP(c, hipGetLastError());
    }
    BH_HIP(c, hipMemsetAsync(c->force, 0, force_bytes(c, n), c->stream));
    return upload_done(c, n);
}

int bh_download_masses(bh_ctx *c, double *mass)
{
    if (!c || !mass) return fail(c, BH_ERR_ARG, "bh_download_masses: null array");
    if (int rc = need_upload(c, "bh_download_masses before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    return download_state(c, c->mass, mass, 1);
}

int bh_sync(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    BH_HIP(c, hipSetDevice(c->device));
    // also reports a tree that outgrew node_capacity during bh_step (the walk of such a step does
    // nothing, so the state is the last good one)
    if (c->is.tree_valid) return check_overflow(c);
    BH_HIP(c, hipStreamSynchronize(c->stream));
    return BH_OK;
}

int bh_download(bh_ctx *c, double *pos, double *vel)
{
    if (!c || !pos) return fail(c, BH_ERR_ARG, "bh_download: null array");
    if (int rc = need_upload(c, "bh_download before bh_upload")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    int rc = c->is.tree_valid ? check_overflow(c) : BH_OK;
    if (rc) return rc;
    BH_HIP(c, hipStreamSynchronize(c->stream));
    rc = download_state(c, c->pos, pos, 2);
    return rc || !vel ? rc : download_state(c, c->vel, vel, 2);
}

int bh_build_tree(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (int rc = need_upload(c, "bh_build_tree before bh_upload")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    c->forces_outdated();                    // (a build that is not quiet: no force walk follows it)
    int rc = enqueue_build(c);
    if (rc) return rc;
    return check_overflow(c);
}

int bh_compute_forces(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (int rc = need_upload(c, "bh_compute_forces before bh_upload")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    int rc = enqueue_build(c);
    if (!rc) rc = enqueue_walk(c, false, false);
    if (!rc) rc = check_overflow(c);
    c->forces_computed(rc == BH_OK && forces_cover_all(c));        // (not current either when any of the three failed)
    return rc;
}

// the events of a batch of `nsteps` timed steps: one pair per step around the walk kernel (bounded pool); returns how many
// steps get a pair through *want
static int step_events(bh_ctx *c, int32_t nsteps, int *want)
{
    *want = std::min<int>(nsteps, 4096);
    while ((int)c->ev.size() < 2 * *want) {
        hipEvent_t e;
        BH_HIP(c, hipEventCreate(&e));
        c->ev.push_back(e);
    }
    return BH_OK;
}

// step s of a batch of nsteps: the build and the walk with their events (the last step's build carries the group times)
static int enqueue_timed_step(bh_ctx *c, int s, int nsteps, int want, bool integrate)
{
    if (s == nsteps - 1) BH_HIP(c, hipEventRecord(c->ev_build[0], c->stream));
    int rc = enqueue_build(c, true, s == nsteps - 1);
    if (rc) return rc;
    if (s == nsteps - 1) BH_HIP(c, hipEventRecord(c->ev_build[1], c->stream));
    if (s < want) BH_HIP(c, hipEventRecord(c->ev[2 * s], c->stream));
    rc = enqueue_walk(c, integrate, false);
    if (rc) return rc;
    if (s < want) BH_HIP(c, hipEventRecord(c->ev[2 * s + 1], c->stream));
    return BH_OK;
}

static void steps_enqueued(bh_ctx *c, int32_t nsteps, int want)
{
    c->steps_done += nsteps;
    c->last_nsteps = nsteps;
    c->timed_pairs = want;
    c->step_timed = nsteps > 0;
}

int bh_step(bh_ctx *c, int32_t nsteps)
{
    if (!c || nsteps < 0) return BH_ERR_ARG;
    if (int rc = need_upload(c, "bh_step before bh_upload")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    int want = 0;
    if (int rc = step_events(c, nsteps, &want)) return rc;
    BH_HIP(c, hipEventRecord(c->ev_step[0], c->stream));
    for (int s = 0; s < nsteps; ++s)
        if (int rc = enqueue_timed_step(c, s, nsteps, want, true)) return rc;
    BH_HIP(c, hipEventRecord(c->ev_step[1], c->stream));
    steps_enqueued(c, nsteps, want);
    return BH_OK;
}

// ---- the split operators (bh_split.hpp): kick, drift, the time-step criterion, and the leapfrog built from them
int bh_forces_current(bh_ctx *c, int32_t *current)
{
    if (!c || !current) return fail(c, BH_ERR_ARG, "bh_forces_current: null argument");
    *current = c->is.forces_current ? 1 : 0;
    return BH_OK;
}

// v += a h on the force buffer; h == 0 launches nothing
static int enqueue_kick(bh_ctx *c, double h)
{
    const int64_t n = c->n;
    if (n == 0 || h == 0.0) return BH_OK;
    const dim3 grid(blocks_for(n, kBlock)), block(kBlock);
    switch (c->mode) {
    case Mode::F32:
        hipLaunchKernelGGL(kick_f32_kernel, grid, block, 0, c->stream, (const float2 *)c->force, (float2 *)c->vel, n, (float)h);
        break;
    case Mode::Mixed:
        hipLaunchKernelGGL(kick_mixed_kernel, grid, block, 0, c->stream, (const float2 *)c->force, (double2 *)c->vel, n, h);
        break;
    case Mode::F64:
        hipLaunchKernelGGL(kick_f64_kernel, grid, block, 0, c->stream, (const double2 *)c->force, (const double *)c->mass,
                           (double2 *)c->vel, n, h);
        break;
    case Mode::Exact:
        hipLaunchKernelGGL(kick_exact_kernel, grid, block, 0, c->stream, (const double2 *)c->force, (const double *)c->mass,
                           (double2 *)c->vel, n, h);
        break;
    }
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

// p += v h; whatever describes the old positions stops being current.  The bounds are NOT folded here: the next build takes
// its root box from bounds_partial (slots_valid = false).
static int enqueue_drift(bh_ctx *c, double h)
{
    const int64_t n = c->n;
    c->positions_moved_by_drift();
    if (n == 0 || h == 0.0) return BH_OK;
    const dim3 grid(blocks_for(n, kBlock)), block(kBlock);
    switch (c->mode) {
    case Mode::F32:
        hipLaunchKernelGGL(drift_f32_kernel, grid, block, 0, c->stream, (const float2 *)c->vel, (float2 *)c->pos, n, (float)h);
        break;
    case Mode::Mixed:
    case Mode::F64:
        hipLaunchKernelGGL(drift_f64_kernel, grid, block, 0, c->stream, (const double2 *)c->vel, (double2 *)c->pos, n, h);
        break;
    case Mode::Exact:
        hipLaunchKernelGGL(drift_exact_kernel, grid, block, 0, c->stream, (const double2 *)c->vel, (double2 *)c->pos, n, h);
        break;
    }
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

int bh_kick(bh_ctx *c, double h)
{
    if (!c) return BH_ERR_ARG;
    if (!std::isfinite(h)) return fail(c, BH_ERR_ARG, "bh_kick: h must be finite");
    if (int rc = split_check(c, "bh_kick")) return rc;
    if (int rc = need_forces(c, "bh_kick")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    return enqueue_kick(c, h);
}

int bh_drift(bh_ctx *c, double h)
{
    if (!c) return BH_ERR_ARG;
    if (!std::isfinite(h)) return fail(c, BH_ERR_ARG, "bh_drift: h must be finite");
    if (int rc = split_check(c, "bh_drift")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    return enqueue_drift(c, h);
}

int bh_timestep(bh_ctx *c, double eta, double length, bh_timestep_t *out)
{
    if (!c) return BH_ERR_ARG;
    if (!out) return fail(c, BH_ERR_ARG, "bh_timestep: null output");
    if (!std::isfinite(eta) || std::isnan(length)) return fail(c, BH_ERR_ARG, "bh_timestep: eta must be finite (and length a number)");
    if (int rc = split_check(c, "bh_timestep")) return rc;
    if (!(length > 0.0)) length = c->eps;                      // "use the softening length"
    if (!(length > 0.0) || !std::isfinite(length))
        return fail(c, BH_ERR_ARG, "bh_timestep: needs a finite length > 0, or a softening length to take its place");
    if (int rc = need_forces(c, "bh_timestep")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    if (!c->ts_part) { if (int rc = alloc_all(c, {part(&c->ts_part, (size_t)kTsParts), part(&c->ts_out, 1)})) return rc; }
    const uint32_t *orig = (c->tree64() || c->is.orig_identity) ? nullptr : c->orig;
    if (c->tree64())
        hipLaunchKernelGGL((timestep_partial_kernel<double2>), dim3(kTsParts), dim3(kBlock), 0, c->stream, (const double2 *)c->force,
                           (const double *)c->mass, orig, c->n, c->ts_part);
    else
        hipLaunchKernelGGL((timestep_partial_kernel<float2>), dim3(kTsParts), dim3(kBlock), 0, c->stream, (const float2 *)c->force,
                           (const double *)nullptr, orig, c->n, c->ts_part);
    hipLaunchKernelGGL(timestep_final_kernel, dim3(1), dim3(kBlock), 0, c->stream, c->ts_part, c->ts_out);
    BH_HIP(c, hipGetLastError());
    TsRecord r{};
    BH_HIP(c, hipMemcpyAsync(&r, c->ts_out, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    bh_timestep_t t{};
    t.n_bodies = c->n;
    if (r.a2 < 0.0) { t.a_max = 0.0; t.worst = -1; }           // no bodies
    else { t.a_max = std::sqrt(r.a2); t.worst = r.index; }
    t.dt = t.a_max == 0.0 ? (double)INFINITY : std::isinf(t.a_max) ? 0.0 : eta * std::sqrt(length / t.a_max);
    *out = t;
    return BH_OK;
}

// nsteps of kick-drift-kick at cfg.dt.  Between two drifts the two half kicks of neighbouring steps are one whole kick on
// the same forces, and a whole kick followed by the drift is the fused epilogue: so the inner nsteps - 1 steps ARE bh_step's
// (same kernels, same batch), between an opening half kick + drift and a closing force walk + half kick.
int bh_step_kdk(bh_ctx *c, int32_t nsteps)
{
    if (!c || nsteps < 0) return BH_ERR_ARG;
    if (int rc = split_check(c, "bh_step_kdk")) return rc;
    if (nsteps == 0) return BH_OK;
    BH_HIP(c, hipSetDevice(c->device));
    const double dt = c->cfg.dt;
    int want = 0;
    if (int rc = step_events(c, nsteps, &want)) return rc;
    BH_HIP(c, hipEventRecord(c->ev_step[0], c->stream));
    if (!c->is.forces_current) {                                  // (else: the closing forces of the previous call)
        int rc = enqueue_build(c);
        if (!rc) rc = enqueue_walk(c, false, false);
        if (rc) return rc;
    }
    if (int rc = enqueue_kick(c, 0.5 * dt)) return rc;
    if (int rc = enqueue_drift(c, dt)) return rc;
    for (int s = 0; s < nsteps; ++s)                           // the last one is the closing force walk
        if (int rc = enqueue_timed_step(c, s, nsteps, want, s < nsteps - 1)) return rc;
    if (int rc = enqueue_kick(c, 0.5 * dt)) return rc;
    BH_HIP(c, hipEventRecord(c->ev_step[1], c->stream));
    steps_enqueued(c, nsteps, want);
    c->forces_computed(forces_cover_all(c));
    return BH_OK;
}

// A walk's output `dev` holds forces (fp64 tree) or accelerations (fp32 / mixed); the other is converted with the masses
// (a = F / m_i: updateAccelerations, project.cu:795-801)
static int forces_or_accels(bh_ctx *c, const void *dev, double *out, bool forces)
{
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    int rc = download_pairs(c, dev, out, 2 * c->n, c->tree64());
    if (rc) return rc;
    if (forces != c->tree64()) {
        std::vector<double> m(std::max<int64_t>(c->n, 1));
        rc = download_pairs(c, c->mass, m.data(), c->n, c->state64());
        if (rc) return rc;
        for (int64_t i = 0; i < 2 * c->n; ++i) out[i] = forces ? out[i] * m[i / 2] : out[i] / m[i / 2];
    }
    return to_caller_order(c, out, 2);
}

int bh_get_forces(bh_ctx *c, double *out)
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_get_forces: null array");
    return forces_or_accels(c, c->force, out, true);
}

int bh_get_accel(bh_ctx *c, double *out)
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_get_accel: null array");
    return forces_or_accels(c, c->force, out, false);
}

int bh_get_interaction_counts(bh_ctx *c, uint32_t *out)
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_get_interaction_counts: null array");
    if (c->mode == Mode::Exact || !(c->cfg.flags & BH_FLAG_WALK_STATS) || !c->body_counts)
        return fail(c, BH_ERR_STATE, "bh_get_interaction_counts: fp32 / mixed / BH_PRECISION_F64 with BH_FLAG_WALK_STATS, after a walk");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    return counts_to_caller_order(c, c->body_counts, out);
}

// ---- the disc (bh_disc.hpp): what writes the state -- initial conditions, and velocities about a table, which write vel alone
// and change no record of bh_run_state.hpp, as bh_kick.  The rotation curve is a query: bh_queries_host.hpp, with disc_alloc.
int bh_initialize_disc(bh_ctx *c, int64_t n, uint64_t seed, double mass, double scale, double r_max)
{
    if (!c) return BH_ERR_ARG;
    if (n < 0 || n > c->cfg.capacity)
        return fail(c, BH_ERR_ARG, "Requested number of bodies exceeds N_BODIES.");
    if (!(std::isfinite(scale) && scale > 0)) return fail(c, BH_ERR_ARG, "bh_initialize_disc: scale must be finite and > 0");
    if (!(r_max > 0)) return fail(c, BH_ERR_ARG, "bh_initialize_disc: truncation radius r_max must be > 0 (+inf: none)");
    if (!std::isfinite(mass)) return fail(c, BH_ERR_ARG, "bh_initialize_disc: mass must be finite");
    BH_HIP(c, hipSetDevice(c->device));
    DiscState &s = c->disc;
    s.init_ms = 0.0;
    s.init_pending = false;
    if (n > 0) {
        const double F = std::isinf(r_max) ? 1.0 : 1.0 - scale / std::sqrt(r_max * r_max + scale * scale);
        const double m = mass / (double)n;
        if (int rc = mark(c, s.ev[0])) return rc;
        with_state(c, [&](auto r2) {
            using Real2 = decltype(r2);
            using Real = decltype(r2.x);
            hipLaunchKernelGGL((disc_init_kernel<Real2, Real>), dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, c->stream, (Real2 *)c->pos,
                               (Real2 *)c->vel, (Real *)c->mass, n, seed, scale, F, m);
        });
        BH_HIP(c, hipGetLastError());
        if (int rc = mark(c, s.ev[1])) return rc;
        s.init_pending = true;
    }
    BH_HIP(c, hipMemsetAsync(c->force, 0, force_bytes(c, n), c->stream));
    return upload_done(c, n);
}

int bh_set_disc_velocities(bh_ctx *c, const double *centre, const double *centre_vel, const double *radii, const double *vt,
                           const double *sigma_r, const double *sigma_t, int32_t k, uint64_t seed)
{
    if (!c) return BH_ERR_ARG;
    if (!radii || !vt || !sigma_r || !sigma_t) return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: null table");
    RadCentre ctr{};
    if (int rc = rad_centre(c, "bh_set_disc_velocities", centre, centre_vel, &ctr)) return rc;
    if (k < 1 || k > kDiscMaxTable)
        return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: k must be 1 .. BH_DISC_MAX_TABLE = " + std::to_string(kDiscMaxTable));
    std::vector<double> tab((size_t)kDiscTables * k);
    for (int32_t j = 0; j < k; ++j) {
        const double r = radii[j], r2 = r * r;
        if (!(std::isfinite(r) && std::isfinite(r2) && r >= 0.0))
            return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: a radius (or its square) is not finite or is negative");
        if (j > 0 && !(radii[j - 1] < r && tab[(size_t)j - 1] < r2))
            return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: the radii and their squares must be strictly ascending");
        if (!(std::isfinite(vt[j]) && std::isfinite(sigma_r[j]) && std::isfinite(sigma_t[j])))
            return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: a table entry is not finite");
        if (sigma_r[j] < 0.0 || sigma_t[j] < 0.0) return fail(c, BH_ERR_ARG, "bh_set_disc_velocities: a dispersion is negative");
        tab[(size_t)j] = r2; tab[(size_t)k + j] = r; tab[(size_t)2 * k + j] = vt[j]; tab[(size_t)3 * k + j] = sigma_r[j];
        tab[(size_t)4 * k + j] = sigma_t[j];
    }
    if (int rc = split_check(c, "bh_set_disc_velocities")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = disc_alloc(c)) return rc;
    DiscState &s = c->disc;
    s.vel_ms = 0.0;
    if (c->n == 0) return BH_OK;
    if (int rc = mark(c, s.ev[6])) return rc;
    BH_HIP(c, hipMemcpyAsync(s.tables, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const uint32_t *orig = (c->tree64() || c->is.orig_identity) ? nullptr : c->orig;
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        hipLaunchKernelGGL((disc_velocities_kernel<Real2>), dim3(rad_grid(c)), dim3(kBlock), tab.size() * sizeof(double), c->stream,
                           (const Real2 *)c->pos, (Real2 *)c->vel, orig, c->n, ctr, seed, s.tables, (int)k);
    });
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[7])) return rc;
    BH_HIP(c, hipStreamSynchronize(c->stream));                  // (tab lives on this stack until the copy has run)
    return span_ms(c, s.ev[6], s.ev[7], &s.vel_ms);
}

int bh_disc_times(bh_ctx *c, double *init_ms, double *curve_max_ms, double *curve_deposit_ms, double *velocities_ms)
{
    if (!c || !init_ms || !curve_max_ms || !curve_deposit_ms || !velocities_ms) return fail(c, BH_ERR_ARG, "bh_disc_times: null argument");
    DiscState &s = c->disc;
    if (s.init_pending) {                                          // bh_initialize_disc does not wait for its kernel: this does
        BH_HIP(c, hipSetDevice(c->device));
        BH_HIP(c, hipStreamSynchronize(c->stream));
        if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.init_ms)) return rc;
        s.init_pending = false;
    }
    *init_ms = s.init_ms;
    *curve_max_ms = s.max_ms;
    *curve_deposit_ms = s.deposit_ms;
    *velocities_ms = s.vel_ms;
    return BH_OK;
}

// ---- diagnostics (bh_diag.hpp): potential walk and reductions
// A tree of the current state is built in a quiet scope (quietly) for the potential walk and the force check.
// The walk writes phi and its own term counts only: force, body_counts, group_cost, partial, the event timings and
// walk_launches are not touched.
static int diag_alloc(bh_ctx *c)
{
    if (c->phi) return BH_OK;
    const size_t cap = (size_t)std::max<int64_t>(c->cfg.capacity, 1);
    return alloc_all(c, {part(&c->phi, cap), part(&c->phi_counts, cap), part(&c->diag_part, (size_t)kDiagParts * 2 * kDiagQuantities),
                         part(&c->diag_out, (size_t)kDiagQuantities)});
}

static int enqueue_potential(bh_ctx *c)
{
    // (false: bh_stats after a potential on a BH_FLAG_WALK_STATS context reads zero walk counters -- as it always has)
    if (int rc = quietly(c, 0, [&] { return enqueue_build(c, false); })) return rc;
    if (c->n == 0) return BH_OK;
    const unsigned grid = blocks_for(c->n, kBlock);
    if (c->tree64()) {
        const double2 *pos = static_cast<const double2 *>(c->pos);
        const int accept = c->mode == Mode::F64 ? kAcceptThr : c->exact_thresholds ? kAcceptExactThr : kAcceptSize;
        dispatch([&](auto compat) {
            constexpr bool CP = decltype(compat)::value;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, c->stream, c->gd, c->ld, c->perm, pos, c->n, c->cfg.theta,
                                   c->cfg.G, c->eps2, c->ctr, c->phi, c->phi_counts);
            };
            if (accept == kAcceptThr) go(potential_f64_kernel<CP, kAcceptThr>);
            else if (accept == kAcceptExactThr) go(potential_f64_kernel<CP, kAcceptExactThr>);
            else go(potential_f64_kernel<CP, kAcceptSize>);
        }, c->compat);
    } else {
        hipLaunchKernelGGL(potential_f32_kernel, dim3(grid), dim3(kBlock), 0, c->stream, c->qf, c->aux, c->spos, c->smass, c->perm,
                           c->n, c->cfg.G, c->eps2f, c->ctr, c->phi, c->phi_counts);
    }
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

int bh_compute_potential(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (int rc = diag_check(c, "bh_compute_potential")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    int rc = diag_alloc(c);
    if (!rc) rc = enqueue_potential(c);
    if (!rc) rc = check_overflow(c);
    c->potential_computed(rc == BH_OK);
    return rc;
}

// phi and, if asked for, its term counts in caller order; `stale`: the error text when phi is not the current state's
static int download_potential(bh_ctx *c, double *phi, uint32_t *counts, const char *stale)
{
    if (!c->is.phi_current) return fail(c, BH_ERR_STATE, stale);
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t n = c->n;
    if (n == 0) return BH_OK;
    BH_HIP(c, hipMemcpy(phi, c->phi, n * sizeof(double), hipMemcpyDeviceToHost));
    int rc = to_caller_order(c, phi, 1);
    if (rc || !counts) return rc;
    return counts_to_caller_order(c, c->phi_counts, counts);
}

int bh_get_potential(bh_ctx *c, double *phi, uint32_t *counts)
{
    if (!c || !phi) return fail(c, BH_ERR_ARG, "bh_get_potential: null array");
    if (int rc = diag_check(c, "bh_get_potential")) return rc;
    return download_potential(c, phi, counts, "bh_get_potential: no potential of the current state (bh_compute_potential)");
}

// the eight sums of bh_diag.hpp over the state and phi, in the two fixed-shape passes: q on the host when this returns
static int energy_sums(bh_ctx *c, double (&q)[kDiagQuantities])
{
    state_ptrs(c, [&](auto pos, auto vel, auto mass) {
        hipLaunchKernelGGL((energy_partial_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(kDiagParts), dim3(kBlock), 0,
                           c->stream, pos, vel, mass, c->phi, c->n, c->diag_part);
    });
    hipLaunchKernelGGL(energy_final_kernel, dim3(1), dim3(kBlock), 0, c->stream, c->diag_part, c->diag_out);
    BH_HIP(c, hipGetLastError());
    BH_HIP(c, hipMemcpyAsync(q, c->diag_out, sizeof(q), hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    return BH_OK;
}

int bh_energy(bh_ctx *c, bh_energy_t *out)
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_energy: null argument");
    if (int rc = diag_check(c, "bh_energy")) return rc;
    if (!c->is.phi_current) { if (int rc = bh_compute_potential(c)) return rc; }
    BH_HIP(c, hipSetDevice(c->device));
    double q[kDiagQuantities];
    if (int rc = energy_sums(c, q)) return rc;
    bh_energy_t e{};
    e.mass = q[0];
    e.com[0] = q[0] != 0.0 ? q[1] / q[0] : 0.0;
    e.com[1] = q[0] != 0.0 ? q[2] / q[0] : 0.0;
    e.momentum[0] = q[3]; e.momentum[1] = q[4];
    e.angular_momentum = q[5];
    e.kinetic = 0.5 * q[6];
    e.potential = 0.5 * q[7];
    e.total = e.kinetic + e.potential;
    e.n_bodies = c->n;
    *out = e;
    return BH_OK;
}

// ---- direct sums and the Barnes-Hut force check (bh_direct.hpp)
// The direct kernel reads the state only.  The check's tree forces come from a quiet build (quietly) and the
// precision's own force walk (enqueue_walk, not integrating: n_threads applies as in a step) with the walk's outputs --
// force, body_counts, group_cost -- swapped for scratch buffers, and walk_launches, group_cost_valid and the walk counters of
// bh_stats put back: bh_get_forces, bh_get_interaction_counts, bh_stats and the ORB weights still describe the last real
// force walk, and a following bh_step runs bit for bit as it would have.
static int check_targets(bh_ctx *c, const char *what, const int64_t *targets, int64_t n_targets)
{
    if (targets) {
        for (int64_t t = 0; t < n_targets; ++t)
            if (targets[t] < 0 || targets[t] >= c->n)
                return fail(c, BH_ERR_ARG, std::string(what) + ": target " + std::to_string(targets[t]) + " outside [0, n)");
    } else if (n_targets != c->n) {
        return fail(c, BH_ERR_ARG, std::string(what) + ": targets == NULL takes all n bodies (n_targets must be n)");
    }
    return BH_OK;
}

// out[n_targets][2]: the direct-sum forces of the targets (NULL: bodies 0 .. n_targets-1), launches of up to capacity targets
static int direct_forces_host(bh_ctx *c, const int64_t *targets, int64_t n_targets, double *out)
{
    if (n_targets == 0) return BH_OK;
    const int64_t chunk = std::max<int64_t>(c->cfg.capacity, 1);
    if (!c->direct_out) { if (int rc = alloc_all(c, {part(&c->direct_targets, (size_t)chunk), part(&c->direct_out, (size_t)chunk)})) return rc; }
    const uint32_t *slot_of = nullptr;
    if (!c->tree64() && !c->is.orig_identity) {            // (fp32 / mixed after a physical re-order: slots are not caller indices)
        if (!c->slot_of) { if (int rc = dev_alloc(c, &c->slot_of, (size_t)chunk)) return rc; }
        hipLaunchKernelGGL(direct_slot_kernel, dim3(blocks_for(c->n, kBlock)), dim3(kBlock), 0, c->stream, c->orig, c->n, c->slot_of);
        slot_of = c->slot_of;
    }
    for (int64_t t0 = 0; t0 < n_targets; t0 += chunk) {
        const int64_t k = std::min(chunk, n_targets - t0);
        if (targets) BH_HIP(c, hipMemcpyAsync(c->direct_targets, targets + t0, k * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        const int64_t *tg = targets ? c->direct_targets : nullptr;
        state_ptrs(c, [&](auto pos, auto, auto mass) {
            hipLaunchKernelGGL((direct_forces_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(blocks_for(k, kBlock)),
                               dim3(kBlock), 0, c->stream, pos, mass, slot_of, tg, t0, k, c->n, c->cfg.G, c->eps2, c->direct_out);
        });
        BH_HIP(c, hipGetLastError());
        BH_HIP(c, hipMemcpyAsync(out + 2 * t0, c->direct_out, k * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        BH_HIP(c, hipStreamSynchronize(c->stream));
    }
    return BH_OK;
}

// the check walk's tree forces (caller order, all n) into out[n][2]
static int check_walk(bh_ctx *c, double *out)
{
    const size_t cap = (size_t)std::max<int64_t>(c->cfg.capacity, 1);
    int rc = BH_OK;
    if (!c->check_force) {
        char *f = nullptr;
        rc = dev_alloc(c, &f, force_bytes(c, (int64_t)cap));
        c->check_force = f;
        if (!rc && c->group_cost) rc = dev_alloc(c, &c->check_cost, cap / kWave + 2);
        if (rc) return rc;
    }
    if ((c->cfg.flags & BH_FLAG_WALK_STATS) && !c->check_counts) { if ((rc = dev_alloc(c, &c->check_counts, cap))) return rc; }
    // (the check's walk counts as well: its counters are kept around build and walk together)
    rc = quietly(c, kQuietCounters | kQuietOutputs, [&] {
        const int r = enqueue_build(c, false);
        return r ? r : enqueue_walk(c, false, false);
    });
    if (!rc) rc = check_overflow(c);
    return rc ? rc : forces_or_accels(c, c->check_force, out, true);
}

int bh_direct_forces(bh_ctx *c, const int64_t *targets, int64_t n_targets, double *forces)
{
    if (!c) return BH_ERR_ARG;
    if (!forces || n_targets < 0) return fail(c, BH_ERR_ARG, "bh_direct_forces: null output array or n_targets < 0");
    if (int rc = diag_check(c, "bh_direct_forces")) return rc;
    if (int rc = check_targets(c, "bh_direct_forces", targets, n_targets)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    return direct_forces_host(c, targets, n_targets, forces);
}

int bh_force_check(bh_ctx *c, const int64_t *targets, int64_t n_targets, double *tree, double *direct)
{
    if (!c) return BH_ERR_ARG;
    if (!tree || !direct || n_targets < 0) return fail(c, BH_ERR_ARG, "bh_force_check: null output array or n_targets < 0");
    if (int rc = diag_check(c, "bh_force_check")) return rc;
    if (int rc = check_targets(c, "bh_force_check", targets, n_targets)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    std::vector<double> all((size_t)std::max<int64_t>(2 * c->n, 1));
    if (int rc = check_walk(c, all.data())) return rc;
    for (int64_t t = 0; t < n_targets; ++t) {
        const int64_t i = targets ? targets[t] : t;
        tree[2 * t] = all[2 * i]; tree[2 * t + 1] = all[2 * i + 1];
    }
    return direct_forces_host(c, targets, n_targets, direct);
}

// ---- tree export: DFS pre-order, children in index order (TraverseTreeToFile, project.cu:504-534)
static int export_tree_host(bh_ctx *c, std::vector<bh_tree_node> &out, std::vector<int32_t> &depth)
{
    if (!c->is.tree_valid) return fail(c, BH_ERR_STATE, "no tree built yet");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    TreeCounters h{};
    BH_HIP(c, hipMemcpy(&h, c->ctr, sizeof(h), hipMemcpyDeviceToHost));
    if (h.overflow || (int64_t)h.n_internal > c->internal_cap) return fail(c, BH_ERR_CAPACITY, "tree overflowed node_capacity");
    const int64_t nn = 1 + 4 * (int64_t)h.n_internal;
    double box[4];
    BH_HIP(c, hipMemcpy(box, c->box, sizeof(box), hipMemcpyDeviceToHost));
    std::vector<NodeD> gd;
    std::vector<LinkD> ld;
    std::vector<QuadF> qf;
    std::vector<NodeAux> aux;
    std::vector<uint32_t> perm(std::max<int64_t>(c->n, 1));
    if (c->n > 0) BH_HIP(c, hipMemcpy(perm.data(), c->perm, c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!c->tree64() && !c->is.orig_identity && c->n > 0) {          // slots -> the caller's body indices
        std::vector<uint32_t> o(c->n);
        BH_HIP(c, hipMemcpy(o.data(), c->orig, c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (auto &b : perm) b = o[b];
    }
    if (c->tree64()) {
        gd.resize(nn); ld.resize(nn);
        BH_HIP(c, hipMemcpy(gd.data(), c->gd, nn * sizeof(NodeD), hipMemcpyDeviceToHost));
        BH_HIP(c, hipMemcpy(ld.data(), c->ld, nn * sizeof(LinkD), hipMemcpyDeviceToHost));
    } else {
        const int64_t nq = (int64_t)h.n_internal + 1;      // quad 0 = root
        if (!c->is.aux_full && c->n > 0) {                    // the step's node kernel writes bucket records only
            launch_nodes_fast(c, true, c->stream);
            c->all_node_records_written();
            BH_HIP(c, hipGetLastError());
            BH_HIP(c, hipStreamSynchronize(c->stream));
        }
        qf.resize(nq); aux.resize(4 * nq);
        BH_HIP(c, hipMemcpy(qf.data(), c->qf, nq * sizeof(QuadF), hipMemcpyDeviceToHost));
        BH_HIP(c, hipMemcpy(aux.data(), c->aux, 4 * nq * sizeof(NodeAux), hipMemcpyDeviceToHost));
    }
    struct Item { int32_t node; int32_t depth; int64_t parent_out; int slot; double x0, x1, y0, y1; int state; };
    std::vector<Item> stack;
    stack.push_back({0, 0, -1, 0, box[0], box[1], box[2], box[3], 0});
    out.clear(); depth.clear();
    out.reserve(nn); depth.reserve(nn);
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const int64_t node_limit = c->tree64() ? nn : 4 * ((int64_t)h.n_internal + 1);
        if (it.node < 0 || it.node >= node_limit) return fail(c, BH_ERR_DEVICE, "corrupt child link in device tree");
        bh_tree_node q{};
        int32_t child;       // id of child 0, or -1
        if (c->tree64()) {
            q.comx = gd[it.node].cx; q.comy = gd[it.node].cy; q.mass = gd[it.node].m;
            q.particle = (double)ld[it.node].occ;
            child = ld[it.node].child;
        } else {
            const QuadF &f = qf[it.node >> 2];
            const int sl = it.node & 3;
            const NodeAux &ax = aux[it.node];
            q.comx = f.xy[2 * sl]; q.comy = f.xy[2 * sl + 1]; q.mass = f.m[sl];
            child = f.child[sl] >= 1 ? 4 * f.child[sl] : -1;
            if (child < 0 && ax.count == 1) {      // single occupant: the reference's PARTICLE_INDEX
                const int64_t body = perm[ax.first];
                q.particle = (it.depth == c->Dm) ? (double)(-body - 2) : (double)body;
            } else q.particle = -1.0;
        }
        q.xmin = it.x0; q.xmax = it.x1; q.ymin = it.y0; q.ymax = it.y1;
        for (int k = 0; k < 4; ++k) q.child[k] = -1.0;
        const int64_t me = (int64_t)out.size();
        if (it.parent_out >= 0) out[it.parent_out].child[it.slot] = (double)me;
        out.push_back(q);
        depth.push_back(it.depth);
        if (child >= 0) {
            const double mx = (it.x0 + it.x1) / 2.0, my = (it.y0 + it.y1) / 2.0;
            for (int k = 3; k >= 0; --k) {          // push reversed: child 0 is visited first
                // k is the GEOMETRIC child index (the reference's order); with Hilbert keys the
                // sibling sits in slot H[state][k] of the quad
                const int slot = c->hilbert ? hilbert_digit(it.state, k) : k;
                Item ch{child + slot, it.depth + 1, me, k,
                        (k & 1) ? mx : it.x0, (k & 1) ? it.x1 : mx,
                        (k & 2) ? my : it.y0, (k & 2) ? it.y1 : my,
                        c->hilbert ? hilbert_next(it.state, k) : 0};
                stack.push_back(ch);
            }
        }
    }
    return BH_OK;
}

int bh_export_tree(bh_ctx *c, bh_tree_node *nodes, int32_t *depth, int64_t cap, int64_t *n_nodes)
{
    if (!c || !n_nodes) return fail(c, BH_ERR_ARG, "bh_export_tree: null argument");
    std::vector<bh_tree_node> out;
    std::vector<int32_t> dep;
    int rc = export_tree_host(c, out, dep);
    if (rc) return rc;
    *n_nodes = (int64_t)out.size();
    if (!nodes || cap < (int64_t)out.size()) return fail(c, BH_ERR_CAPACITY, "bh_export_tree: buffer too small");
    std::memcpy(nodes, out.data(), out.size() * sizeof(bh_tree_node));
    if (depth) std::memcpy(depth, dep.data(), dep.size() * sizeof(int32_t));
    return BH_OK;
}

int bh_write_quadtree_file(bh_ctx *c, const char *path)
{
    if (!c || !path) return fail(c, BH_ERR_ARG, "bh_write_quadtree_file: null argument");
    std::vector<bh_tree_node> out;
    std::vector<int32_t> dep;
    int rc = export_tree_host(c, out, dep);
    if (rc) return rc;
    std::vector<double> pos(std::max<int64_t>(2 * c->n, 2));
    rc = download_state(c, c->pos, pos.data(), 2);
    if (rc) return rc;
    FILE *fp = std::fopen(path, "w");
    if (!fp) return fail(c, BH_ERR_IO, std::string("cannot open ") + path);
    for (size_t i = 0; i < out.size(); ++i) {
        const bh_tree_node &q = out[i];
        // `file << depth << " " << xmin ...` with the default ostream precision == "%g"
        std::fprintf(fp, "%d %g %g %g %g %g", dep[i], q.xmin, q.xmax, q.ymin, q.ymax, q.mass);
        const long long occ = (long long)q.particle;
        if (occ != -1) {
            const long long b = occ >= 0 ? occ : -(occ + 2);   // the reference reads out of bounds here
            std::fprintf(fp, " occupantIndex=%lld occupantPos=(%g,%g)", occ, pos[2 * b], pos[2 * b + 1]);
        } else if (q.mass > 0) {
            std::fprintf(fp, " occupantIndex=%lld occupantPos=(%g,%g)", occ, q.comx, q.comy);
        }
        std::fputc('\n', fp);
    }
    std::fclose(fp);
    return BH_OK;
}

int bh_stats(bh_ctx *c, bh_stats_t *out)
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_stats: null argument");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    std::memset(out, 0, sizeof(*out));
    out->n_bodies = c->n;
    out->steps_done = c->steps_done;
    out->walk_launches = (uint64_t)c->last.walk_launches;
    out->device_bytes = c->device_bytes;
    TreeCounters h{};
    BH_HIP(c, hipMemcpy(&h, c->ctr, sizeof(h), hipMemcpyDeviceToHost));
    out->sort_spill_buckets = h.sort_spills;
    out->sort_rerun_buckets = h.sort_reruns;
    if (c->is.tree_valid) {
        out->n_internal = h.n_internal;
        out->n_nodes = 1 + 4 * (int64_t)h.n_internal;
        out->visits = h.visits;
        out->interactions = h.interactions;
        out->wave_nodes = h.wave_nodes;
        out->wave_quads = h.wave_quads;
        out->wave_accepts = h.wave_accepts;
    }
    if (c->let_timed) {
        float ms = 0.f;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_let[0], c->ev_let[1])); out->let_tree_ms = ms;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_let[1], c->ev_let[2])); out->let_pack_ms = ms;
    }
    if (c->step_timed) {
        float ms = 0.f;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_step[0], c->ev_step[1]));
        out->last_step_ms = (double)ms / std::max(1, c->last_nsteps);
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_build[0], c->ev_build[1]));
        out->build_ms = ms;
        double acc = 0.0;
        for (int s = 0; s < c->timed_pairs; ++s) {
            BH_HIP(c, hipEventElapsedTime(&ms, c->ev[2 * s], c->ev[2 * s + 1]));
            acc += ms;
        }
        out->walk_ms = c->timed_pairs ? acc / c->timed_pairs : 0.0;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_build[0], c->ev_grp[0])); out->keys_ms = ms;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_grp[0], c->ev_grp[1])); out->sort_ms = ms;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_grp[1], c->ev_grp[2])); out->scan_ms = ms;
        BH_HIP(c, hipEventElapsedTime(&ms, c->ev_grp[2], c->ev_build[1])); out->nodes_ms = ms;
        // algorithmic bytes per body of one build.  keys: position in, key (+ index) out;
        // sort: per LSD pass 8 (histogram) + 16 (scatter of packed keys; 24 with a separate index array), or the
        // bucket sort's 9 + 17 + 20 (histogram + bucket byte, scatter, in-LDS sort with the unpacked write-out);
        // prep: key, index, position and mass in, count and sorted copies out (+ 24 of prefix-sum terms when the
        // state is fp64); scans: counts in and out, cell starts, terms -> prefix sums; nodes: ~0.72 cells per body,
        // each reading its key window share, ranks and five prefix sums and writing an 80-byte quad
        const int passes = (2 * c->Dm + kSortBits - 1) / kSortBits;
        const uint64_t keys_b = (c->state64() ? 24u : 16u) + (c->last.last_sort_packed ? 0u : 4u);
        const uint64_t sort_b = c->last.last_sort_bucket ? 46u : (uint64_t)passes * (c->last.last_sort_packed ? 24u : 32u);
        const uint64_t prep_b = c->state64() ? 76u : 40u, scan_b = c->state64() ? 59u : 47u, nodes_b = c->tree64() ? 140u : 117u;
        out->build_bytes = (uint64_t)c->n * (keys_b + sort_b + prep_b + scan_b + nodes_b);
        out->walk_bytes = out->wave_nodes ? (uint64_t)c->n * 44u + out->wave_nodes * 20u : 0u;
    }
    return BH_OK;
}

// How the in-LDS bucket sorts ended so far: out[0] buckets finished by placement, out[1] buckets that went through byte passes
// (cumulative since bh_create; bh_sort.hpp "Placement").  The workgroup of bucket b counts in words of its own -- 256 atomics
// on one word at the end of every bucket's chain cost the kernel 2.5 us --, summed here.  A wait and a copy, no launch.
int bh_sort_paths(bh_ctx *c, uint64_t out[2])
{
    if (!c || !out) return fail(c, BH_ERR_ARG, "bh_sort_paths: null argument");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> h((size_t)2 * kBucketsBig);
    BH_HIP(c, hipMemcpy(h.data(), c->sort_paths, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    out[0] = out[1] = 0;
    for (int b = 0; b < kBucketsBig; ++b) { out[0] += h[(size_t)b]; out[1] += h[(size_t)kBucketsBig + b]; }
    return BH_OK;
}

// What the last build's sort was given, decided and wrote: plain copies after a wait, no launch, no event of the run state.
// Nothing between the sort and the next build writes keys[0] of a build that was offered direct input (its output is keys[1] /
// vals[1], the counting pass scatters into keys_scatter); bh_migrate_pack does, and a LET context is refused for it.
int bh_sort_snapshot(bh_ctx *c, int64_t info[8], uint32_t *decision, uint64_t *range_keys, uint64_t *list, uint64_t *keys_in,
                     uint64_t *keys_sorted, uint32_t *perm)
{
    if (!c || !info) return fail(c, BH_ERR_ARG, "bh_sort_snapshot: null argument");
    if (c->let_mode) return fail(c, BH_ERR_STATE, "bh_sort_snapshot: not in LET mode (bh_migrate_pack reuses the sort's buffers)");
    if (!c->is.tree_valid || !c->sort_rec.valid) return fail(c, BH_ERR_STATE, "bh_sort_snapshot: no build to report (build a tree first)");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    const bh_ctx::SortRecord &r = c->sort_rec;
    const int64_t out[8] = {r.offered ? 1 : 0, r.n, r.nb, (int64_t)r.len, (int64_t)r.cap, (int64_t)r.subcap, r.nsub, kDirectSubs};
    for (int k = 0; k < 8; ++k) info[k] = out[k];
    const size_t n = (size_t)r.n;
    if (n > 0 && keys_sorted) BH_HIP(c, hipMemcpy(keys_sorted, c->keys_sorted, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n > 0 && perm) BH_HIP(c, hipMemcpy(perm, c->perm, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!r.offered) return BH_OK;
    if (decision) {
        std::vector<uint32_t> block((size_t)kDirectCounterWords);
        BH_HIP(c, hipMemcpy(block.data(), r.count, block.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int k = 0; k <= kDirectSubs; ++k) decision[k] = block[(size_t)kDirectStride * (size_t)k];
    }
    if (range_keys) BH_HIP(c, hipMemcpy(range_keys, c->direct_range_keys, (size_t)r.nb * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (list) BH_HIP(c, hipMemcpy(list, c->direct_list, (size_t)r.nsub * r.subcap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (keys_in) BH_HIP(c, hipMemcpy(keys_in, c->keys[0], n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_step_times(bh_ctx *c, double *step_ms, double *walk_ms, int32_t cap, int32_t *n_out)
{
    if (!c || !n_out) return fail(c, BH_ERR_ARG, "bh_step_times: null argument");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    const int n = c->step_timed ? c->timed_pairs : 0;
    *n_out = n;
    if (cap < n) return (step_ms || walk_ms) ? fail(c, BH_ERR_CAPACITY, "bh_step_times: buffer too small") : BH_OK;
    for (int s = 0; s < n; ++s) {
        float ms = 0.f;
        if (walk_ms) { BH_HIP(c, hipEventElapsedTime(&ms, c->ev[2 * s], c->ev[2 * s + 1])); walk_ms[s] = ms; }
        // a step ends where its walk ends; the first one starts where bh_step started
        if (step_ms) { BH_HIP(c, hipEventElapsedTime(&ms, s ? c->ev[2 * s - 1] : c->ev_step[0], c->ev[2 * s + 1])); step_ms[s] = ms; }
    }
    return BH_OK;
}

// ---- multi-GPU plumbing -------------------------------------------------------------------------
int bh_set_owned_fraction(bh_ctx *c, int32_t rank, int32_t world)
{
    if (!c || world < 1 || world > 64 || rank < 0 || rank >= world) return fail(c, BH_ERR_ARG, "bh_set_owned_fraction: bad rank/world (world <= 64)");
    c->rank = rank;
    c->world = world;
    return BH_OK;
}

int bh_owned_range(bh_ctx *c, int64_t *lo, int64_t *hi)
{
    if (!c || !lo || !hi) return BH_ERR_ARG;
    owned_range(c, lo, hi);
    return BH_OK;
}

int bh_device_state(bh_ctx *c, void **pos, void **vel, void **mass, int64_t *n, int32_t *elem_bytes)
{
    if (!c) return BH_ERR_ARG;
    if (pos) *pos = c->pos;
    if (vel) *vel = c->vel;
    if (mass) *mass = c->mass;
    if (n) *n = c->n;
    if (elem_bytes) *elem_bytes = c->state64() ? 8 : 4;
    return BH_OK;
}

int bh_device_sorted(bh_ctx *c, void **sorted_state)
{
    if (!c) return BH_ERR_ARG;
    if (c->state64()) return fail(c, BH_ERR_STATE, "the sorted exchange buffer exists in fp32 mode only");
    if (sorted_state) *sorted_state = c->sstate;
    return BH_OK;
}

}  // extern "C"

namespace bh {
__global__ __launch_bounds__(kBlock) void scatter_sorted_kernel(const uint32_t *__restrict__ perm,
                                                                 const float4 *__restrict__ sstate,
                                                                 float2 *__restrict__ pos,
                                                                 float2 *__restrict__ vel, int64_t n)
{
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t b = perm[s];
    const float4 t = sstate[s];
    pos[b] = float2{t.x, t.y};
    vel[b] = float2{t.z, t.w};
}
}  // namespace bh

extern "C" {

int bh_step_local(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (int rc = need_upload(c, "bh_step_local before bh_upload")) return rc;
    if (c->state64()) return fail(c, BH_ERR_STATE, "bh_step_local: fp32 mode only");
    BH_HIP(c, hipSetDevice(c->device));
    int rc = enqueue_build(c);
    if (rc) return rc;
    return enqueue_walk(c, true, true);
}

int bh_scatter_sorted(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (c->state64()) return fail(c, BH_ERR_STATE, "bh_scatter_sorted: fp32 mode only");
    BH_HIP(c, hipSetDevice(c->device));
    if (c->n > 0) {
        hipLaunchKernelGGL(scatter_sorted_kernel, dim3(blocks_for(c->n, kBlock)), dim3(kBlock), 0, c->stream,
                           c->perm, c->sstate, (float2 *)c->pos, (float2 *)c->vel, c->n);
        BH_HIP(c, hipGetLastError());
    }
    c->positions_moved_by_scatter();
    c->steps_done += 1;
    return BH_OK;
}

// ---- distributed step with locally-essential trees --------------------------------------------------
int bh_let_local_quads(bh_ctx *c, int64_t *local_quads)
{
    if (!c || !local_quads) return fail(c, BH_ERR_ARG, "bh_let_local_quads: null argument");
    *local_quads = c->internal_cap + 1;
    return BH_OK;
}

int bh_let_configure(bh_ctx *c, int32_t rank, int32_t world, int64_t let_cap, int64_t forest_base)
{
    if (!c || world < 1 || world > kMaxWorld || rank < 0 || rank >= world || let_cap < 1)
        return fail(c, BH_ERR_ARG, "bh_let_configure: bad rank/world/let_cap (world <= 64)");
    if (forest_base < c->internal_cap + 1)
        return fail(c, BH_ERR_ARG, "bh_let_configure: forest_base must be the LARGEST bh_let_local_quads of all ranks "
                                   "(a sender writes child links in the receiver's index space)");
    if (forest_base + (int64_t)world * let_cap > 0x7fffffffLL)
        return fail(c, BH_ERR_ARG, "bh_let_configure: forest too large for 32-bit quad indices");
    if (c->tree64()) return fail(c, BH_ERR_STATE, "bh_let_configure: fp32 and mixed precision only");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    int rc = 0;
    auto A = [&](auto **pp, size_t count) { if (!rc) rc = dev_alloc(c, pp, count); };
    if (c->let_mode) {
        // a second call may only change let_cap (LetStepper.autotune: size the blocks from measured counts)
        if (rank != c->rank || world != c->world || forest_base != c->forest_base)
            return fail(c, BH_ERR_STATE, "bh_let_configure: rank/world/forest_base cannot change once configured");
        if (let_cap == c->let_cap) return BH_OK;
        dev_free(c, c->qf); dev_free(c, c->let_send);
        c->qf = nullptr; c->let_send = nullptr;
    } else {
        c->rank = rank; c->world = world;
        c->quads_local = c->internal_cap + 1;
        dev_free(c, c->qf);              // the single-tree node array: the forest below replaces it
        c->qf = nullptr;
        A(&c->needmask, (size_t)c->quads_local);
        A(&c->let_tsum, (size_t)kMaxWorld);            // per-peer slot counters of the LET extraction
        A(&c->let_outidx, (size_t)world * c->quads_local);
        A(&c->lbounds, 4 * kLetBoxes); A(&c->all_bounds, 4 * kLetBoxes * (size_t)world);
        A(&c->acc_part, (size_t)std::max<int64_t>(c->cfg.capacity, 1));
        A(&c->let_ctr, 1);
    }
    c->let_cap = let_cap;
    c->forest_base = forest_base;
    A(&c->qf, (size_t)(forest_base + (int64_t)world * let_cap));
    A(&c->let_send, (size_t)world * let_cap);
    if (rc) return rc;
    BH_HIP(c, hipMemset(c->let_ctr, 0, sizeof(LetCounters)));
    BH_HIP(c, hipMemset(c->let_tsum, 0, kMaxWorld * sizeof(uint32_t)));
    BH_HIP(c, hipMemset(c->needmask, 0, (size_t)std::max<int64_t>(c->quads_local, 1) * sizeof(uint64_t)));
    c->let_mode = true;
    c->external_box = true;
    c->let_configured();
    return BH_OK;
}

// quiet (the scope's struct pair alone: nothing to copy on the device): the walk's records stay for the next bh_let_bounds (a
// step after the diagnostic describes itself by the same boxes)
static int let_bounds(bh_ctx *c, bool quiet, const char *who)
{
    if (int rc = let_check(c, who, kLetBodies)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    const RunState saved = *c;
    int count = c->carry.partial_count;
    if (count <= 0) {
        count = kLetBoxes * kLetBoxParts;
        with_state(c, [&](auto r2) {
            using Real2 = decltype(r2);
            hipLaunchKernelGGL((let_slice_bounds_kernel<Real2>), dim3((unsigned)count), dim3(kBlock), 0, c->stream, (const Real2 *)c->pos, c->n,
                               c->partial);
        });
    }
    hipLaunchKernelGGL(let_local_bounds_kernel, dim3(kLetBoxes), dim3(kWave), 0, c->stream, c->partial, count, c->lbounds);
    c->let_bounds_taken();
    if (quiet) c->quiet_end(saved);
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

int bh_let_bounds(bh_ctx *c) { return let_bounds(c, false, "bh_let_bounds"); }
int bh_let_bounds_quiet(bh_ctx *c) { return let_bounds(c, true, "bh_let_bounds_quiet"); }

int bh_let_pointers(bh_ctx *c, void **lbounds, void **all_bounds, void **send, void **recv, int64_t *block_bytes,
                    int32_t *boxes_per_rank)
{
    if (int rc = let_check(c, "bh_let_pointers", kLetConfigured)) return rc;
    if (lbounds) *lbounds = c->lbounds;
    if (all_bounds) *all_bounds = c->all_bounds;
    if (send) *send = c->let_send;
    if (recv) *recv = c->qf + c->forest_base;
    if (block_bytes) *block_bytes = c->let_cap * (int64_t)sizeof(QuadF);
    if (boxes_per_rank) *boxes_per_rank = kLetBoxes;
    return BH_OK;
}

// quiet (the distributed diagnostics): the whole call in a quiet scope -- the local tree without a re-order, build count and
// samples_n put back --, the walk counters of bh_stats copied aside and back (let_box_kernel clears them), the bh_let_build
// timings left alone (they are recorded outside a scope only), and the permutation the last force walk's group costs are indexed
// through kept for bh_orb_histogram.  The LET size counters take this build's sizes like any other's.
static int let_build(bh_ctx *c, bool quiet, const char *who)
{
    if (int rc = let_check(c, who, kLetBodies)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto stamp = [&](int i) { if (!quiet) (void)hipEventRecord(c->ev_let[i], st); };
    auto body = [&]() -> int {
        stamp(0);
        hipLaunchKernelGGL(let_box_kernel, dim3(1), dim3(64), 0, st, c->all_bounds, c->world * kLetBoxes, c->box, c->ctr,
                           c->let_ctr, c->Dm);
        if (int rc = enqueue_build(c, !quiet)) return rc;
        stamp(1);
        const int64_t nq = c->quads_local;
        hipLaunchKernelGGL(let_mark_alloc_kernel, dim3(blocks_for(4 * nq, kBlock)), dim3(kBlock), 0, st, c->qf, c->all_bounds,
                           c->world, c->rank, c->ctr, c->internal_cap, c->needmask, c->let_tsum, c->let_outidx, nq);
        hipLaunchKernelGGL(let_pack_kernel, dim3(blocks_for(nq, kBlock)), dim3(kBlock), 0, st, c->qf, c->needmask,
                           c->let_outidx, nq, c->world, c->rank, c->ctr, c->internal_cap, c->let_send,
                           (uint32_t)c->let_cap, c->forest_base + (int64_t)c->rank * c->let_cap, c->let_tsum, c->let_ctr);
        stamp(2);
        return BH_OK;
    };
    if (int rc = quiet ? quietly(c, kQuietCounters | kQuietCostPerm, body) : body()) return rc;
    if (!quiet) c->let_timed = true;
    c->let_built();
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

int bh_let_build(bh_ctx *c) { return let_build(c, false, "bh_let_build"); }
int bh_let_build_quiet(bh_ctx *c) { return let_build(c, true, "bh_let_build_quiet"); }

// the walks of a built LET context; an integrating one is a step
static int let_walk(bh_ctx *c, const char *who, bool integrate, int part)
{
    if (int rc = let_check(c, who, kLetTree)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = enqueue_walk(c, integrate, false, part)) return rc;
    if (integrate) c->steps_done += 1;
    return BH_OK;
}

int bh_let_walk(bh_ctx *c) { return let_walk(c, "bh_let_walk", true, 0); }
int bh_let_forces(bh_ctx *c) { return let_walk(c, "bh_let_forces", false, 0); }
// The forest walk in two launches, so that the all_to_all of the LETs can run under the first:
// bh_let_walk_local needs only bh_let_build's local tree; bh_let_walk_remote needs the received
// blocks, adds their contribution and finishes the step (integrate != 0) or just the forces.
int bh_let_walk_local(bh_ctx *c) { return let_walk(c, "bh_let_walk_local", false, 1); }
int bh_let_walk_remote(bh_ctx *c, int32_t integrate) { return let_walk(c, "bh_let_walk_remote", integrate != 0, 2); }

// ---- diagnostics of the distributed step (bh_diag.hpp: forest_potential_f32_kernel and the reductions) ----------------
// The forest the last bh_let_build left and the caller completed with the peers' blocks, walked by the potential kernel: it
// writes phi and its own counts, so force, body_counts, group_cost, partial, the walk counters and the timings stay the last
// force walk's.
static int let_diag_check(bh_ctx *c, const char *what)
{
    return c->let_mode ? BH_OK : fail(c, BH_ERR_STATE, std::string(what) + ": LET mode only (bh_let_configure; BH_PRECISION_F32 / MIXED) -- "
                                                       "a single context has bh_compute_potential / bh_energy");
}

int bh_let_potential(bh_ctx *c)
{
    if (!c) return BH_ERR_ARG;
    if (int rc = let_diag_check(c, "bh_let_potential")) return rc;
    if (!c->is.tree_valid) return fail(c, BH_ERR_STATE, "bh_let_potential before bh_let_build");
    if (c->is.let_moved) return fail(c, BH_ERR_STATE, "bh_let_potential: the bodies have moved since the last bh_let_build");
    BH_HIP(c, hipSetDevice(c->device));
    int rc = diag_alloc(c);
    if (!rc && c->n > 0) {
        hipLaunchKernelGGL(forest_potential_f32_kernel, dim3(blocks_for(c->n, kBlock)), dim3(kBlock), 0, c->stream, c->qf, c->aux,
                           c->spos, c->smass, c->perm, c->n, c->cfg.G, c->eps2f, c->ctr, (int32_t)c->world, (int32_t)c->rank, c->forest_base,
                           c->let_cap, c->phi, c->phi_counts);
        BH_HIP(c, hipGetLastError());
    }
    if (!rc) rc = check_overflow(c);
    c->potential_computed(rc == BH_OK);
    return rc;
}

int bh_let_get_potential(bh_ctx *c, double *phi, uint32_t *counts)
{
    if (!c || !phi) return fail(c, BH_ERR_ARG, "bh_let_get_potential: null array");
    if (int rc = let_diag_check(c, "bh_let_get_potential")) return rc;
    return download_potential(c, phi, counts, "bh_let_get_potential: no potential of the current state (bh_let_potential)");
}

int bh_let_energy(bh_ctx *c, double *sums)
{
    if (!c || !sums) return fail(c, BH_ERR_ARG, "bh_let_energy: null argument");
    if (int rc = let_diag_check(c, "bh_let_energy")) return rc;
    if (!c->is.phi_current) { if (int rc = bh_let_potential(c)) return rc; }
    BH_HIP(c, hipSetDevice(c->device));
    double q[kDiagQuantities];
    if (int rc = energy_sums(c, q)) return rc;
    for (int k = 0; k < kDiagQuantities; ++k) sums[k] = q[k];
    return BH_OK;
}

// ---- device-side migration and re-balancing (bh_migrate.hpp) ----------------------------------------
int bh_set_ids(bh_ctx *c, const int64_t *ids)
{
    if (!c || !ids) return fail(c, BH_ERR_ARG, "bh_set_ids: null argument");
    if (!c->gid) return fail(c, BH_ERR_STATE, "bh_set_ids: fp32 and mixed precision only");
    if (int rc = need_upload(c, "bh_set_ids before bh_upload")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    BH_HIP(c, hipMemcpy(c->gid, ids, c->n * sizeof(int64_t), hipMemcpyHostToDevice));
    return BH_OK;
}

int bh_get_ids(bh_ctx *c, int64_t *ids)
{
    if (!c || !ids) return fail(c, BH_ERR_ARG, "bh_get_ids: null argument");
    if (!c->gid) return fail(c, BH_ERR_STATE, "bh_get_ids: fp32 and mixed precision only");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    BH_HIP(c, hipMemcpy(ids, c->gid, c->n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

static int check_cuts(bh_ctx *c, const bh_orb_cuts *cuts, const char *who)
{
    if (!c || !cuts) return fail(c, BH_ERR_ARG, std::string(who) + ": null argument");
    if (c->tree64()) return fail(c, BH_ERR_STATE, std::string(who) + ": fp32 and mixed precision only");
    if (int rc = need_upload(c, std::string(who) + " before bh_upload")) return rc;
    if (cuts->world < 1 || cuts->world > kMaxWorld || cuts->n_cuts != cuts->world - 1)
        return fail(c, BH_ERR_ARG, std::string(who) + ": world must be 1..64 and n_cuts = world - 1");
    return BH_OK;
}

int bh_orb_histogram(bh_ctx *c, const bh_orb_cuts *cuts, int32_t level, void **hist, int64_t *n_words)
{
    int rc = check_cuts(c, cuts, "bh_orb_histogram");
    if (rc) return rc;
    if (!hist || !n_words || level < 0) return fail(c, BH_ERR_ARG, "bh_orb_histogram: bad argument");
    BH_HIP(c, hipSetDevice(c->device));
    const size_t words = (size_t)std::max(cuts->n_cuts, 1) * BH_ORB_BINS;
    if (!c->orb_hist) {
        rc = dev_alloc(c, &c->orb_hist, (size_t)BH_ORB_MAX_CUTS * BH_ORB_BINS);
        if (rc) return rc;
    }
    BH_HIP(c, hipMemsetAsync(c->orb_hist, 0, words * sizeof(unsigned long long), c->stream));
    if (c->n > 0) {
        // weights: the cost of the body's 64-body group in the last full walk; they are indexed by sorted
        // position, so the bodies are visited through the last build's permutation
        const bool weighted = c->last.group_cost_valid && c->is.tree_valid;
        const uint32_t *perm = weighted ? (c->last.cost_perm ? c->last.cost_perm : c->perm) : nullptr;   // (the last force walk's order)
        const uint32_t *cost = weighted ? c->group_cost : nullptr;
        const unsigned g = blocks_for(c->n, kBlock);
        with_state(c, [&](auto r2) {
            using Real2 = decltype(r2);
            hipLaunchKernelGGL((orb_hist_kernel<Real2>), dim3(g), dim3(kBlock), 0, c->stream, (const Real2 *)c->pos, perm, cost,
                               c->n, *cuts, (int)level, c->orb_hist);
        });
        BH_HIP(c, hipGetLastError());
    }
    *hist = c->orb_hist;
    *n_words = (int64_t)words;
    return BH_OK;
}

static int migrate_buffers(bh_ctx *c)
{
    if (c->mig_send) return BH_OK;
    const size_t cap = (size_t)std::max<int64_t>(c->cfg.capacity, 1) * kMigrateRecord;
    int rc = dev_alloc(c, &c->mig_send, cap);
    if (!rc) rc = dev_alloc(c, &c->mig_recv, cap);
    return rc;
}

int bh_migrate_pack(bh_ctx *c, const bh_orb_cuts *cuts, int64_t *send_counts)
{
    int rc = check_cuts(c, cuts, "bh_migrate_pack");
    if (rc) return rc;
    if (!send_counts) return fail(c, BH_ERR_ARG, "bh_migrate_pack: null argument");
    BH_HIP(c, hipSetDevice(c->device));
    rc = migrate_buffers(c);
    if (rc) return rc;
    const int64_t n = c->n;
    const int W = cuts->world;
    for (int r = 0; r < W; ++r) send_counts[r] = 0;
    c->migration_packed();                                  // the sort buffers are reused from here on
    if (n == 0) { BH_HIP(c, hipStreamSynchronize(c->stream)); return BH_OK; }
    hipStream_t st = c->stream;
    const unsigned g = blocks_for(n, kBlock);
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        hipLaunchKernelGGL((migrate_classify_kernel<Real2>), dim3(g), dim3(kBlock), 0, st, (const Real2 *)c->pos, n, *cuts,
                           c->keys[0], c->vals[0]);
    });
    // one stable radix pass on the destination rank (< 64 < 256): slots grouped by destination, slot order kept
    const int cur = enqueue_lsd_passes<kSortItems>(st, c->keys, c->vals, c->radix_counts, c->bsum_sort, n, kSortBits, false);
    const uint32_t *orig = c->is.orig_identity ? nullptr : c->orig;
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        using Real = decltype(r2.x);
        hipLaunchKernelGGL((migrate_pack_kernel<Real2, Real>), dim3(g), dim3(kBlock), 0, st, c->vals[cur], (const Real2 *)c->pos,
                           (const Real2 *)c->vel, (const Real *)c->mass, orig, c->gid, n, c->mig_send);
    });
    BH_HIP(c, hipGetLastError());
    uint32_t totals[kMaxWorld];
    BH_HIP(c, hipMemcpyAsync(totals, c->bsum_sort, W * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    int64_t sum = 0;
    for (int r = 0; r < W; ++r) { send_counts[r] = totals[r]; sum += totals[r]; }
    if (sum != n) return fail(c, BH_ERR_DEVICE, "bh_migrate_pack: destination counts do not add up");
    return BH_OK;
}

int bh_migrate_pointers(bh_ctx *c, void **send, void **recv, int64_t *capacity_records)
{
    if (!c) return BH_ERR_ARG;
    if (c->tree64()) return fail(c, BH_ERR_STATE, "bh_migrate_pointers: fp32 and mixed precision only");
    BH_HIP(c, hipSetDevice(c->device));
    int rc = migrate_buffers(c);
    if (rc) return rc;
    if (send) *send = c->mig_send;
    if (recv) *recv = c->mig_recv;
    if (capacity_records) *capacity_records = std::max<int64_t>(c->cfg.capacity, 1);
    return BH_OK;
}

int bh_migrate_unpack(bh_ctx *c, int64_t n_new)
{
    if (!c) return BH_ERR_ARG;
    if (c->tree64() || !c->mig_recv) return fail(c, BH_ERR_STATE, "bh_migrate_unpack before bh_migrate_pack");
    if (n_new < 0 || n_new > c->cfg.capacity)
        return fail(c, BH_ERR_CAPACITY, "bh_migrate_unpack: " + std::to_string(n_new) + " bodies arrive, capacity is " +
                                        std::to_string(c->cfg.capacity));
    BH_HIP(c, hipSetDevice(c->device));
    if (n_new > 0) {
        const unsigned g = blocks_for(n_new, kBlock);
        with_state(c, [&](auto r2) {
            using Real2 = decltype(r2);
            using Real = decltype(r2.x);
            hipLaunchKernelGGL((migrate_unpack_kernel<Real2, Real>), dim3(g), dim3(kBlock), 0, c->stream, c->mig_recv, n_new,
                               (Real2 *)c->pos, (Real2 *)c->vel, (Real *)c->mass, (float2 *)c->force, c->gid);
        });
        BH_HIP(c, hipGetLastError());
    }
    c->n = n_new;
    c->bodies_replaced();                                     // (arrival order is the caller order from here on)
    return BH_OK;
}

int bh_let_counts(bh_ctx *c, uint32_t *counts, int32_t *overflow)
{
    if (!c || !c->let_mode || !counts) return fail(c, BH_ERR_STATE, "bh_let_counts: not in LET mode");
    BH_HIP(c, hipSetDevice(c->device));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    LetCounters h{};
    BH_HIP(c, hipMemcpy(&h, c->let_ctr, sizeof(h), hipMemcpyDeviceToHost));
    BH_HIP(c, hipMemset(c->let_ctr, 0, sizeof(LetCounters)));        // reading starts a new observation interval
    for (int r = 0; r < c->world; ++r) counts[r] = h.count[r];
    if (overflow) { *overflow = (int32_t)h.overflow; return BH_OK; }   // the caller inspects the flag
    if (h.overflow) return fail(c, BH_ERR_CAPACITY, "a locally-essential tree exceeded let_cap");
    return BH_OK;
}

}  // extern "C"

