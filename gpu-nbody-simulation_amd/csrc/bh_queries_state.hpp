// bh_queries_state.hpp -- what the context keeps for the analysis queries of bh_queries_host.hpp, one struct per family
// (bh_ctx has one member of each; DiscState serves the rotation curve there and bh_set_disc_velocities in bh_engine.hip).  Everything is allocated on first use and lives as long as the context.  Part of the
// bh_engine.hip translation unit, included there after the kernels' headers and before bh_ctx -- bh_queries_host.hpp needs the
// whole context and comes after it: hence a header of its own.
#pragma once

namespace bh {

// a grow-only device allocation carved into arrays for up to `cap` items (block_regrow)
struct DevBlock {
    char *base = nullptr;
    uint64_t bytes = 0;
    int64_t cap = 0;
};

// moment maps (bh_moments.hpp): the first pass's record, the body counter, and the 4-plane int64 grid, which grows to the
// largest map asked for (`cells` of them per plane)
struct MapState {
    MapMax *max = nullptr;
    unsigned long long *count = nullptr;
    long long *planes = nullptr;
    int64_t cells = 0;
};

// radial profiles and Lagrangian radii (bh_radial.hpp): the first pass's record, the select's flags, the squared edges, the
// 6-plane int64 profile of up to BH_RADIAL_MAX_BINS + 2 slots, a round's histograms
struct RadState {
    RadMax *max = nullptr;
    unsigned long long *flags = nullptr;
    double *e2 = nullptr;
    long long *planes = nullptr, *hist = nullptr;
    int blocks = 512;                  // BH_RADIAL_BLOCKS: most persistent workgroups of the radial kernels
    hipEvent_t ev[4 + 2 * kRadRounds] = {};                 // around the first pass, the deposit, and every select round
    double max_ms = 0.0, main_ms = 0.0, round_ms[kRadRounds] = {};     // of the last call (bh_radial_times)
};

// azimuthal modes (bh_modes.hpp): the first pass's record, the squared edges, and the int64 planes of up to kModMaxPlanes x
// (BH_MODES_MAX_BINS + 2) slots; the launch shape is the radial kernels' (rad.blocks)
struct ModState {
    ModMax *max = nullptr;
    double *e2 = nullptr;
    long long *planes = nullptr;
    hipEvent_t ev[4] = {};                                      // around the first pass and around the deposit
    double max_ms = 0.0, deposit_ms = 0.0;                      // of the last call (bh_modes_times)
};

// the disc (bh_disc.hpp): the rotation curve's first-pass record, squared edges and 5-plane int64 sums of up to
// BH_DISC_MAX_BINS + 2 slots, and the five tables of bh_set_disc_velocities; the launch shape is the radial kernels' (rad.blocks)
struct DiscState {
    DiscMax *max = nullptr;
    double *e2 = nullptr, *tables = nullptr;
    long long *planes = nullptr;
    hipEvent_t ev[8] = {};                                      // around the initialiser, the first pass, the deposit, the velocities
    bool init_pending = false;                                  // ev[0], ev[1] are recorded and not yet read (bh_initialize_disc does not wait)
    double init_ms = 0.0, max_ms = 0.0, deposit_ms = 0.0, vel_ms = 0.0;     // of the last call of each (bh_disc_times)
};

// the field at arbitrary points (bh_field.hpp): one block for a launch of up to block.cap points -- the points, their results, two
// key arrays and the sorted order, the sort's count matrix and row totals
struct FieldState {
    DevBlock block;
    double2 *points = nullptr, *accel = nullptr;
    uint64_t *keys[2] = {nullptr, nullptr};
    double *phi = nullptr;
    uint32_t *order = nullptr, *counts = nullptr, *radix = nullptr, *rows = nullptr;
};

// neighbour queries (bh_neighbours.hpp), grown as the field's block: one block for the search structure of up to block.cap
// bodies, one for a launch of up to qblock.cap queries with `entries` list entries in all.  Pair counts and groups build and search the
// same structure and mark the same events.
struct NbState {
    DevBlock block, qblock;
    int64_t entries = 0;
    uint64_t *keys[2] = {nullptr, nullptr}, *pkeys[2] = {nullptr, nullptr};
    uint32_t *slot = nullptr, *sidx = nullptr, *radix = nullptr, *rowsum = nullptr, *order = nullptr, *evals = nullptr;
    double2 *spos = nullptr, *points = nullptr;
    NbBox *boxes = nullptr;
    NbBounds *bounds = nullptr;
    double *box = nullptr, *d2 = nullptr;
    int32_t *off = nullptr;
    int64_t *idx = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};    // around the build and around a launch's sort and search
    double build_ms = 0.0, query_ms = 0.0;                      // of the last call (bh_neighbours_times)
};

// pair counts (bh_pairs.hpp): the squared edges, then the int64 histogram and the evals word
struct PairState {
    double *e2 = nullptr;
    unsigned long long *hist = nullptr;
    double build_ms = 0.0, query_ms = 0.0;                      // of the last call (bh_pair_counts_times)
};

// friends-of-friends groups (bh_groups.hpp): one block for up to block.cap bodies beside the neighbour structure's, and the
// catalogue of the last bh_groups call on the host (no record of bh_run_state.hpp: it is that call's result, whatever the run
// does afterwards)
struct FofState {
    DevBlock block;
    uint32_t *parent = nullptr, *root = nullptr, *minidx = nullptr, *count = nullptr, *rec_label = nullptr, *rec_count = nullptr;
    long long *label = nullptr;
    unsigned long long *sums = nullptr;
    GrpCounters *ctr = nullptr;
    GrpMax *max = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};                      // after the labels, after the catalogue
    double build_ms = 0.0, link_ms = 0.0, cat_ms = 0.0;         // of the last call (bh_groups_times)
    std::vector<int64_t> cat_labels, cat_counts, cat_sums;
    int32_t cat_exp[kGrpPlanes] = {0, 0, 0, 0, 0};
};

// spanning trees (bh_mst.hpp): one block for up to block.cap bodies beside the neighbour structure's -- the union-find, the
// components of bodies and nodes, the per-component minima, the lanes' candidates and the edges as they were appended --, and
// one for a launch of up to sblock.cap members of subsets with their edges
struct MstState {
    DevBlock block, sblock;
    uint32_t *parent = nullptr, *comp = nullptr, *inv = nullptr, *nodecomp = nullptr, *bad = nullptr;
    unsigned long long *seedmin = nullptr, *mind2 = nullptr, *minpair = nullptr, *cand_d2 = nullptr, *cand_pair = nullptr, *edge_pair = nullptr,
                       *edge_d2 = nullptr, *set_pair = nullptr;
    double *set_d2 = nullptr;
    int64_t *members = nullptr;
    MstCounters *ctr = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};                      // after the rounds, after the sort; subsets: around a launch
    double build_ms = 0.0, rounds_ms = 0.0, sort_ms = 0.0;      // of the last call (bh_spanning_tree_times)
};

// bound pairs (bh_binaries.hpp): one block for up to block.cap bodies beside the neighbour structure's -- the sorted velocities
// and masses, the nodes' mass bounds, the partners in caller order and as sorted positions, room for block.cap / 2 + 1 records --,
// and the catalogue of the last bh_binaries call on the host, ascending in lo (as FofState's: that call's result, whatever the
// run does afterwards)
struct BinState {
    DevBlock block;
    double2 *svel = nullptr;
    double *smass = nullptr, *nodemass = nullptr, *eps = nullptr, *rec = nullptr;
    int64_t *partner = nullptr;
    int32_t *psort = nullptr;
    uint32_t *rec_lo = nullptr, *rec_hi = nullptr;
    BinCounters *ctr = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};             // after the sorted copies and mass bounds, the search, the records
    double build_ms = 0.0, search_ms = 0.0, cat_ms = 0.0;       // of the last call (bh_binaries_times)
    std::vector<int64_t> cat_lo, cat_hi;
    std::vector<double> cat_rec;                                // kBinRecord doubles a record
};

// neighbour lists (bh_neighbour_lists.hpp) beside the neighbour structure's blocks: one block for a launch of up to block.cap
// queries (row lengths, cursors, evals, the per-query r2, the rows of the two sort kernels, the scan's tile totals), one for
// up to eblock.cap entries, and a second of that size once a row is sorted through global memory
struct NblState {
    DevBlock block, eblock, ablock;
    uint32_t *counts = nullptr, *evals = nullptr, *rows_lds = nullptr, *rows_merge = nullptr, *ent_idx = nullptr, *alt_idx = nullptr;
    int64_t *cursors = nullptr;
    double *rad2 = nullptr;
    uint64_t *tiles = nullptr;
    unsigned long long *ent_d2 = nullptr, *alt_d2 = nullptr;
    NblCounters *ctr = nullptr;
    int64_t budget = (int64_t)1 << 24;  // BH_LISTS_ENTRIES: most entries of a launch
    int sort_lds = 512;                 // BH_LISTS_SORT_LDS: the longest row the in-LDS sort takes
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};             // around a launch's scan and fill, and after its sorts
    double build_ms = 0.0, count_ms = 0.0, fill_ms = 0.0, sort_ms = 0.0;       // of the last call (bh_neighbour_lists_times)
    std::vector<uint32_t> evals_host;                           // per query, caller order: of the last filling call
};

}  // namespace bh
