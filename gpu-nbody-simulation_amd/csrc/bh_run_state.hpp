// bh_run_state.hpp -- what the engine's host code knows to be current, and the events that change it (the
// table of events against facts).  Plain C++, no HIP: tests/test_run_state_cpu.py replays the engine's call sequences on it with
// the host compiler.  bh_ctx embeds one RunState; bh_engine.hip reads the members anywhere and writes them through the events only.
#pragma once
#include <cstdint>

namespace bh {

struct Current {                   // what is current for the state in the arrays
    bool uploaded = false;         // the state arrays hold a body set (bh_upload / bh_initialize has run)
    bool tree_valid = false;       // a build has completed in these buffers and its counters may be read -- NOT "a tree of the
                                   // current positions": an integrating walk and bh_scatter_sorted keep it, a drift does not
    bool forces_current = false;   // the force buffer holds the accelerations (fp64 tree: the forces) of the CURRENT positions of
                                   // ALL bodies, slot for slot, under the current law (bh_split.hpp)
    bool phi_current = false;      // phi holds the potential of the current positions under the current law
    bool let_moved = false;        // an integrating walk has moved the bodies since the last bh_let_build (nothing else clears it)
    bool orig_identity = true;     // slot == caller index: no build has physically re-ordered this body set
    bool aux_full = false;         // aux[] holds every node's record (an export since the last build), not only the buckets'
};
struct BuildCarry {                // what the next build reads from the previous one
    int64_t builds = 0;            // builds of n > 0 bodies since the body set arrived: the re-order cadence
    int64_t samples_n = -1;        // spos (fp64 tree: perm) holds the sorted order of a build of this many bodies (-1: none)
    int partial_count = 0;         // LET mode, > 0: partial[] holds that many per-workgroup min/max records of the current positions
    bool slots_valid = false;      // the last walk folded the bounds of the current positions into bslots
    bool slots_dirty = true;       // bslots may hold something else than +-inf (written, not yet consumed by keys_kernel)
};
struct LastRun {                   // what the last real build and force walk report to the caller
    int64_t walk_launches = 0;     // walk kernel launches of the last force walk (bh_stats)
    const uint32_t *cost_perm = nullptr;   // non-null: group_cost is indexed through this, not through perm (a quiet LET build since)
    bool group_cost_valid = false; // group_cost holds the cost of every 64-body group in a walk over all bodies of this set
    bool last_sort_bucket = false, last_sort_packed = false;   // what the last build's sort was (bh_stats build_bytes)
};
struct BuildDone {                 // what a build did: n bodies; own_box: the root box came from the bounds slot records (false: LET
    int64_t n;                     // mode's external box); launched = false: the launches failed -- what was enqueued is recorded,
    bool own_box, sort_bucket, sort_packed, reordered, launched;   // tree_valid stays as it was
};

struct RunState {
    Current is;
    BuildCarry carry;
    LastRun last;

    // bh_migrate_unpack: another set of bodies in caller order; nothing an earlier build, walk or potential left describes them
    // (samples_n: the next build sorts with the LSD passes).  let_moved, aux_full, slots_dirty, walk_launches and the sort stay.
    void bodies_replaced()
    {
        carry.partial_count = 0; carry.slots_valid = false; carry.samples_n = -1; carry.builds = 0; last.group_cost_valid = false;
        is.phi_current = false; is.forces_current = false; is.tree_valid = false; is.orig_identity = true; last.cost_perm = nullptr;
    }
    void new_bodies() { bodies_replaced(); is.uploaded = true; }                 // bh_upload, bh_initialize
    // bh_set_softening: phi is another law's after ANY call, the forces only when the length changed
    void law_changed(bool value_changed) { if (value_changed) is.forces_current = false; is.phi_current = false; }
    // bh_build_tree: a build that may re-order the state, and no force walk after it
    void forces_outdated() { is.forces_current = false; }
    // every build, quiet or not (a quiet one is undone in carry and last by quiet_end, and keeps tree_valid and aux_full)
    void build_completed(const BuildDone &b)
    {
        last.cost_perm = nullptr;
        if (b.own_box) {       // n > 0: prep_kernel has put the records back to +-inf; else bounds_partial wrote them unless the walk had
            if (b.n > 0) carry.slots_dirty = false; else if (!carry.slots_valid) carry.slots_dirty = true;
            carry.slots_valid = false;
        }
        if (b.n > 0) { last.last_sort_bucket = b.sort_bucket; last.last_sort_packed = b.sort_packed; carry.builds += 1; carry.samples_n = b.n; }
        if (b.reordered) is.orig_identity = false;
        is.aux_full = false;
        if (b.launched) is.tree_valid = true;
    }
    void all_node_records_written() { is.aux_full = true; }                      // the export's second node pass
    // a force walk: its launches are counted from zero unless it continues the previous one (LET: the received trees' part)
    void walk_begins(bool continues) { if (!continues) last.walk_launches = 0; }
    void walk_launched() { last.walk_launches += 1; }
    void partials_recorded(int count) { carry.partial_count = count; }           // LET mode: the walk writes `partial`
    // an integrating walk; folded: its workgroups fold the bounds of the new positions into bslots.  tree_valid stays.
    void positions_moved_by_walk(bool folded)
    {
        carry.slots_valid = folded; if (folded) carry.slots_dirty = true;
        is.phi_current = false; is.let_moved = true; is.forces_current = false;
    }
    // a walk over all bodies of an fp32 tree has written group_cost, in the order of perm
    void group_costs_written() { last.group_cost_valid = true; last.cost_perm = nullptr; }
    // bh_compute_forces, bh_step_kdk return; all: completed and covered every body.  A non-integrating walk by itself sets nothing.
    void forces_computed(bool all) { is.forces_current = all; }
    // bh_drift: the bounds are not folded, and the tree is gone (bh_sync checks no overflow, bh_stats reports no nodes)
    void positions_moved_by_drift() { is.forces_current = false; is.phi_current = false; is.tree_valid = false; carry.slots_valid = false; }
    // bh_scatter_sorted: neither tree_valid, let_moved nor partial_count
    void positions_moved_by_scatter() { carry.slots_valid = false; is.phi_current = false; is.forces_current = false; }
    void potential_computed(bool ok) { is.phi_current = ok; }                    // bh_compute_potential, bh_let_potential
    void let_configured() { is.tree_valid = false; }                             // the forest replaces the node array
    void let_bounds_taken() { carry.partial_count = 0; carry.slots_valid = false; }   // the records are consumed
    void let_built() { is.let_moved = false; }                                   // after the build_completed of its local tree
    void migration_packed() { is.tree_valid = false; }                           // the sort buffers are reused from here on
    // The quiet scope: the record is copied aside (RunState saved = *this), a diagnostic's builds and walks fire the events above,
    // and quiet_end puts back, as whole structs, everything a later build reads from an earlier one and everything the last real
    // build and walk report.  `is` is not put back: a quiet build leaves tree_valid and aux_full as it made them.
    void quiet_end(const RunState &saved) { carry = saved.carry; last = saved.last; }
    // on the copy, before quiet_end: the quiet LET build has copied the last force walk's permutation aside for the ORB weights
    void costs_indexed_through(const uint32_t *perm_copy) { last.cost_perm = perm_copy; }
};

}  // namespace bh
