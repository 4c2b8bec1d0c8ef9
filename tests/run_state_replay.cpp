// Replays the engine's call sequences on csrc/bh_run_state.hpp alone (tests/test_run_state_cpu.py compiles and runs this with the
// host compiler).  `Engine` composes the events as bh_engine.hip does for one GPU and n > 0 bodies; the sequences are those of
// tests/test_gpu_split.py.  Exit status 0: every accepted and refused call came out as on the device.
#include "bh_run_state.hpp"

#include <cstdio>
#include <string>

using namespace bh;

namespace {

constexpr int OK = 0, ERR_STATE = -5;
int failures = 0;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Engine {
    RunState s;
    double eps = 0.0;
    int64_t n = 257;

    void build(bool may_reorder) { s.build_completed(BuildDone{n, true, n <= 4096, true, may_reorder && s.carry.builds % 16 == 0, true}); }
    void walk(bool integrate)
    {
        s.walk_begins(false);
        if (integrate) s.positions_moved_by_walk(n >= 2);
        s.walk_launched();
        s.group_costs_written();
    }
    int upload() { s.new_bodies(); return OK; }
    int compute_forces()
    {
        if (!s.is.uploaded) return ERR_STATE;
        build(true);
        walk(false);
        s.forces_computed(true);
        return OK;
    }
    int build_tree()
    {
        if (!s.is.uploaded) return ERR_STATE;
        s.forces_outdated();
        build(true);
        return OK;
    }
    int step(int k)
    {
        if (!s.is.uploaded) return ERR_STATE;
        for (int i = 0; i < k; ++i) { build(true); walk(true); }
        return OK;
    }
    int kick() const { return s.is.uploaded && s.is.forces_current ? OK : ERR_STATE; }
    int timestep() const { return kick(); }
    int drift()
    {
        if (!s.is.uploaded) return ERR_STATE;
        s.positions_moved_by_drift();
        return OK;
    }
    int step_kdk(int k)
    {
        if (!s.is.uploaded) return ERR_STATE;
        if (k == 0) return OK;
        if (!s.is.forces_current) { build(true); walk(false); }
        s.positions_moved_by_drift();
        for (int i = 0; i < k; ++i) { build(true); walk(i < k - 1); }
        s.forces_computed(true);
        return OK;
    }
    int set_softening(double e) { s.law_changed(e != eps); eps = e; return OK; }
    int compute_potential()
    {
        if (!s.is.uploaded) return ERR_STATE;
        const RunState saved = s;
        build(false);
        s.quiet_end(saved);
        s.potential_computed(true);
        return OK;
    }
    int get_potential() const { return s.is.uploaded && s.is.phi_current ? OK : ERR_STATE; }
    bool stale() const { return kick() == ERR_STATE && timestep() == ERR_STATE; }
    bool current() const { return kick() == OK && timestep() == OK; }
};

// test_gpu_split.py::test_when_the_forces_are_current (set_softening: its F32 branch)
void when_the_forces_are_current()
{
    Engine e;
    CHECK(e.kick() == ERR_STATE && e.drift() == ERR_STATE && e.timestep() == ERR_STATE && e.step_kdk(1) == ERR_STATE);   // before upload
    e.upload();
    CHECK(e.stale());                                          // before compute_forces
    e.compute_forces();
    CHECK(e.current() && e.current());                         // (a kick keeps them)
    e.drift();
    CHECK(e.stale());
    CHECK(!e.s.is.tree_valid);                                 // (bh_sync checks no overflow, bh_export_tree refuses)
    e.compute_forces();
    e.step(1);
    CHECK(e.stale());
    CHECK(e.s.is.tree_valid);                                  // (an integrating walk keeps the tree's counters readable)
    e.compute_forces();
    e.upload();
    CHECK(e.stale());
    e.compute_forces();
    e.build_tree();
    CHECK(e.stale());
    e.compute_forces();
    e.drift();                                                 // drift(0.0): moves nobody, the rule is the drift's all the same
    CHECK(e.stale());
    e.compute_forces();
    e.set_softening(1e-3);
    CHECK(e.stale());
    e.compute_forces();
    e.set_softening(1e-3);                                     // the same value again: nothing changes
    CHECK(e.current());
    e.compute_forces();
    CHECK(e.current());                                        // (the refused calls in between fire no event)
    e.step_kdk(0);                                             // a no-op
    CHECK(e.current());
    e.step_kdk(2);
    CHECK(e.current());                                        // the closing forces
    e.n = 0;                                                   // n = 0 is valid
    e.upload();
    CHECK(e.compute_forces() == OK && e.kick() == OK && e.timestep() == OK && e.drift() == OK && e.step_kdk(2) == OK);
}

// test_gpu_split.py::test_the_potential_survives_a_kick_and_not_a_drift
void the_potential_survives_a_kick_and_not_a_drift()
{
    Engine e;
    e.upload();
    e.compute_forces();
    CHECK(e.compute_potential() == OK);
    CHECK(e.kick() == OK);
    CHECK(e.get_potential() == OK);
    e.compute_forces();
    CHECK(e.current());                                        // (the quiet build has not outdated the forces)
    e.drift();
    CHECK(e.get_potential() == ERR_STATE);
    e.compute_potential();
    e.set_softening(e.eps);                                    // any setter call outdates the potential, never the forces by itself
    CHECK(e.get_potential() == ERR_STATE);
}

template <typename... T>
std::string bytes(const T &...m)
{
    std::string b;
    (b.append(reinterpret_cast<const char *>(&m), sizeof m), ...);
    return b;
}

// every byte of every member of the two groups the quiet scope restores (a member added to either struct fails to compile here:
// give it a value below and a place in the image)
std::string image(const RunState &s)
{
    const auto &[builds, samples_n, partial_count, slots_valid, slots_dirty] = s.carry;
    const auto &[walk_launches, cost_perm, group_cost_valid, last_sort_bucket, last_sort_packed] = s.last;
    return bytes(builds, samples_n, partial_count, slots_valid, slots_dirty, walk_launches, cost_perm, group_cost_valid, last_sort_bucket,
                 last_sort_packed);
}

void the_quiet_scope_restores_both_groups()
{
    static const uint32_t perm_copy[1] = {0};
    for (int round = 0; round < 2; ++round) {
        RunState s;
        s.new_bodies();
        // every member distinct from its default (round 1: the other value of what the events inside would set the same)
        s.carry = BuildCarry{7, 4353, 18, true, false};
        s.last = LastRun{3, perm_copy, true, round == 0, round == 0};
        if (round == 1) { s.carry.slots_valid = false; s.carry.slots_dirty = true; s.carry.builds = 16; s.last.group_cost_valid = false; }
        const std::string before = image(s);
        const Current is = s.is;
        const RunState saved = s;
        s.build_completed(BuildDone{4353, true, round == 1, round == 1, false, true});    // the quiet build: the other sort
        CHECK(image(s) != before);
        CHECK(s.carry.builds != saved.carry.builds && s.carry.samples_n == 4353 && s.last.cost_perm == nullptr);
        s.walk_begins(false);                                                             // the check's force walk, 18 passes
        for (int p = 0; p < 18; ++p) s.walk_launched();
        s.group_costs_written();
        CHECK(s.last.walk_launches == 18 && s.last.group_cost_valid);
        s.partials_recorded(5);                                                           // the LET side: bounds taken quietly
        s.let_bounds_taken();
        CHECK(s.carry.partial_count == 0);
        s.quiet_end(saved);
        CHECK(image(s) == before);
        // what is current: only the tree and the node records are the quiet build's
        CHECK(s.is.tree_valid && !s.is.aux_full && s.is.uploaded == is.uploaded && s.is.forces_current == is.forces_current &&
              s.is.phi_current == is.phi_current && s.is.let_moved == is.let_moved && s.is.orig_identity == is.orig_identity);
    }
    // the quiet LET build keeps the last force walk's permutation for the ORB weights
    RunState s;
    s.new_bodies();
    s.build_completed(BuildDone{4353, false, false, true, true, true});
    s.group_costs_written();
    RunState saved = s;
    saved.costs_indexed_through(perm_copy);
    s.build_completed(BuildDone{4353, false, true, true, false, true});
    s.let_built();
    s.quiet_end(saved);
    CHECK(s.last.cost_perm == perm_copy && s.last.group_cost_valid && !s.last.last_sort_bucket && s.carry.builds == 1);
}

}  // namespace

int main()
{
    when_the_forces_are_current();
    the_potential_survives_a_kick_and_not_a_drift();
    the_quiet_scope_restores_both_groups();
    std::printf("%d failed checks\n", failures);
    return failures ? 1 : 0;
}
