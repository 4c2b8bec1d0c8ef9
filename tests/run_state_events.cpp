// Applies named events of csrc/bh_run_state.hpp to one RunState (tests/test_sequence_cpu.py compiles and runs this with the host
// compiler).  Standard input: one event per line, its name and then its integer arguments; standard output: after every event the
// four facts a return code depends on, "uploaded tree_valid forces_current phi_current".  `nop` fires nothing (a call without an
// event of its own); quiet_begin / quiet_end are the quiet scope: the record copied aside, and RunState::quiet_end on the copy.
// A build is one with its own root box whose launches succeeded, as every build of a single-GPU context is.
#include "bh_run_state.hpp"

#include <cstdio>
#include <string>
#include <iostream>

using namespace bh;

int main()
{
    RunState s, saved;
    std::string ev;
    while (std::cin >> ev) {
        long long a = 0, b = 0;
        if (ev == "nop") {}
        else if (ev == "new_bodies") s.new_bodies();
        else if (ev == "bodies_replaced") s.bodies_replaced();
        else if (ev == "law_changed") { std::cin >> a; s.law_changed(a != 0); }
        else if (ev == "forces_outdated") s.forces_outdated();
        else if (ev == "build_completed") {                       // n, reordered
            std::cin >> a >> b;
            s.build_completed(BuildDone{(int64_t)a, true, a <= 4096, true, b != 0, true});
        }
        else if (ev == "all_node_records_written") s.all_node_records_written();
        else if (ev == "walk_begins") { std::cin >> a; s.walk_begins(a != 0); }
        else if (ev == "walk_launched") s.walk_launched();
        else if (ev == "positions_moved_by_walk") { std::cin >> a; s.positions_moved_by_walk(a != 0); }
        else if (ev == "group_costs_written") s.group_costs_written();
        else if (ev == "forces_computed") { std::cin >> a; s.forces_computed(a != 0); }
        else if (ev == "positions_moved_by_drift") s.positions_moved_by_drift();
        else if (ev == "potential_computed") { std::cin >> a; s.potential_computed(a != 0); }
        else if (ev == "quiet_begin") saved = s;
        else if (ev == "quiet_end") s.quiet_end(saved);
        else { std::printf("unknown event %s\n", ev.c_str()); return 2; }
        if (!std::cin) { std::printf("missing argument of %s\n", ev.c_str()); return 2; }
        std::printf("%d %d %d %d\n", (int)s.is.uploaded, (int)s.is.tree_valid, (int)s.is.forces_current, (int)s.is.phi_current);
    }
    return 0;
}
