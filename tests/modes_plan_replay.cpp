// modes_plan_replay.cpp -- runs the LDS selector of the azimuthal modes (csrc/bh_query_host.hpp: modes_planes, modes_plan) with
// the host compiler; a helper of tests/test_modes_cpu.py, which compiles it and compares with tests/modes_ref.py.
//   modes_plan_replay  ->  one line "M rates nb P tile bytes" for every (M, rates) and a set of nb around each boundary
#include <cstdio>

#include "bh_query_host.hpp"

int main()
{
    for (int M = 0; M <= 16; ++M)
        for (int rates = 0; rates < 2; ++rates) {
            const int P = bh::modes_planes(M, rates != 0);
            const int edge = (bh::kModesLdsBytes / 8 - 2 * P - 1) / (P + 1);
            const int nbs[] = {1, 64, edge - 1, edge, edge + 1, edge + 2, 4095, 4096};
            for (int nb : nbs) {
                if (nb < 1 || nb > 4096) continue;
                const bh::ModesPlan plan = bh::modes_plan(P, nb);
                std::printf("%d %d %d %d %d %zu\n", M, rates, nb, P, plan.tile, plan.bytes);
            }
        }
    return 0;
}
