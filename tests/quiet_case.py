"""One more input of the single-GPU non-perturbation tests (test_gpu_energy, test_gpu_direct, test_gpu_field, test_gpu_soft): what
bh_stats reports about the last real build and force walk is the same before and after a diagnostic, and the run goes on bit for
bit.

n = 4,353 = 17 * 256 + 1: above the 4,096 bodies one bucket sorts, so the first build after an upload takes the LSD passes and a
diagnostic's quiet build right after it the splitter path of the bucket sort (build_bytes tells them apart); below the bit-exact
mode's breadth-first limit of 12,288; 18 launches at n_threads = 256.  All four precisions in one pass, one precision of each tree
kind in passes of 256."""
import functools

import numpy as np

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import initial_conditions as IC

P = G.Precision
N = 4353
CASES = [(P.F64_EXACT, 0), (P.F64, 0), (P.MIXED, 0), (P.F32, 0), (P.F32, 256), (P.F64, 256)]
IDS = [f"{p.name}-{t}" for p, t in CASES]
KEPT = ("build_bytes", "walk_launches", "visits", "interactions", "wave_nodes", "wave_quads", "wave_accepts", "steps_done")


@functools.lru_cache(maxsize=None)
def bodies():
    m, p, v = IC.make("plummer", N, 4, quasi_static=True)
    for a in (m, p, v):
        a.setflags(write=False)
    return m, p, v


def check(prec, n_threads, diagnostic, **cfg):
    """upload; step(1); s0 = stats(); diagnostic(engine); s1 = stats(): the KEPT fields are equal; then two further steps are
    bitwise those of a control engine that made no diagnostic call."""
    m, p, v = bodies()

    def engine():
        return G.BarnesHutEngine(G.BhConfig(capacity=N, precision=prec, n_threads=n_threads, **cfg))

    with engine() as e, engine() as control:
        for x in (e, control):
            x.upload(p, v, m)
            x.step(1)
        s0 = e.stats()
        diagnostic(e)
        s1 = e.stats()
        for k in KEPT:
            print(f"{prec.name} n_threads {n_threads} {k}: {getattr(s0, k)} -> {getattr(s1, k)}")
        assert s0.build_bytes > 0 and s0.steps_done == 1 and s0.walk_launches == (1 if n_threads == 0 else 18)
        for k in KEPT:
            assert getattr(s1, k) == getattr(s0, k), (k, getattr(s0, k), getattr(s1, k))
        e.step(2)
        control.step(2)
        (x1, v1), (x0, v0) = e.download(), control.download()
        assert np.array_equal(x1, x0) and np.array_equal(v1, v0)
        assert e.stats().walk_launches == control.stats().walk_launches
