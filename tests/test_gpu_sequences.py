"""Seeded call sequences over the whole single-GPU API on one context (tests/sequence_case.py): a diagnostic between any two
state changes -- between a kick and a drift, after a drift, after a bare build, on the build count at which the state is
re-ordered, right after an upload of fewer bodies, after a new softening length, directly after another diagnostic -- changes
neither the trajectory nor bh_stats nor what is refused, and gives what it gives alone.  Three oracles, all bit for bit: the
twin's return codes, a control context that makes the movers only, and fresh witness contexts.

Every precision runs its pair-coverage sequences and six random ones; F32 and MIXED with BH_REORDER_EVERY 2 and 3 in turn, so that
re-orderings fall inside the sequences; the fp64 trees never re-order."""
import pytest

pytestmark = pytest.mark.gpu

import sequence_case as S  # noqa: E402

P = S.P
ENV = ("BH_REORDER_EVERY", "BH_SORT_DIRECT", "BH_SORT_BUCKET", "BH_WALK_SPLIT", "BH_WALK_ASM", "BH_EXACT_BFS_MAX", "BH_EXACT_BPW",
       "BH_BUILD_ITEMS")


def env_of(precision, index):
    return {"BH_REORDER_EVERY": 2 + index % 2} if precision in (P.F32, P.MIXED) else {}


def run(monkeypatch, precision, seq, env, n_threads=0, flags=0):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    compared, refused = S.run(precision, seq, env, n_threads, flags)
    assert compared + refused == len(seq) and compared > 0


CASES = [(p, name, k) for p in S.PRECISIONS for k, (name, _) in enumerate(S.sequences(p))]


@pytest.mark.parametrize("precision,name,index", CASES, ids=[f"{p.name}-{name}" for p, name, _ in CASES])
def test_sequence(monkeypatch, precision, name, index):
    # the pair-coverage sequences count their walks (BH_FLAG_WALK_STATS; the bit-exact walks as the other tests run them, without),
    # so that the walk counters of bh_stats are something a diagnostic could change; the random ones run the uncounted walks
    flags = S.WALK_STATS if name.startswith("pair") and precision != P.F64_EXACT else 0
    run(monkeypatch, precision, S.sequences(precision)[index][1], env_of(precision, index), flags=flags)


@pytest.mark.parametrize("precision", [P.F32, P.F64], ids=lambda p: p.name)
@pytest.mark.parametrize("index", [0, 1])
def test_random_sequence_in_passes_of_256(monkeypatch, precision, index):
    """n_threads = 256: 18 walk launches at set A, in the steps and in the force check alike"""
    run(monkeypatch, precision, S.random_sequence(precision, index), env_of(precision, index + 1), n_threads=256)


@pytest.mark.parametrize("switch", ["BH_SORT_DIRECT=2", "BH_SORT_BUCKET=0"])
def test_f32_random_sequence_with_another_sort(monkeypatch, switch):
    """direct input taken whatever the number of bodies that changed bucket; no bucket sort at all (the LSD passes always)"""
    k, v = switch.split("=")
    run(monkeypatch, P.F32, S.random_sequence(P.F32, 2), {"BH_REORDER_EVERY": 2, k: int(v)})


# ---- the sequences' finding: upload(A); step(1) on contexts that step side by side ---------------------------------------
@pytest.mark.parametrize("precision", [P.F64, P.F64_EXACT], ids=lambda p: p.name)
def test_contexts_stepping_side_by_side_build_the_tree_of_one_alone(precision):
    """The reduced sequence is upload(A); step(1) -- no diagnostic -- on a context whose kernels share the GPU with another
    stream's: F64-random0 (upload(A); energy(); step(3)) differed from its control in one run of two.  The fp64 trees' one-launch
    mass pass (com_up_kernel) let a thread that started late sum a cell its children had already finished, which took one more
    from the parent's count: the parent was summed before its last subdivided child, and six cells up to the root lacked six
    bodies' mass (measured at the parent commit: one context in about 150 pairs, the same six cells every time; the keys and the
    permutation were right).  Three contexts per round, each held to the exported tree and the state of a context that stepped
    alone.  The case cannot fail on a right build; on a build with that fault it fails with high probability only (about four
    in five at the measured rate), so a pass there is possible."""
    import numpy as np
    m, p, v = S.bodies("A")

    def result(e):
        nodes, depth = e.export_tree()
        return S.frozen(e.download() + (e.forces(), nodes.view(np.uint8), depth))

    with S._engine(precision, 0) as alone:
        alone.upload(p, v, m)
        alone.step(1)
        want = result(alone)
    for r in range(250):
        with S._engine(precision, 0) as a, S._engine(precision, 0) as b, S._engine(precision, 0) as c:
            for e in (a, b, c):
                e.upload(p, v, m)
            for e in (a, b, c):
                e.step(1)
            for name, e in (("first", a), ("second", b), ("third", c)):
                assert result(e) == want, f"round {r}: the {name} of three contexts stepping side by side"
