"""bh_binaries and bh_binaries_catalogue on the device, held to the brute-force twin tests/binaries_ref.py: partner, eps, lo, hi and
all eleven record columns are compared with np.array_equal, on the state DOWNLOADED from the engine (in F32 that is the fp32 state
as the device holds it).  The partner is the first candidate in a strict total order, so there is one right answer.

  1. the definition: no body, one, two; a bound and an unbound pair; the inclusive edge d2 == R^2; coincident bodies; a tie
     decided by index and a partner that is not mutual; a hierarchical triple;
  2. pruning adversaries: a fast fly-by nearer than the partner, one far heavy body that binds everybody (the nodes' mass
     bounds), zero masses, a line, two clumps 1e12 apart;
  3. launch edges: sizes around a leaf, a wave, a workgroup and a new level of boxes;
  4. all four precisions, after steps (caller indices after a physical re-order), with a softening set (it does not enter);
  5. at size, where the twin is too big: the partner from the rows of neighbours(32) -- two independent device paths;
  6. the work counters;
  7. the errors of include/bhgpu.h;
  8. the run is not perturbed;
  9. project.py --binaries-file."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
import binaries_ref as B  # noqa: E402
import quiet_case as Q  # noqa: E402

P = G.Precision
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]
BOTH = pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
INF = float("inf")
COLUMNS = ("separation", "energy", "semi_major_axis", "eccentricity", "period", "binding_energy", "mass")
_TWINS = {}


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    kw.setdefault("G", 1.0)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def upload(e, pos, vel=None, mass=None):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    e.upload(pos, np.zeros_like(pos) if vel is None else np.asarray(vel, dtype=np.float64).reshape(-1, 2),
             np.ones(len(pos)) if mass is None else np.asarray(mass, dtype=np.float64))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def twin(pos, vel, mass, g, R):
    """the twin's catalogue of a state, computed once per state and R (F32 and MIXED, F64 and F64_EXACT hold the same state)"""
    key = (pos.tobytes(), vel.tobytes(), mass.tobytes(), g, R)
    if key not in _TWINS:
        _TWINS[key] = B.catalogue(pos, vel, mass, g, R)
    return _TWINS[key]


def same_as_twin(e, R, what="", g=1.0):
    """binaries(R) of the engine's own state against the twin, bit for bit; returns the BhBinaries"""
    pos, vel = e.download()
    mass = e.masses()
    n = len(pos)
    partner, eps, lo, hi, rec = twin(pos, vel, mass, g, R)
    b = e.binaries(R, with_stats=True)
    print(f"{what} n={n} R={R!r}: stats {b.stats}, pairs {len(b.lo)}, bound {(b.partner >= 0).sum()}")
    assert b.n == n and b.partner.dtype == np.int64 and b.lo.dtype == np.int64 and b.hi.dtype == np.int64
    assert b.partner.shape == b.eps.shape == (n,) and b.lo.shape == b.hi.shape == (len(lo),)
    bad = np.nonzero((b.partner != partner) | (b.eps != eps))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} partners differ; first body {bad[0]}: got {(b.partner[bad[0]], b.eps[bad[0]])}, "
                           f"twin {(partner[bad[0]], eps[bad[0]])}")
    assert np.array_equal(b.partner, partner) and np.array_equal(b.eps, eps)
    assert np.array_equal(b.lo, lo) and np.array_equal(b.hi, hi)
    for k, name in enumerate(COLUMNS):
        assert np.array_equal(getattr(b, name), rec[:, k], equal_nan=True), (what, name)
    assert np.array_equal(b.com, rec[:, 7:9], equal_nan=True) and np.array_equal(b.velocity, rec[:, 9:11], equal_nan=True), what
    assert b.stats[3] == len(lo) and b.fraction == (2.0 * len(lo) / n if n else 0.0)
    assert b.total_binding_energy == math.fsum(rec[:, 5].tolist()) or np.isnan(rec[:, 5]).any()
    return b


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------
@BOTH
def test_no_body_one_two_and_a_bound_and_an_unbound_pair(precision):
    with engine(8, precision) as e:
        upload(e, np.zeros((0, 2)))
        b = same_as_twin(e, 1.0, "no body")
        assert b.n == 0 and len(b.lo) == 0 and b.stats == (0, 0, 0, 0) and b.fraction == 0.0 and b.total_binding_energy == 0.0
        upload(e, [[0.25, -3.0]])
        b = same_as_twin(e, 1.0, "one body")
        assert list(b.partner) == [-1] and list(b.eps) == [INF] and len(b.lo) == 0
        upload(e, [[0.0, 0.0], [1.0, 0.0]])                          # at rest: eps = -2
        b = same_as_twin(e, 2.0, "two bodies")
        assert list(b.partner) == [1, 0] and list(b.eps) == [-2.0, -2.0] and (list(b.lo), list(b.hi)) == ([0], [1])
        assert (b.separation[0], b.energy[0], b.semi_major_axis[0], b.eccentricity[0], b.mass[0], b.binding_energy[0]) == (1.0, -2.0, 0.5, 1.0, 2.0, 1.0)
        assert list(b.com[0]) == [0.5, 0.0] and list(b.velocity[0]) == [0.0, 0.0]
        # a bound pair, and a pair flying apart: 0.5 * 16 - 2 > 0
        upload(e, [[0.0, 0.0], [1.0, 0.0], [100.0, 0.0], [101.0, 0.0]], [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 4.0]])
        b = same_as_twin(e, 2.0, "bound and unbound")
        assert list(b.partner) == [1, 0, -1, -1] and list(b.eps) == [-2.0, -2.0, INF, INF] and list(b.lo) == [0]


@BOTH
def test_the_edge_is_inclusive_coincident_bodies_are_no_candidates_and_ties_go_to_the_smaller_index(precision):
    with engine(8, precision) as e:
        upload(e, [[1.0, 2.0], [1.75, 3.0]])                         # 3-4-5: d2 = 1.5625 exactly
        b = same_as_twin(e, 1.25, "d2 == R^2")
        assert list(b.partner) == [1, 0] and b.separation[0] == 1.25
        b = same_as_twin(e, float(np.nextafter(1.25, 0.0)), "just inside R")
        assert list(b.partner) == [-1, -1] and len(b.lo) == 0
        upload(e, [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]])              # two coincident bodies and a third
        b = same_as_twin(e, INF, "coincident")
        assert list(b.partner) == [2, 2, 0] and (list(b.lo), list(b.hi)) == ([0], [2])
        upload(e, [[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])              # collinear, equal, at rest
        b = same_as_twin(e, INF, "three collinear")
        assert list(b.partner) == [1, 0, 1] and list(b.eps) == [-2.0, -2.0, -2.0] and (list(b.lo), list(b.hi)) == ([0], [1])
        b = same_as_twin(e, 1.0, "three collinear, R = 1")
        assert list(b.partner) == [1, 0, 1]


@BOTH
def test_a_hierarchical_triple_lists_the_inner_pair_only(precision):
    m, p, v = B.kepler_pair(1.0, 0.5, 0.0078125, 0.25, 1.0)
    mo, po, vo = B.kepler_pair(1.5, 0.75, 1.0, 0.125, 2.0)            # the inner pair's centre of mass and a third body
    pos = np.concatenate([p + po[0], po[1:]])
    vel = np.concatenate([v + vo[0], vo[1:]])
    with engine(8, precision) as e:
        upload(e, pos, vel, np.concatenate([m, mo[1:]]))
        b = same_as_twin(e, INF, "triple")
        # (the third body is bound to the pair, not to either star: against one star alone it has the inner orbit's speed)
        assert list(b.partner[:2]) == [1, 0] and b.partner[2] in (-1, 0, 1) and (list(b.lo), list(b.hi)) == ([0], [1])
        assert abs(b.semi_major_axis[0] / 0.0078125 - 1.0) < 0.05    # (perturbed by nobody: the third body is not in eps_01)


# ---- 2. pruning adversaries -----------------------------------------------------------------------------------------------------
def background(n, seed):
    m, p, v, _ = B.cluster(n, n // 10, seed)
    return m, p, v


@BOTH
def test_a_fast_fly_by_is_nearer_than_the_partner(precision):
    m, p, v = background(400, 41)
    A, F, H = 100, 250, 399                                           # a light body, the fly-by next to it, a heavy body farther away
    p[A], v[A], m[A] = [20.0, 20.0], [0.0, 0.0], 0.0009765625         # (outside the cluster, which ends at radius 8.6)
    p[F], v[F], m[F] = [20.0009765625, 20.0], [0.0, 50.0], 0.0009765625
    p[H], v[H], m[H] = [20.25, 20.0], [0.0, 0.125], 1.0
    with engine(400, precision) as e:
        upload(e, p, v, m)
        for R in (1.0, INF):
            b = same_as_twin(e, R, "fly-by")
            assert b.partner[A] == H and b.partner[F] != A and b.eps[A] < 0.0
        b = same_as_twin(e, 0.125, "fly-by, the heavy body beyond R")
        assert b.partner[A] == -1


@BOTH
def test_one_far_heavy_body_binds_the_light_ones(precision):
    """a body a million times heavier, 40 lengths away: the bound of a far node rests on the node's largest mass"""
    rng = np.random.default_rng(42)
    n = 600
    p = rng.uniform(size=(n, 2))
    v = rng.normal(size=(n, 2)) * 1e-3
    m = np.full(n, 1e-6)
    heavy = 377
    p[heavy], v[heavy], m[heavy] = [30.0, 30.0], [0.0, 0.0], 1.0
    with engine(n, precision) as e:
        upload(e, p, v, m)
        b = same_as_twin(e, 100.0, "heavy body")
        assert (b.partner == heavy).sum() > n // 2
        assert len(b.lo) >= 1 and heavy in np.concatenate([b.lo, b.hi])       # the heavy body's own partner names it back
        b = same_as_twin(e, 2.0, "heavy body beyond R")
        assert (b.partner != heavy).all()


@BOTH
def test_zero_masses_a_line_and_two_clumps(precision):
    rng = np.random.default_rng(43)
    m, p, v = background(300, 43)
    with engine(300, precision) as e:
        mz = m.copy()
        mz[[5, 6, 150]] = 0.0
        p[6], v[6] = p[5] + [0.001, 0.0], v[5]                        # two bodies without mass side by side and at rest: eps = 0
        upload(e, p, v, mz)
        b = same_as_twin(e, 0.5, "zero masses")
        assert b.partner[5] != 6 and b.partner[6] != 5
        line = p.copy()
        line[:, 1] = 0.25
        upload(e, line, v, m)
        same_as_twin(e, 0.5, "line")
        same_as_twin(e, INF, "line, no cut")
        far = np.concatenate([p[:150], 1e12 + p[150:] * 1e6])         # (fp32 resolves 65,536 at 1e12)
        mass = np.concatenate([m[:150], m[150:] * 1e10])
        order = rng.permutation(300)
        upload(e, far[order], v[order], mass[order])
        b = same_as_twin(e, INF, "two clumps")
        there = order >= 150                                          # (caller index c holds body order[c])
        assert (b.partner >= 0).sum() > 250 and len(b.lo) > 20
        assert (there[b.lo] == there[b.hi]).all()
        same_as_twin(e, 3e5, "two clumps, R between the scales")


# ---- 3. launch edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 2049])
@BOTH
def test_launch_edges(precision, n):
    m, p, v, _ = B.cluster(n, n // 4, n)
    with engine(n, precision) as e:
        upload(e, p, v, m)
        b = same_as_twin(e, 0.05, f"{precision.name} cluster")
        assert len(b.lo) >= n // 4 - 2
        if n <= 513:
            same_as_twin(e, INF, f"{precision.name} cluster, no cut")


# ---- 4. all four precisions, caller indices after a physical re-order, the softening --------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_all_precisions_before_and_after_steps_and_with_a_softening(precision):
    n = 1500
    m, p, v, _ = B.cluster(n, 75, 9)
    with engine(n, precision, dt=1e-7) as e:                           # (a step far below the tightest pair's period)
        e.upload(p, v, m)
        a = same_as_twin(e, 0.05, f"{precision.name} cluster")
        assert len(a.lo) >= 70
        e.step(21)
        b = same_as_twin(e, 0.05, f"{precision.name} cluster after 21 steps")
        assert len(b.lo) >= 50
        h = b.hardness()
        assert h.shape == b.lo.shape and np.array_equal(h, b.binding_energy / (e.energy().kinetic / n))
        if precision != P.F64_EXACT:                                   # (the bit-exact mode takes the unsoftened law only)
            e.set_softening(0.01)
            c = e.binaries(0.05)
            for name in ("partner", "eps", "lo", "hi", "com") + COLUMNS:
                assert np.array_equal(getattr(c, name), getattr(b, name)), name


# ---- 5. at size: the partner from the neighbour lists ---------------------------------------------------------------------------
def test_fifty_thousand_against_the_neighbour_lists():
    n, R = 50000, 0.015
    m, p, v, planted = B.cluster(n, 2500, 6)
    with engine(n, P.F32, dt=1e-7) as e:
        e.upload(p, v, m)
        e.step(2)
        pos, vel = e.download()
        mass = e.masses()
        b = e.binaries(R, with_stats=True)
        print("stats", b.stats, "times", e.binaries_times(), "pairs", len(b.lo))
        cnt = e.count_within(R).astype(np.int64)
        assert cnt.max() <= 32, cnt.max()
        idx, d2n = e.neighbours(32)
        # every candidate set is among the first cnt entries of the body's row: eps of those, in the twin's operation order
        cols = np.arange(32)[None, :]
        inside = cols < cnt[:, None]
        j = np.where(inside, idx, 0)
        dx, dy = pos[j, 0] - pos[:, None, 0], pos[j, 1] - pos[:, None, 1]
        d2 = dx * dx + dy * dy
        assert np.array_equal(d2[inside], d2n[inside]) and (d2[inside] <= R * R).all()
        ux, uy = vel[j, 0] - vel[:, None, 0], vel[j, 1] - vel[:, None, 1]
        v2 = ux * ux + uy * uy
        M = mass[:, None] + mass[j]
        with np.errstate(divide="ignore", invalid="ignore"):
            eps = 0.5 * v2 - (1.0 * M) / np.sqrt(d2)
        cand = inside & (d2 > 0.0) & (eps < 0.0)
        low = np.where(cand, eps, np.inf).min(axis=1)
        jj = np.where(cand & (eps == low[:, None]), j, n).min(axis=1)            # the smallest index among the ties
        partner = np.where(cand.any(axis=1), jj, -1)
        bad = np.nonzero((b.partner != partner) | (b.eps != low))[0]
        assert len(bad) == 0, (len(bad), bad[:5], b.partner[bad[:5]], partner[bad[:5]])
        lo, hi = B.mutual(partner)
        assert np.array_equal(b.lo, lo) and np.array_equal(b.hi, hi) and len(lo) >= 2000
        rec = B.elements(pos, vel, mass, 1.0, lo, hi)
        for k, name in enumerate(COLUMNS):
            assert np.array_equal(getattr(b, name), rec[:, k]), name
        assert np.array_equal(b.com, rec[:, 7:9]) and np.array_equal(b.velocity, rec[:, 9:11])
        got = set(zip(b.lo.tolist(), b.hi.tolist()))
        there = sum((min(int(a), int(c)), max(int(a), int(c))) in got for a, c, _, _ in planted)
        print("planted pairs in the catalogue:", there)
        assert there >= 2250
        tight = b.within(3e-4)
        assert 2000 <= len(tight.lo) <= len(b.lo) and (tight.semi_major_axis <= 3e-4).all()


# ---- 6. the work counters -------------------------------------------------------------------------------------------------------
def test_stats_and_repeatability():
    n, R = 4096, 0.05
    m, p, v, _ = B.cluster(n, 200, 12)
    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        a = e.binaries(R, with_stats=True)
        again = e.binaries(R, with_stats=True)
        print("stats", a.stats, again.stats, "times", e.binaries_times())
        for x in ("partner", "eps", "lo", "hi", "energy", "com"):
            assert np.array_equal(getattr(a, x), getattr(again, x)), x
        assert a.stats == again.stats                              # the header declares all four counters deterministic
        within = int(e.count_within(R).astype(np.int64).sum())
        assert 0 < a.stats[0] <= within + 16 * n                   # energies are computed inside R only; 2 * 8 seeds a body
        assert a.stats[1] <= a.stats[0] and a.stats[1] * n >= a.stats[0] and a.stats[2] >= n and a.stats[3] == len(a.lo)
        bt, st, ct = e.binaries_times()
        assert bt > 0.0 and st > 0.0 and ct >= 0.0
        before = e.stats().device_bytes
        e.binaries(R)
        assert e.stats().device_bytes == before                    # the buffers are kept


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def code_and_text(f, *a, **kw):
    try:
        f(*a, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_errors():
    m, p, v, _ = B.cluster(1000, 50, 3)
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    with engine(1000, P.F64) as e:
        assert code_and_text(e.binaries, 1.0)[0] == ERR_STATE       # before upload
        e.upload(p, v, m)
        for R in (0.0, -1.0, float("nan"), -INF):
            code, text = code_and_text(e.binaries, R)
            assert code == ERR_ARG and "max_separation" in text, (R, code, text)
        assert code_and_text(e.binaries, INF)[0] == 0
        b = e.binaries(0.05)
        g = len(b.lo)
        assert g >= 50
        lib, h = e._lib, e._h
        partner, eps, npairs = np.zeros(1000, dtype=np.int64), np.zeros(1000), C.c_int64()
        assert lib.bh_binaries(h, 0.05, partner.ctypes.data_as(i64), eps.ctypes.data_as(dp), C.byref(npairs), None) == 0
        assert npairs.value == g and np.array_equal(partner, b.partner)
        assert lib.bh_binaries(h, 0.05, None, None, C.byref(npairs), None) == 0 and npairs.value == g
        assert lib.bh_binaries(h, 0.05, partner.ctypes.data_as(i64), eps.ctypes.data_as(dp), None, None) == ERR_ARG
        assert lib.bh_binaries(None, 0.05, None, None, C.byref(npairs), None) == ERR_ARG
        assert lib.bh_binaries_times(h, None, None, None) == ERR_ARG
        # the catalogue of the last call: too little room is BH_ERR_CAPACITY and copies nothing
        lo, hi, rec = np.full(g, -7, dtype=np.int64), np.full(g, -7, dtype=np.int64), np.full((g, 11), -7.0)
        plo, phi, prec = lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), rec.ctypes.data_as(dp)
        assert lib.bh_binaries_catalogue(h, g - 1, plo, phi, prec) == ERR_CAPACITY
        assert (lo == -7).all() and (hi == -7).all() and (rec == -7.0).all()
        assert lib.bh_binaries_catalogue(h, -1, plo, phi, prec) == ERR_ARG
        assert lib.bh_binaries_catalogue(h, g, plo, phi, prec) == 0
        assert np.array_equal(lo, b.lo) and np.array_equal(hi, b.hi) and np.array_equal(rec[:, 2], b.semi_major_axis)
        assert lib.bh_binaries_catalogue(h, g + 5, None, None, None) == 0
        # a position that is not finite: found by the bounds pass; a velocity or a mass that is NaN follows the formulas
        for bad in (float("nan"), INF):
            q = p.copy()
            q[517, 0] = bad
            e.upload(q, v, m)
            code, text = code_and_text(e.binaries, 0.05)
            assert code == ERR_ARG and "non-finite position" in text and "bounds pass" in text, (code, text)
        w, mm = v.copy(), m.copy()
        w[100, 1] = float("nan")
        mm[200] = float("nan")
        e.upload(p, w, mm)
        c = same_as_twin(e, 0.05, "NaN velocity and mass")
        assert c.partner[100] == -1 and c.partner[200] == -1 and not np.isin(c.partner, [100, 200]).any()
        e.upload(p[:0], v[:0], m[:0])                                # no bodies
        c = e.binaries(1.0, with_stats=True)
        assert c.n == 0 and len(c.lo) == 0 and c.stats == (0, 0, 0, 0)
    for g_bad in (0.0, -1.0):
        with engine(1000, P.F64, G=g_bad) as e:
            e.upload(p, v, m)
            code, text = code_and_text(e.binaries, 0.05)
            assert code == ERR_ARG and "G must be > 0" in text, (g_bad, code, text)


def test_a_let_context_has_no_binaries():
    m, p, v, _ = B.cluster(1000, 50, 3)
    with engine(1000, P.F32) as e:
        e.upload(p, v, m)
        e.let_configure(0, 2, 1024)
        code, text = code_and_text(e.binaries, 0.05)
        assert code == ERR_STATE and "single GPU" in text, (code, text)
    with engine(1000, P.F32) as e:                                 # the replicated scheme: world > 1
        e.upload(p, v, m)
        e.set_owned_fraction(0, 2)
        assert code_and_text(e.binaries, 0.05)[0] == ERR_STATE


# ---- 8. non-perturbation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_binaries_between_two_steps_change_nothing(precision, n_threads):
    cfg = dict(max_depth=21, reference_compat=False) if precision in (P.F32, P.MIXED) else {}
    Q.check(precision, n_threads, lambda e: (e.binaries(0.05), e.binaries(INF), e.binaries_times()), **cfg)


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------
def test_project_binaries_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), binaries_file="bin.csv", binaries_separation=0.05, **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flag nothing changes
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and not (b / "bin.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name

    def check(path, R):
        lines = open(path).read().splitlines()
        assert lines[0] == "# i,j,r,a,e,period,binding_energy"
        rows = [l.split(",") for l in lines[1:]]
        _, _, lo, hi, rec = B.catalogue(pa, va, m, 6.67e-11, R)
        assert len(rows) == len(lo) > 20
        assert [int(r[0]) for r in rows] == list(lo) and [int(r[1]) for r in rows] == list(hi)
        got = np.array([[float(x) for x in r[2:]] for r in rows])
        assert np.array_equal(got, rec[:, [0, 2, 3, 4, 5]])
        with G.BarnesHutEngine(G.BhConfig(capacity=1024)) as e:
            e.upload(pa, va, m)
            api = e.binaries(R)
        assert np.array_equal(api.lo, lo) and np.array_equal(got[:, 1], api.semi_major_axis) and np.array_equal(got[:, 4], api.binding_energy)

    check(a / "bin.csv", 0.05)
    with pytest.raises(ValueError):
        project.runSimulationGpu(m, p, v, 1, out_dir=str(b), binaries_file="bin.csv")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--binaries-file", "main_bin.csv",
                             "--binaries-separation", "inf"]) == 0
    finally:
        os.chdir(cwd)
    check(tmp_path / "main_bin.csv", INF)
