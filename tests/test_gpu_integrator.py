"""Every walk epilogue's kick-drift against its exact twin (tests/integrator_ref.py), bit for bit.

After step(1), accelerations() holds the accelerations that step used (F32 / MIXED: the device's fp32 acc_out widened;
fp64 precisions: forces() / masses()), and download() the new state.  So
    v' == kick(a, dt, v)  and  p' == drift(v', dt, p)
is asserted per body and per component with ==, for each of three single steps (BH_REORDER_EVERY=2: the state is
physically re-ordered in between), in every separately compiled copy of the epilogue: the fp32 kernel's instantiations,
its state64 branch (MIXED), the sorted exchange branch, the two-launch forest walk, the F64 walk (hand-written and
portable) and the two F64_EXACT walks.  What is fused, which dt and which a enter: integrator_ref.kick_drift and
DESIGN.md section 2.  tests/test_integrator_cpu.py shows that on this fixture an unfused fp32 epilogue, a drift with
the old velocity and an fp64 epilogue with float32(dt) are each told apart from the right one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd.engine import (FLAG_LDS_STACK, FLAG_WALK_NO_SPLIT, FLAG_WALK_PORTABLE,  # noqa: E402
                                             FLAG_WALK_STATS)
import integrator_ref as R  # noqa: E402
from let_ranks import EmulatedRanks  # noqa: E402

P = G.Precision
ENV = ("BH_EXACT_BFS_MAX", "BH_EXACT_BPW", "BH_WALK_ASM", "BH_WALK_SPLIT", "BH_REORDER_EVERY")
KIND = {P.F32: "f32", P.MIXED: "mixed", P.F64: "f64", P.F64_EXACT: "exact"}
STEPS = 3


def _env(monkeypatch, **kw):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def bodies(n, precision, masses="scaled", seed=0):
    """The fixture as `precision` holds it: fp32 values for F32, not fp32-representable for MIXED."""
    m, p, v = R.make_fixture(n, seed, masses)
    if n == 1:
        v = np.array([[1e-42, 0.0]])                          # subnormal in fp32: a == 0 must hand it back unchanged
    if precision == P.F32:
        return R.to_f32(m), R.to_f32(p), R.to_f32(v)
    if precision == P.MIXED:
        p = p * (1.0 + 3e-9 * np.random.default_rng(1).standard_normal(p.shape))
        assert not np.array_equal(p, R.to_f32(p))
    return m, p, v


def engine(n, precision, **kw):
    kw.setdefault("G", R.FIX_G)
    kw.setdefault("dt", R.FIX_DT)
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    else:
        kw.setdefault("max_depth", 16)
    return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=precision, **kw))


def accel_of(e):
    """The accelerations the last walk used, as the epilogue had them."""
    if e.cfg.precision in (P.F32, P.MIXED):
        return e.accelerations()
    a = R.accel_exact(e.forces(), e.masses())
    assert np.array_equal(e.accelerations(), a, equal_nan=True)
    return a


def same(got, want, what, step):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (f"{what} of step {step}: {len(bad)} of {len(got)} bodies differ from the twin; first "
                           f"{bad[0]}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}")


def check_steps(e, advance=None, first_accel=None, v_bound=False, steps=STEPS):
    """`steps` single steps of engine e, each held to the twin.  advance(e) performs one step and returns the
    accelerations it used (default: step(1), accel_of).  v_bound: the velocity is held to the derived bound of the
    F64 walk with arbitrary masses instead (module test below), the position stays bitwise."""
    kind, dt = KIND[e.cfg.precision], e.cfg.dt
    p, v = e.download()
    for s in range(steps):
        if advance is None:
            e.step(1)
            a = accel_of(e)
        else:
            a = advance(e)
        pn, vn = e.download()
        if s == 0 and first_accel is not None:
            assert np.array_equal(a, first_accel)
        ok = np.isfinite(a).all(axis=1)
        assert ok.mean() >= 0.99 and np.isfinite(pn[ok]).all() and np.isfinite(vn[ok]).all()
        vt, pt = R.kick_drift(a[ok], v[ok], p[ok], dt, kind)
        if v_bound:
            _, pt = R.kick_drift(np.zeros_like(a[ok]), vn[ok], p[ok], dt, kind)     # p' = fma64(v', dt, p) from the device's v'
            err = np.abs(vn[ok] - vt)
            bound = 4 * 2.0 ** -53 * np.abs(a[ok] * dt) + np.spacing(np.abs(vn[ok]))
            print(f"step {s}: max |v' - twin| / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all(), (err / bound).max()
        else:
            same(vn[ok], vt, "velocities", s)
        same(pn[ok], pt, "positions", s)
        if len(p) > 1:
            assert not np.array_equal(pn, p)
        p, v = pn, vn
    return p, v


def run(monkeypatch, precision, n=1000, env=None, masses="scaled", **cfg):
    _env(monkeypatch, **(env or {}))
    m, p, v = bodies(n, precision, masses)
    with engine(n, precision, **cfg) as e:
        e.upload(p, v, m)
        p0, v0 = e.download()
        assert np.array_equal(p0, p) and np.array_equal(v0, v)
        return check_steps(e, v_bound=(precision == P.F64 and masses == "scaled"))


# ---- F32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, FLAG_WALK_PORTABLE, FLAG_LDS_STACK | FLAG_WALK_NO_SPLIT, FLAG_WALK_STATS],
                         ids=["default", "portable", "lds_nosplit", "stats"])
def test_f32_flags(monkeypatch, flags):
    run(monkeypatch, P.F32, flags=flags)


@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_f32_split(monkeypatch, split):
    run(monkeypatch, P.F32, env={"BH_WALK_SPLIT": split})


@pytest.mark.parametrize("flags", [0, FLAG_WALK_PORTABLE], ids=["default", "portable"])
def test_f32_softened(monkeypatch, flags):
    run(monkeypatch, P.F32, softening=0.01, flags=flags)


def test_f32_n_threads_passes(monkeypatch):
    """n_threads = 256: four launches per step.  The accelerations of the step are those of a compute_forces() just before
    it: a later pass does not see the bodies an earlier pass has moved."""
    _env(monkeypatch)
    n = 1000
    m, p, v = bodies(n, P.F32)
    with engine(n, P.F32, n_threads=256) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a0 = e.accelerations()
        check_steps(e, first_accel=a0)
        assert e.stats().walk_launches == 4


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("precision", [P.F32, P.MIXED], ids=["f32", "mixed"])
def test_sizes(monkeypatch, precision, n):
    """The ragged last wave, and the size just above the one-bucket sort and the small-launch walks.  n = 1: the body has
    the velocity (1e-42, 0), subnormal in fp32, and a == 0: it comes back with that velocity -- the epilogue keeps gradual
    underflow (the twin has no flush switch)."""
    pn, vn = run(monkeypatch, precision, n=n)
    if n == 1:
        want = bodies(1, precision)[2]
        assert want[0, 0] != 0.0 and np.array_equal(vn, want)
        if precision == P.F32:
            assert want[0, 0] < 2.0 ** -126


# ---- MIXED -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "portable", "split4", "softened"])
def test_mixed(monkeypatch, case):
    cfg = {"portable": dict(flags=FLAG_WALK_PORTABLE), "softened": dict(softening=0.01)}.get(case, {})
    run(monkeypatch, P.MIXED, env={"BH_WALK_SPLIT": 4} if case == "split4" else None, **cfg)


# ---- F64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", ["pow2", "scaled"])
@pytest.mark.parametrize("case", ["asm", "portable", "softened"])
def test_f64(monkeypatch, case, masses):
    """Masses that are powers of two: (G m) * sum / m is exactly G * sum, forces() / m is the device's a, and v' and p' are
    both bitwise.  Arbitrary masses: p' == fma64(v', dt, p) stays bitwise (it depends on the downloaded v' only); three
    roundings separate fl(fl(G m) * sum) / m from fl(G * sum), and two more end the two kicks, so
        |v' - fma64(F / m, dt, v)| <= 4 * 2^-53 * |F / m * dt| + ulp(v')."""
    cfg = {"portable": dict(flags=FLAG_WALK_PORTABLE), "softened": dict(softening=0.01)}.get(case, {})
    run(monkeypatch, P.F64, masses=masses, **cfg)


# ---- F64_EXACT -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["cooperative", "bfs"])
def test_exact(monkeypatch, walk):
    run(monkeypatch, P.F64_EXACT, env={"BH_EXACT_BFS_MAX": 0} if walk == "cooperative" else None, max_depth=10)


# ---- the sorted exchange path ----------------------------------------------------------------------------------------------
def test_f32_sorted_exchange_path(monkeypatch):
    """step_local() integrates into the sorted exchange buffer (the to_sorted branch), scatter_sorted() brings it back to
    the caller's order; the walk writes acc_out on this path as on the others."""
    _env(monkeypatch)
    n = 1000
    m, p, v = bodies(n, P.F32)

    def advance(e):
        e.step_local()
        a = e.accelerations()
        e.scatter_sorted()
        return a

    with engine(n, P.F32) as e:
        e.upload(p, v, m)
        e.set_owned_fraction(0, 1)
        assert e.owned_range() == (0, n)
        e.compute_forces()
        a0 = e.accelerations()
        check_steps(e, advance=advance, first_accel=a0)


# ---- the forest walk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_launches", [False, True], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("precision", [P.F32, P.MIXED], ids=["f32", "mixed"])
def test_forest_walk(monkeypatch, precision, two_launches):
    """Three emulated ranks; every rank's own download() before and after a distributed step against its own
    accelerations().  two_launches: part 1 parks the raw sums of the local tree, part 2 adds the received trees and
    integrates."""
    _env(monkeypatch)
    n, world = 3000, 3
    m, p, v = bodies(n, precision)
    er = EmulatedRanks(m, p, v, world, let_cap=None, precision=precision, max_depth=21, reference_compat=False,
                       G=R.FIX_G, dt=R.FIX_DT)
    try:
        state = [e.download() for e in er.engs]
        for s in range(STEPS):
            er.step(two_launches=two_launches)
            for r, e in enumerate(er.engs):
                assert e.n >= 64
                a = e.accelerations()
                pn, vn = e.download()
                ok = np.isfinite(a).all(axis=1)
                assert ok.mean() >= 0.99
                vt, pt = R.kick_drift(a[ok], state[r][1][ok], state[r][0][ok], R.FIX_DT, KIND[precision])
                same(vn[ok], vt, f"rank {r}: velocities", s)
                same(pn[ok], pt, f"rank {r}: positions", s)
                assert not np.array_equal(pn, state[r][0])
                state[r] = (pn, vn)
    finally:
        er.close()


# ---- calls that do not integrate -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(P), ids=[x.name for x in P])
def test_non_integrating_calls_leave_the_state(monkeypatch, precision):
    _env(monkeypatch)
    n = 1000
    m, p, v = bodies(n, precision)
    pts = np.array([[0.0, 0.0], [0.05, -0.07], [0.031, -0.019], [0.3, 0.3], [-0.1, 0.1]]) + 1e-4
    with engine(n, precision) as e:
        e.upload(p, v, m)
        p0, v0 = e.download()
        for call in (e.compute_forces, e.potential, lambda: e.field(pts), lambda: e.step(0)):
            call()
            pn, vn = e.download()
            assert np.array_equal(pn, p0) and np.array_equal(vn, v0)
        e.step(1)                                            # (and the state is a live one: a step does move it)
        assert not np.array_equal(e.download()[0], p0)
