"""bh_kick, bh_drift, bh_timestep and bh_step_kdk on the device.

  * compute_forces(); kick(dt); drift(dt) IS step(1), bit for bit, at the wave and workgroup edges of the elementwise
    kernels, through a physical re-ordering of the state (BH_REORDER_EVERY=2);
  * kick(h) and drift(h) equal the twin tests/split_ref.py for a half step, a negative step and h = 0;
  * the state rules of include/bhgpu.h: when the forces count as current, and that the diagnostics keep them so;
  * step_kdk is the composition the header states, reuses its closing forces, and leaves nothing stale behind;
  * the leapfrog is second order where the fused step is first order (the eccentric pair of DESIGN.md section 17);
  * the time-step criterion against numpy on accelerations(), and the adaptive loop against the same loop in numpy;
  * project.py --integrator kdk.

Fixture, G and dt: integrator_ref.make_fixture, 1, 0.01, as tests/test_gpu_integrator.py holds them."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
import integrator_ref as R  # noqa: E402
import split_ref as S  # noqa: E402
import test_gpu_integrator as TI  # noqa: E402

P = G.Precision
KIND = TI.KIND
DT = R.FIX_DT
ERR_ARG, ERR_STATE = -1, -5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 2, 63, 64, 65, 257, 1000]            # one body, the wave edges, a last partial 256-block, several blocks


def loaded(n, precision, masses="scaled", **cfg):
    m, p, v = TI.bodies(n, precision, masses)
    e = TI.engine(n, precision, **cfg)
    e.upload(p, v, m)
    return e


def forces_only(e):
    """compute_forces() without the download of the forces."""
    e._check(e._lib.bh_compute_forces(e._h))


def code(call, *args):
    try:
        call(*args)
    except G.BhError as err:
        return err.code
    return 0


def same_state(a, b, what):
    (pa, va), (pb, vb) = a.download(), b.download()
    bad = np.flatnonzero((pa != pb).any(axis=1) | (va != vb).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(pa)} bodies differ; first {bad[0]}: {pa[bad[0]]}, {va[bad[0]]} != {pb[bad[0]]}, {vb[bad[0]]}"
    return pa, va


# ---- split equals fused --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["f32", "mixed", "exact", "f64_pow2", "f64_scaled"])
def test_split_equals_fused(monkeypatch, case, n):
    TI._env(monkeypatch)
    precision = {"f32": P.F32, "mixed": P.MIXED, "exact": P.F64_EXACT}.get(case, P.F64)
    masses = "pow2" if case == "f64_pow2" else "scaled"
    with loaded(n, precision, masses) as a, loaded(n, precision, masses) as b:
        p0 = b.download()[0]
        for s in range(3):
            a.step(1)
            forces_only(b)
            if case == "f64_scaled":
                # the fused F64 epilogue kicks with G * sum, the operator with ((G m) * sum) / m: held to the twin instead
                acc = TI.accel_of(b)
                pb, vb = b.download()
            b.kick(DT)
            b.drift(DT)
            if case == "f64_scaled":
                pn, vn = b.download()
                ok = np.isfinite(acc).all(axis=1)
                assert ok.mean() >= 0.99
                vt = S.kick(acc[ok], vb[ok], DT, "f64")
                TI.same(vn[ok], vt, "velocities", s)
                TI.same(pn[ok], S.drift(vt, pb[ok], DT, "f64"), "positions", s)
            else:
                same_state(a, b, f"step {s}")
        if n > 1:
            assert not np.array_equal(b.download()[0], p0)


# ---- the twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(P), ids=[x.name for x in P])
def test_kick_and_drift_equal_the_twin(monkeypatch, precision):
    TI._env(monkeypatch)
    kind = KIND[precision]
    with loaded(1000, precision) as e:
        forces_only(e)
        a = TI.accel_of(e)
        ok = np.isfinite(a).all(axis=1)
        assert ok.mean() >= 0.99
        for h in (DT / 2, -DT, 0.0):                          # (the kick keeps the forces current: three in a row)
            p0, v0 = e.download()
            e.kick(h)
            p1, v1 = e.download()
            assert np.array_equal(p1, p0)
            TI.same(v1[ok], S.kick(a[ok], v0[ok], h, kind), f"kick({h}): velocities", 0)
            assert (h == 0.0) == np.array_equal(v1, v0)
        for h in (DT / 2, -DT, 0.0):
            p0, v0 = e.download()
            e.drift(h)
            p1, v1 = e.download()
            assert np.array_equal(v1, v0)
            TI.same(p1[ok], S.drift(v0[ok], p0[ok], h, kind), f"drift({h}): positions", 0)
            assert (h == 0.0) == np.array_equal(p1, p0)


# ---- state rules -----------------------------------------------------------------------------------------------------------
def _stale(e):
    return code(e.kick, DT) == ERR_STATE and code(e.timestep, 0.02, 1e-3) == ERR_STATE


def _current(e):
    return code(e.kick, DT) == 0 and code(e.timestep, 0.02, 1e-3) == 0


@pytest.mark.parametrize("precision", [P.F32, P.F64_EXACT], ids=["F32", "F64_EXACT"])
def test_when_the_forces_are_current(monkeypatch, precision):
    TI._env(monkeypatch)
    n = 257
    m, p, v = TI.bodies(n, precision)
    with TI.engine(n, precision) as e:
        for call in (lambda: e.kick(DT), lambda: e.drift(DT), lambda: e.timestep(0.02, 1e-3), lambda: e.step_kdk(1)):
            assert code(call) == ERR_STATE                    # before upload
        e.upload(p, v, m)
        assert _stale(e)                                      # before compute_forces
        forces_only(e)
        assert _current(e) and _current(e)                    # (a kick keeps them)
        e.drift(DT)
        assert _stale(e)
        forces_only(e)
        e.step(1)
        assert _stale(e)
        forces_only(e)
        e.upload(p, v, m)
        assert _stale(e)
        forces_only(e)
        e.build_tree()
        assert _stale(e)
        forces_only(e)
        e.drift(0.0)                                          # (moves nobody; the rule is the drift's all the same)
        assert _stale(e)
        if precision == P.F32:
            forces_only(e)
            e.set_softening(1e-3)
            assert _stale(e)
            forces_only(e)
            e.set_softening(1e-3)                             # the same value again: nothing changes
            assert _current(e)
        forces_only(e)
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert code(e.kick, bad) == ERR_ARG and code(e.drift, bad) == ERR_ARG and code(e.timestep, bad, 1e-3) == ERR_ARG
        assert e._lib.bh_timestep(e._h, 0.02, 1e-3, None) == ERR_ARG and code(e.step_kdk, -1) == ERR_ARG
        assert _current(e)                                    # (a refused call changes nothing)
        done, (p1, v1) = e.stats().steps_done, e.download()
        e.step_kdk(0)                                         # a no-op
        assert e.stats().steps_done == done and all(np.array_equal(x, y) for x, y in zip(e.download(), (p1, v1)))
        e.step_kdk(2)
        assert e.stats().steps_done == done + 2 and _current(e)      # the closing forces
        # n = 0 is valid
        e.upload(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        forces_only(e)
        e.kick(DT)
        t = e.timestep(0.02, 1e-3)
        assert (t.dt, t.a_max, t.worst, t.n_bodies) == (float("inf"), 0.0, -1, 0)
        e.drift(DT)
        e.step_kdk(2)
        e.sync()


def test_let_mode_refuses_the_operators(monkeypatch):
    TI._env(monkeypatch)
    n = 257
    with loaded(n, P.F32) as e:
        forces_only(e)
        e.let_configure(0, 2, 1024)
        for call in (lambda: e.kick(DT), lambda: e.drift(DT), lambda: e.timestep(0.02, 1e-3), lambda: e.step_kdk(1)):
            assert code(call) == ERR_STATE
    with loaded(n, P.F32) as e:                               # the replicated scheme: a rank walks only its share
        forces_only(e)
        e.set_owned_fraction(0, 2)
        for call in (lambda: e.kick(DT), lambda: e.drift(DT), lambda: e.timestep(0.02, 1e-3), lambda: e.step_kdk(1)):
            assert code(call) == ERR_STATE


@pytest.mark.parametrize("precision", list(P), ids=[x.name for x in P])
def test_the_diagnostics_keep_the_forces_current(monkeypatch, precision):
    TI._env(monkeypatch)
    n = 1000
    pts = np.array([[0.0, 0.0], [0.05, -0.07], [0.3, 0.3]]) + 1e-4
    with loaded(n, precision) as a, loaded(n, precision) as b:
        for e in (a, b):
            e.step(1)                                         # (so that the state has been re-ordered once)
            forces_only(e)
        a.energy()
        a.field(pts)
        a.force_error(sample=64)
        a.direct_forces(np.arange(8))
        f = a.forces()
        assert np.array_equal(f, b.forces())
        a.kick(DT / 2)
        b.kick(DT / 2)
        same_state(a, b, "kick after the diagnostics")
        assert a.timestep(0.02, 1e-3) == b.timestep(0.02, 1e-3)
        a.step(2)
        b.step(2)
        same_state(a, b, "steps after the diagnostics")


def test_the_potential_survives_a_kick_and_not_a_drift(monkeypatch):
    TI._env(monkeypatch)
    n = 257
    with loaded(n, P.F64) as e:
        forces_only(e)
        phi = e.potential()
        e.kick(DT)
        out = np.zeros(n)
        assert e._lib.bh_get_potential(e._h, out.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        assert np.array_equal(out, phi)
        forces_only(e)
        e.drift(DT)
        assert e._lib.bh_get_potential(e._h, out.ctypes.data_as(C.POINTER(C.c_double)), None) == ERR_STATE


# ---- KDK composition ---------------------------------------------------------------------------------------------------------
KDK_CASES = [(P.F32, 1000), (P.F64, 1000), (P.F64_EXACT, 257)]


@pytest.mark.parametrize("precision,n", KDK_CASES, ids=[x.name for x, _ in KDK_CASES])
def test_step_kdk_is_its_composition(monkeypatch, precision, n):
    TI._env(monkeypatch)
    with loaded(n, precision) as a, loaded(n, precision) as b:
        p0 = a.download()[0]
        a.step_kdk(5)
        forces_only(b); b.kick(DT / 2); b.drift(DT)
        b.step(4)
        forces_only(b); b.kick(DT / 2)
        same_state(a, b, "step_kdk(5)")
        assert np.array_equal(a.forces(), b.forces())
        assert a.stats().steps_done == 5 and not np.array_equal(a.download()[0], p0)
        assert code(a.timestep, 0.02, 1e-3) == 0              # the forces are current on return
    with loaded(n, precision) as a, loaded(n, precision) as b:
        a.step_kdk(1)
        a.step_kdk(1)
        forces_only(b); b.kick(DT / 2); b.drift(DT); forces_only(b); b.kick(DT / 2)
        b.kick(DT / 2); b.drift(DT); forces_only(b); b.kick(DT / 2)      # no force walk in front: the closing forces serve
        same_state(a, b, "step_kdk(1) twice")
        assert a.stats().steps_done == 2


@pytest.mark.parametrize("precision,n", [(P.F64_EXACT, 257), (P.F32, 1000)], ids=["F64_EXACT", "F32"])
def test_step_kdk_leaves_nothing_stale(monkeypatch, precision, n):
    TI._env(monkeypatch, BH_REORDER_EVERY=0)
    m = TI.bodies(n, precision)[0]
    with loaded(n, precision) as a, TI.engine(n, precision) as b:
        a.step_kdk(3)
        p, v = a.download()
        b.upload(p, v, m)
        for s in range(10):
            a.step(1)
            b.step(1)
            same_state(a, b, f"step {s} after step_kdk")


# ---- order of convergence ------------------------------------------------------------------------------------------------------
def _energy_error(scheme, dt, t_end=10.0):
    m, p, v = S.pair(0.5)
    with G.BarnesHutEngine(G.BhConfig(capacity=2, precision=P.F64, G=1.0, dt=dt, max_depth=16)) as e:
        e.upload(p, v, m)
        e0 = e.energy().total
        advance = e.step_kdk if scheme == "kdk" else e.step
        worst = 0.0
        for _ in range(int(round(t_end / dt))):
            advance(1)
            worst = max(worst, abs(e.energy().total - e0) / abs(e0))
    return worst


def test_order_of_convergence():
    """The twin (tests/split_ref.py) gives ratios of 3.99 and 2.03 and a factor of 20.7; the F64 walk of two bodies is the
    direct sum to 1e-12 relative."""
    kdk = [_energy_error("kdk", dt) for dt in (0.01, 0.005)]
    euler = [_energy_error("euler", dt) for dt in (0.01, 0.005)]
    print(f"max |dE/E|: kdk {kdk[0]:.4e} {kdk[1]:.4e} (ratio {kdk[0] / kdk[1]:.3f}), euler {euler[0]:.4e} {euler[1]:.4e} "
          f"(ratio {euler[0] / euler[1]:.3f}), euler / kdk at 0.01: {euler[0] / kdk[0]:.2f}")
    assert 3.5 <= kdk[0] / kdk[1] <= 4.5
    assert 1.8 <= euler[0] / euler[1] <= 2.3
    assert kdk[0] < euler[0] / 10


# ---- the criterion -------------------------------------------------------------------------------------------------------------
def _ulps(x, y):
    return abs(x - y) / np.spacing(abs(y))


@pytest.mark.parametrize("precision", list(P), ids=[x.name for x in P])
def test_timestep_against_numpy(monkeypatch, precision):
    TI._env(monkeypatch)
    n, eta, length = 1000, 0.02, 1e-3
    soft = [0.0] if precision == P.F64_EXACT else [0.0, length]     # (the bit-exact mode takes no softening)
    for eps in soft:
        with loaded(n, precision, softening=eps) as e:
            e.step(1)                                         # (F32 / MIXED: device slots are no caller indices from here on)
            forces_only(e)
            a = e.accelerations()
            a2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
            assert np.isfinite(a2).all()
            top = np.sort(a2)[-2:]
            assert top[1] - top[0] > 1e-12 * top[1]           # the maximum is nobody's tie
            a_max = np.sqrt(a2.max())
            t = e.timestep(eta, length)
            print(f"{precision.name} eps = {eps}: dt {t.dt!r}, a_max {t.a_max!r}, worst {t.worst}")
            assert t.n_bodies == n and t.worst == int(np.argmax(a2))
            assert _ulps(t.a_max, a_max) <= 4 and _ulps(t.dt, eta * np.sqrt(length / a_max)) <= 4
            assert e.timestep(eta, length) == t               # the same bits twice
            if eps:
                assert e.timestep(eta) == t and e.timestep(eta, 0.0) == t and e.timestep(eta, -1.0) == t
            else:
                assert code(e.timestep, eta) == ERR_ARG and code(e.timestep, eta, 0.0) == ERR_ARG


def test_timestep_of_coincident_bodies_and_of_no_acceleration():
    m = np.full(6, 0.25)
    p = np.array([[0.1, 0.2], [-0.3, 0.05], [0.4, -0.1], [-0.3, 0.05], [0.0, -0.4], [0.25, 0.3]])     # 3 sits on 1
    with G.BarnesHutEngine(G.BhConfig(capacity=6, precision=P.F64, G=1.0, dt=DT, max_depth=16)) as e:
        e.upload(p, np.zeros((6, 2)), m)
        forces_only(e)
        a = e.accelerations()
        assert not np.isfinite(a[1]).all() and not np.isfinite(a[3]).all() and np.isfinite(a[[0, 2, 4, 5]]).all()
        t = e.timestep(0.02, 1e-3)
        assert t.dt == 0.0 and t.a_max == float("inf") and t.worst == 1 and t.n_bodies == 6
        e.upload([[0.5, 0.5]], [[0.0, 0.0]], [1.0])           # one body: no acceleration at all
        forces_only(e)
        t = e.timestep(0.02, 1e-3)
        assert t.dt == float("inf") and t.a_max == 0.0 and t.worst == 0 and t.n_bodies == 1


# ---- the adaptive loop -----------------------------------------------------------------------------------------------------------
def test_step_adaptive_against_numpy():
    ecc, eta, length, t_end = 0.9, 0.05, 0.05, 3.0
    t_np, steps_np, p_np, v_np, dts, clips = S.pair_adaptive(ecc, eta, length, t_end)
    # no dt of the numpy run lies within 1e-9 of a value it is clipped against, except the final clip to t_end itself:
    # a 1e-12 difference in the forces cannot change a decision
    margin = min(abs(d - c) / c for d, cs in zip(dts[:-1], clips[:-1]) for c in cs)
    assert margin > 1e-9 and dts[-1] > clips[-1][-1] * (1 + 1e-9) and steps_np > 100
    m, p, v = S.pair(ecc)
    with G.BarnesHutEngine(G.BhConfig(capacity=2, precision=P.F64, G=1.0, dt=DT, max_depth=16)) as e:
        e.upload(p, v, m)
        t, steps = e.step_adaptive(t_end, eta, length=length)
        pn, vn = e.download()
        print(f"adaptive: {steps} steps (numpy {steps_np}), max |dp| {np.abs(pn - p_np).max():.3e}")
        assert t == 3.0 and steps == steps_np
        assert np.allclose(pn, p_np, rtol=1e-9, atol=0.0)
        assert code(e.timestep, eta, length) == 0             # the closing forces are current
        # dt_max clips every step; t starts where the caller says
        t2, steps2 = e.step_adaptive(3.0 + 8e-4, eta, length=length, dt_max=1e-4, t=3.0)
        assert t2 == 3.0 + 8e-4 and steps2 in (8, 9)
        e.upload(p, np.zeros((2, 2)), [0.0, 0.0])             # massless bodies in an fp64 precision: a = 0 / 0
        with pytest.raises(G.BhError):
            e.step_adaptive(1.0, eta, length=length)


# ---- the command line ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def cwd_with_init(tmp_path, monkeypatch):
    for f in ("masses", "positions", "velocities"):
        shutil.copy(os.path.join(GOLD, "init1024", f"{f}_init.txt"), tmp_path / f"{f}_init.txt")
    monkeypatch.chdir(tmp_path)
    return tmp_path


def _by_hand(init1024, advance_name, tmp_path):
    """runSimulationGpu's sequence for 20 steps with an energy file and no cadence, driven by hand: the last energy line."""
    m, p, v = init1024
    cfg = G.BhConfig(capacity=1024, theta=project.THETA, G=project.G, dt=project.DELTA_T, max_depth=project.QUADTREE_MAX_DEPTH,
                     precision=P.F32, reference_compat=True, softening=1e-3)
    with G.BarnesHutEngine(cfg) as e:
        e.upload(p, v, m)
        advance = getattr(e, advance_name)
        e.energy()
        e.build_tree(); e.write_quadtree_file(str(tmp_path / "hand_init.txt")); advance(1)
        advance(18)
        e.build_tree(); e.write_quadtree_file(str(tmp_path / "hand_final.txt")); advance(1)
        en = e.energy()
        pos, vel = e.download()
    line = ",".join(["20"] + ["%.17g" % x for x in (20 * project.DELTA_T, en.kinetic, en.potential, en.total, en.momentum[0],
                                                     en.momentum[1], en.angular_momentum)])
    return line, pos, vel


ARGS = ["-DN_BODIES=1024", "-DN_SIMULATIONS=20", "--precision", "f32", "--softening", "1e-3", "--energy-file", "energy.csv"]


def test_cli_integrator_kdk(cwd_with_init, init1024, capsys):
    assert project.main(ARGS + ["--integrator", "kdk"]) == 0
    capsys.readouterr()
    lines = open("energy.csv").read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0,0,")
    want, _, _ = _by_hand(init1024, "step_kdk", cwd_with_init)
    assert lines[-1] == want
    for mine, hand in (("quadtree_init_gpu.txt", "hand_init.txt"), ("quadtree_final_gpu.txt", "hand_final.txt")):
        assert open(mine, "rb").read() == open(hand, "rb").read()
    euler, _, _ = _by_hand(init1024, "step", cwd_with_init)
    assert euler != want                                      # (another integrator, another state)


def test_cli_without_the_flag_is_the_fused_step(cwd_with_init, init1024, capsys):
    files = ("energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt")
    assert project.main(ARGS) == 0
    plain = [open(f, "rb").read() for f in files]
    assert project.main(ARGS + ["--integrator", "euler"]) == 0
    capsys.readouterr()
    assert plain == [open(f, "rb").read() for f in files]
    want, pos, vel = _by_hand(init1024, "step", cwd_with_init)
    assert plain[0].decode().splitlines()[-1] == want
    assert plain[1] == open("hand_init.txt", "rb").read() and plain[2] == open("hand_final.txt", "rb").read()
    m, p, v = init1024
    pos2, vel2, _ = project.runSimulationGpu(m, p, v, 20, precision=P.F32, softening=1e-3)
    assert np.array_equal(pos2, pos) and np.array_equal(vel2, vel)
    with pytest.raises(ValueError):
        project.runSimulationGpu(m, p, v, 1, integrator="rk4")
