"""bh_azimuthal_modes, bh_modes_max and bh_modes_deposit on the device, held to the numpy twin tests/modes_ref.py: every
comparison is np.array_equal on the int64 planes and the two exponents.

  * all four precisions x n in {1, 2, 256, 257, 4099} x (M, rates) in {(0, no), (2, no), (2, yes), (16, yes)} at 32 bins on the
    fixture of radial_ref.fixture (bodies on edges, at the centre, with a subnormal r2, mirror images, inside edges[0] and beyond
    edges[nb], a massless one), with the pieces of a distributed call; 4,609 bodies with BH_RADIAL_BLOCKS=2 (ten trips);
  * the LDS boundary: the largest nb whose histogram is private and the next, and with 4,096 bins a workgroup whose bodies span
    exactly the tile (summed in LDS at an offset) and one slot more (deposited directly), for 6 and for 67 planes;
  * the results do not depend on the order of the bodies in memory (a physical re-order, a permuted upload);
  * a call between two steps changes nothing of the run;
  * bodies at rest, a NaN velocity with and without rates, the errors of include/bhgpu.h;
  * the four-body square and the rigid rotator of tests/test_modes_cpu.py through the engine;
  * project.py --modes-file and --bar-file;
  * LetStepper.azimuthal_modes over gloo, world 1 and 2."""
import ctypes as C
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import project  # noqa: E402
from gpu_nbody_simulation_amd.distributed import wrap_device  # noqa: E402
import modes_ref as MR  # noqa: E402
import quiet_case as Q  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5
HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]
SIZES = [1, 2, 256, 257, 4099]
CONFIGS = [(0, False), (2, False), (2, True), (16, True)]
NB = 32
ENV = ("BH_EXACT_BFS_MAX", "BH_EXACT_BPW", "BH_WALK_ASM", "BH_WALK_SPLIT", "BH_REORDER_EVERY", "BH_RADIAL_BLOCKS")


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def bodies(n, precision, nb=NB, **kw):
    return MR.state_of(*MR.fixture(n, nb, **kw), precision_is_f32=precision == P.F32)


def modes_as_twin(e, pos, vel, mass, edges, M, rates, what, centre=MR.CENTRE, centre_vel=MR.CENTRE_VEL):
    got = e.azimuthal_modes(edges, M, centre, centre_vel, rates, raw=True)
    planes, ex = MR.modes(pos, vel, mass, centre, centre_vel, edges, M, rates)
    assert got.planes.dtype == np.int64 and got.planes.shape == (MR.n_planes(M, rates), len(edges) + 1)
    assert np.array_equal(got.exponents, ex), (what, got.exponents, ex)
    bad = np.argwhere(got.planes != planes)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ from the twin; first (plane, slot) = {bad[0].tolist()}: " \
                          f"{got.planes[tuple(bad[0])]} != {planes[tuple(bad[0])]}"
    assert int(got.planes[-1].sum()) == len(mass)
    return got


def check_everything(e, precision, n, what):
    import torch
    pos, vel, mass = bodies(n, precision)
    e.upload(pos, vel, mass)
    edges = MR.fixture_edges(NB)
    for M, rates in CONFIGS:
        got = modes_as_twin(e, pos, vel, mass, edges, M, rates, f"{what} M={M} rates={rates}")
        if n > 64:
            assert got.planes[-1, 0] > 0 and got.planes[-1, -1] > 0 and got.planes[0].any()
            assert M == 0 or (got.planes[2 * M - 1].any() and got.planes[2 * M].any())
            assert not rates or (got.planes[1 + 2 * M].any() and got.planes[-2].any())
        # the pieces: the maxima, a deposit with the caller's exponents
        mx = e.modes_max(MR.CENTRE, MR.CENTRE_VEL, M, rates)
        assert np.array_equal(mx, MR.maxima(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, M, rates)), (what, M, rates)
        ex = G.modes_exponents(mx, n) - 3                           # coarser than necessary: still exact integers
        ptr = e.modes_deposit(edges, MR.CENTRE, MR.CENTRE_VEL, ex, M, rates)
        rows = MR.n_planes(M, rates)
        dev = wrap_device(ptr, rows * (NB + 2), "<i8", torch.device("cuda:0")).cpu().numpy().reshape(rows, -1)
        assert np.array_equal(dev, MR.deposit(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, M, rates, ex)), (what, M, rates)
    t = e.modes_times()
    assert t[0] > 0.0 and t[1] > 0.0


# ---- the twin, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_planes_equal_the_twin(monkeypatch, precision, n):
    monkeypatch.delenv("BH_RADIAL_BLOCKS", raising=False)
    with engine(n, precision) as e:
        check_everything(e, precision, n, f"{precision.name} n={n}")


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_ten_trips_per_workgroup(monkeypatch, precision):
    monkeypatch.setenv("BH_RADIAL_BLOCKS", "2")
    with engine(4609, precision) as e:
        check_everything(e, precision, 4609, f"{precision.name} two workgroups")


def test_no_bodies():
    with engine(4, P.F64) as e:
        e.upload(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        got = e.azimuthal_modes(MR.fixture_edges(4), 3, MR.CENTRE, rates=True, raw=True)
        assert not got.planes.any() and list(got.exponents) == [0, 0] and np.isnan(got.amplitude).all()


# ---- the LDS boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,rates", [(2, False), (16, True)])
def test_the_last_private_histogram_and_the_first_tiled(monkeypatch, M, rates):
    monkeypatch.delenv("BH_RADIAL_BLOCKS", raising=False)
    last = MR.largest_private_nb(MR.n_planes(M, rates))
    assert MR.plan(MR.n_planes(M, rates), last)[0] == 0 and MR.plan(MR.n_planes(M, rates), last + 1)[0] > 0
    n = 600
    with engine(n, P.F64) as e:
        for nb in (last, last + 1):
            pos, vel, mass = bodies(n, P.F64, nb)
            e.upload(pos, vel, mass)
            got = modes_as_twin(e, pos, vel, mass, MR.fixture_edges(nb), M, rates, f"M={M} rates={rates} nb={nb}")
            assert (got.planes[-1, 1:-1] > 0).sum() > 100


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("M,rates", [(2, False), (16, True)])
def test_a_range_of_slots_at_and_beyond_the_tile(monkeypatch, M, rates, over):
    """4,096 bins, tile T = floor(65,536 / (8 P)).  600 bodies in three workgroups: the first 256 lie within T + over consecutive
    bins -- T: the workgroup sums them in LDS at an offset; T + 1: it deposits directly -- two bodies at the ends making sure of
    it; the second 256 lie in one bin; the rest are spread over all bins, inside and outside."""
    monkeypatch.delenv("BH_RADIAL_BLOCKS", raising=False)
    nb = 4096
    tile = MR.plan(MR.n_planes(M, rates), nb)[0]
    assert tile == 65536 // (8 * MR.n_planes(M, rates))
    span = tile + over
    rng = np.random.default_rng(span)
    edges = MR.fixture_edges(nb)
    h = 2.0 / nb

    def at(bins):
        r = edges[0] + (bins + rng.uniform(0.3, 0.7, len(bins))) * h
        phi = rng.uniform(0.0, 2.0 * np.pi, len(bins))
        return np.array(MR.CENTRE) + np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)

    a = at(np.concatenate([[700, 700 + span - 1], rng.integers(700, 700 + span, 254)]))
    b = at(np.full(256, 3000))
    c = at(rng.integers(-60, nb + 60, 88))
    pos = np.concatenate([a, b, c])
    n = len(pos)
    vel, mass = rng.normal(size=(n, 2)), 10.0 ** rng.uniform(-3.0, 3.0, n)
    r2, _, _ = MR.contributions(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, 0, False)
    slot = MR.slots_of(r2[:256], MR.squared_edges(edges))
    assert slot.max() - slot.min() + 1 == span
    with engine(n, P.F64) as e:
        e.upload(pos, vel, mass)
        modes_as_twin(e, pos, vel, mass, edges, M, rates, f"M={M} rates={rates} span {span}")


# ---- the order of the bodies in memory ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F32, P.MIXED], ids=lambda p: p.name)
def test_a_physical_reorder_changes_nothing(monkeypatch, precision):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "1")
    n = 4097
    pos, vel, mass = bodies(n, precision, hand=False, decades=1.0)
    edges = MR.fixture_edges(NB)
    with engine(n, precision, dt=1e-3) as a, engine(n, precision, dt=1e-3) as b:
        a.upload(pos, vel, mass)
        a.step(3)
        p1, v1 = a.download()
        import torch
        ptr, _, _, _, eb = a.device_state()
        held = wrap_device(ptr, 2 * n, "<f4" if eb == 4 else "<f8", torch.device("cuda:0")).cpu().numpy().reshape(n, 2).astype(np.float64)
        assert not np.array_equal(held, p1)                       # the device order is not the caller's any more
        b.upload(p1, v1, mass)
        ma = modes_as_twin(a, p1, v1, mass, edges, 6, True, "re-ordered")
        mb = b.azimuthal_modes(edges, 6, MR.CENTRE, MR.CENTRE_VEL, True, raw=True)
        assert np.array_equal(ma.planes, mb.planes) and np.array_equal(ma.exponents, mb.exponents)


@pytest.mark.parametrize("precision", [P.F32, P.F64], ids=lambda p: p.name)
def test_a_permuted_upload_changes_nothing(precision):
    n = 4097
    pos, vel, mass = bodies(n, precision)
    perm = np.random.default_rng(1).permutation(n)
    edges = MR.fixture_edges(1500)
    with engine(n, precision) as a, engine(n, precision) as b:
        a.upload(pos, vel, mass)
        b.upload(pos[perm], vel[perm], mass[perm])
        for M, rates in ((2, False), (4, True)):                  # tiles of 1,365 and of 431 slots for 1,502: LDS and memory
            ma, mb = (x.azimuthal_modes(edges, M, MR.CENTRE, MR.CENTRE_VEL, rates, raw=True) for x in (a, b))
            assert np.array_equal(ma.planes, mb.planes) and np.array_equal(ma.exponents, mb.exponents)
            assert ma.planes[1].any()


# ---- the run is not perturbed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_a_call_between_two_steps_changes_nothing(monkeypatch, precision, n_threads):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")

    def calls(e):
        e.azimuthal_modes(G.radial_edges(1e-3, 0.5, 64), 2, (0.0, 0.0))
        e.azimuthal_modes(G.radial_edges(0.0, 0.5, 2000, "linear"), 4, (0.01, 0.0), (0.0, 1e-5), rates=True)
        e.modes_max((0.0, 0.0), None, 16, True)

    Q.check(precision, n_threads, calls)


# ---- rates, and what the first pass refuses ---------------------------------------------------------------------------------
def code_and_text(call, *args, **kw):
    try:
        call(*args, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


@pytest.mark.parametrize("precision", [P.F32, P.F64_EXACT], ids=lambda p: p.name)
def test_rates_on_and_off(precision):
    n = 257
    pos, vel, mass = bodies(n, precision, at_rest=True)
    edges = MR.fixture_edges(NB)
    with engine(n, precision) as e:
        e.upload(pos, vel, mass)
        got = modes_as_twin(e, pos, vel, mass, edges, 3, True, "at rest", centre_vel=(0.0, 0.0))
        assert got.exponents[1] == 0 and not got.planes[7:14].any() and got.planes[:7].any()
        assert not got.rate_coeff.any()
        moving = modes_as_twin(e, pos, vel, mass, edges, 3, True, "at rest, moving centre")
        assert moving.planes[7].any() and moving.planes[13].any()
        bad = vel.copy()
        bad[7, 1] = float("nan")
        e.upload(pos, bad, mass)
        plain = modes_as_twin(e, pos, bad, mass, edges, 3, False, "a NaN velocity, no rates")      # the velocities are not read
        assert np.array_equal(plain.planes[:7], got.planes[:7])
        assert np.array_equal(e.modes_max(MR.CENTRE, None, 3, False), MR.maxima(pos, bad, mass, MR.CENTRE, (0.0, 0.0), 3, False))
        code, text = code_and_text(e.azimuthal_modes, edges, 3, MR.CENTRE, None, True)
        assert code == ERR_ARG and "first pass" in text and "non-finite" in text, (code, text)
        assert code_and_text(e.modes_max, MR.CENTRE, None, 3, True)[0] == ERR_ARG


def test_errors():
    pos, vel, mass = bodies(65, P.F64)
    edges = MR.fixture_edges(4)
    ctr = MR.CENTRE
    nan, inf = float("nan"), float("inf")
    with engine(65, P.F64) as e:
        assert code_and_text(e.azimuthal_modes, edges, 2, ctr)[0] == ERR_STATE         # before any upload
        assert code_and_text(e.modes_max, ctr)[0] == ERR_STATE
        assert code_and_text(e.modes_deposit, edges, ctr, None, [0, 0])[0] == ERR_STATE
        e.upload(pos, vel, mass)
        assert code_and_text(e.azimuthal_modes, edges, 2, ctr)[0] == 0
        for M in (-1, 17):
            assert code_and_text(e.azimuthal_modes, edges, M, ctr)[0] == ERR_ARG, M
            assert code_and_text(e.modes_max, ctr, None, M)[0] == ERR_ARG, M
            assert code_and_text(e.modes_deposit, edges, ctr, None, [0, 0], M)[0] == ERR_ARG, M
        assert code_and_text(e.azimuthal_modes, edges, 0, ctr)[0] == 0 and code_and_text(e.azimuthal_modes, edges, 16, ctr)[0] == 0
        for bad in ([1.0], [], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, inf], [0.0, nan], [0.0, 1e200], [1e-200, 2e-200],
                    np.arange(4098.0)):                                                # nb = 0, nb = 4,097, not ascending ...
            assert code_and_text(e.azimuthal_modes, bad, 2, ctr)[0] == ERR_ARG, bad
            assert code_and_text(e.modes_deposit, bad, ctr, None, [0, 0])[0] == ERR_ARG, bad
        assert code_and_text(e.azimuthal_modes, np.arange(4097.0), 2, ctr)[0] == 0      # BH_MODES_MAX_BINS itself
        for c in [(nan, 0.0), (0.0, inf)]:
            assert code_and_text(e.azimuthal_modes, edges, 2, c)[0] == ERR_ARG
            assert code_and_text(e.azimuthal_modes, edges, 2, ctr, c)[0] == ERR_ARG
            assert code_and_text(e.modes_max, c)[0] == ERR_ARG
        # exponents that would let a sum leave int64 are refused
        good = G.modes_exponents(e.modes_max(ctr, None, 2, True), 65)
        assert code_and_text(e.modes_deposit, edges, ctr, None, good, 2, True)[0] == 0
        for more in ([1, 0], [0, 1]):
            assert code_and_text(e.modes_deposit, edges, ctr, None, good + np.array(more, dtype=np.int32), 2, True)[0] == ERR_ARG
        # null pointers, on the C-ABI itself
        lib, h = e._lib, e._h
        c2, ed = (C.c_double * 2)(*ctr), (C.c_double * 5)(*edges)
        planes, ex, dev, mx = (C.c_int64 * (11 * 6))(), (C.c_int32 * 2)(), C.c_void_p(), (C.c_double * 2)()
        assert lib.bh_azimuthal_modes(h, None, None, ed, 4, 2, 1, planes, ex) == ERR_ARG
        assert lib.bh_azimuthal_modes(h, c2, None, None, 4, 2, 1, planes, ex) == ERR_ARG
        assert lib.bh_azimuthal_modes(h, c2, None, ed, 4, 2, 1, None, ex) == ERR_ARG
        assert lib.bh_azimuthal_modes(h, c2, None, ed, 4, 2, 1, planes, None) == ERR_ARG
        assert lib.bh_azimuthal_modes(None, c2, None, ed, 4, 2, 1, planes, ex) == ERR_ARG
        assert lib.bh_azimuthal_modes(h, c2, None, ed, 4, 2, 1, planes, ex) == 0        # (no centre velocity: 0)
        assert lib.bh_modes_max(h, c2, None, 2, 1, None) == ERR_ARG and lib.bh_modes_max(h, None, None, 2, 1, mx) == ERR_ARG
        assert lib.bh_modes_deposit(h, c2, None, ed, 4, 2, 1, None, C.byref(dev)) == ERR_ARG
        assert lib.bh_modes_deposit(h, c2, None, ed, 4, 2, 1, ex, None) == ERR_ARG
        assert lib.bh_modes_times(h, None, mx) == ERR_ARG and lib.bh_modes_times(h, mx, mx) == 0
        # an infinite position, an overflowing r2 (a body at 1e200), a NaN mass: with and without rates; w = b / r2 that
        # overflows for a tiny r2: with rates only
        for arr, idx, val in [("p", (3, 0), inf), ("p", (5, 1), 1e200), ("m", 11, nan)]:
            bp, bv, bm = pos.copy(), vel.copy(), mass.copy()
            {"p": bp, "v": bv, "m": bm}[arr][idx] = val
            e.upload(bp, bv, bm)
            for rates in (False, True):
                code, text = code_and_text(e.azimuthal_modes, edges, 2, ctr, None, rates)
                assert code == ERR_ARG and "first pass" in text, (arr, rates, code, text)
                assert code_and_text(e.modes_max, ctr, None, 2, rates)[0] == ERR_ARG
        bp, bv = pos.copy(), vel.copy()
        bp[9], bv[9] = [ctr[0] + 1e-150, ctr[1]], [0.0, 1e160]
        e.upload(bp, bv, mass)
        assert code_and_text(e.azimuthal_modes, edges, 2, ctr, None, False)[0] == 0
        code, text = code_and_text(e.azimuthal_modes, edges, 2, ctr, None, True)
        assert code == ERR_ARG and "first pass" in text and "overflows" in text, (code, text)
        bm = mass.copy()
        bm[4] = -1.0
        e.upload(pos, vel, bm)
        modes_as_twin(e, pos, vel, bm, edges, 2, True, "a negative mass")                # allowed, as for a profile
        with pytest.raises(ValueError):
            e.azimuthal_modes(edges, 2, "centre of gravity")


# ---- known answers ----------------------------------------------------------------------------------------------------------
def test_the_square_and_the_rigid_rotator():
    pos, vel, mass = MR.square(0.75)
    edges = np.array([1.0, 4.0])
    with engine(300, P.F64) as e:
        e.upload(pos, vel, mass)
        got = modes_as_twin(e, pos, vel, mass, edges, 16, True, "square", MR.SQUARE_CENTRE, (0.0, 0.0))
        want = np.array([3.0 if k % 4 == 0 else 0.0 for k in range(17)])
        assert np.array_equal(got.coeff[:, 0], want.astype(np.complex128)) and np.array_equal(got.amplitude[:, 0], want / 3.0)
        assert not got.rate_coeff.any() and list(got.count) == [4]
        centre, centre_vel = (0.75, -0.5), (0.125, -0.0625)
        pos, vel, mass = MR.rotator(257, centre=centre, centre_vel=centre_vel)
        e.upload(pos, vel, mass)
        edges = np.array([0.0, 0.5, 1.0, 2.0, 8.0])
        got = modes_as_twin(e, pos, vel, mass, edges, 16, True, "rotator", centre, centre_vel)
        twin = G.azimuthal_modes_from_planes(*MR.modes(pos, vel, mass, centre, centre_vel, edges, 16, True), edges, 16, True, centre, centre_vel)
        strong = 0
        for k in range(17):
            t, w = got.total(k), twin.total(k)
            assert t.amplitude == w.amplitude and t.phase == w.phase and (t.pattern_speed == w.pattern_speed or k == 0), k
            if k and t.amplitude > 0.01:
                strong += 1
                assert abs(t.pattern_speed - MR.OMEGA) <= 1e-12, (k, t)
        assert strong >= 2
        for k, w in MR.convert(got.planes, got.exponents, 16, True).items():
            assert np.array_equal(getattr(got, k), w, equal_nan=True), k
        assert np.abs(got.rate_coeff[0].real / got.mass - MR.OMEGA).max() <= 1e-12
        assert got.centre == centre and got.centre_velocity == centre_vel and got.m_max == 16


def test_the_named_centres(init1024):
    m, p, v = init1024
    with engine(1024, P.F64_EXACT) as e:
        e.upload(p, v, m)
        dc, com = e.density_centre(6), np.array(e.energy().com)
        edges = G.radial_edges(1e-3, 0.2, 16)
        for name, c in (("density", dc), ("com", com)):
            a, b = e.azimuthal_modes(edges, centre=name, raw=True), e.azimuthal_modes(edges, 4, c, raw=True)
            assert a.centre == tuple(c) and a.m_max == 4 and np.array_equal(a.planes, b.planes)
        assert e.azimuthal_modes(edges).planes is None


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def read_rows(path, head=True):
    lines = open(path).read().splitlines()
    rows = np.array([[float(t) for t in l.split(",")] for l in lines[1 if head else 0:]])
    return (lines[0], rows) if head else rows


def test_project_modes_and_bar_files(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), modes_file="modes.csv", modes_bins=16, modes_max=3,
                                         bar_file="bar.csv", bar_every=1, **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flags nothing changes: every other output file is the same, byte for byte
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    assert not (b / "modes.csv").exists() and not (b / "bar.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    head, rows = read_rows(a / "modes.csv")
    assert head == "# r_lo,r_hi,count,mass,amp_1,phase_1,amp_2,phase_2,amp_3,phase_3" and rows.shape == (16, 10)
    bar = read_rows(a / "bar.csv", head=False)
    assert bar.shape == (3, 7) and list(bar[:, 0]) == [0.0, 1.0, 2.0] and list(bar[:, 1]) == [0.0, 1.0, 2.0]
    # the API's numbers of the same states
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        c = e.density_centre(6)
        md = e.azimuthal_modes(project.profile_edges(16, None, "log", pa, c), 3, c)
        t2 = e.azimuthal_modes(project.profile_edges(1, None, "linear", pa, c), 2, c, rates=True).total(2)
        e.upload(p, v, m)
        c0 = e.density_centre(6)
        t0 = e.azimuthal_modes(project.profile_edges(1, None, "linear", p, c0), 2, c0, rates=True).total(2)
    cols = [md.edges[:-1], md.edges[1:], md.count, md.mass]
    for k in (1, 2, 3):
        cols += [md.amplitude[k], md.phase[k]]
    for k, col in enumerate(cols):
        assert np.array_equal(rows[:, k], col, equal_nan=True), k
    assert np.array_equal(bar[2, 2:], [*c, *t2]) and np.array_equal(bar[0, 2:], [*c0, *t0])
    assert 0.0 <= t2.amplitude < 1.0 and math.isfinite(t2.pattern_speed)
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--modes-file", "main.csv",
                             "--modes-bins", "8", "--modes-max", "2", "--modes-range", "0", "0.1", "--modes-spacing", "linear",
                             "--modes-centre", "com", "--bar-file", "bmain.csv", "--bar-mode", "4", "--bar-range", "0.01", "0.1",
                             "--bar-centre", "0.01", "-0.02"]) == 0
    finally:
        os.chdir(cwd)
    head, rows = read_rows(tmp_path / "main.csv")
    bar = read_rows(tmp_path / "bmain.csv", head=False)
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        md = e.azimuthal_modes(G.radial_edges(0.0, 0.1, 8, "linear"), 2, "com")
        t4 = e.azimuthal_modes(np.array([0.01, 0.1]), 4, (0.01, -0.02), rates=True).total(4)
    assert head == "# r_lo,r_hi,count,mass,amp_1,phase_1,amp_2,phase_2"
    assert np.array_equal(rows[:, 2], md.count) and np.array_equal(rows[:, 3], md.mass) and np.array_equal(rows[:, 6], md.amplitude[2], equal_nan=True)
    assert bar.shape == (2, 7) and np.array_equal(bar[1, 2:], [0.01, -0.02, *t4])


# ---- distributed ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2])
def test_let_stepper_modes(tmp_path, world):
    """World processes over gloo on the one GPU (with this one: at most three with the device open), each with its own timeout.
    After two steps and a rebalance() every rank's planes are the twin's of the gathered bodies."""
    port = _free_port()
    script = os.path.join(HERE, "modes_ranks.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), str(tmp_path)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{o[-3000:]}"
    import modes_ranks as RR
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([x["ids"] for x in ranks])
    assert sorted(ids.tolist()) == list(range(RR.N))
    if world > 1:
        assert all(len(x["ids"]) > 0 for x in ranks)
    assert all(int(x["raised"]) == (4 if world > 1 else 1) for x in ranks)    # (one rank cannot disagree with itself)
    pos, vel, mass = (np.concatenate([x[k] for x in ranks]) for k in ("pos", "vel", "mass"))
    edges = MR.fixture_edges(RR.NB)
    planes, ex = MR.modes(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, RR.M, True)
    plain, plain_e = MR.modes(pos, vel, mass, MR.CENTRE, (0.0, 0.0), edges, 2, False)
    conv = MR.convert(planes, ex, RR.M, True)
    assert planes[-1, 1:-1].all()
    for r, x in enumerate(ranks):
        assert np.array_equal(x["planes"], planes) and np.array_equal(x["e"], ex), r
        assert np.array_equal(x["plain_planes"], plain) and np.array_equal(x["plain_e"], plain_e), r
        assert np.array_equal(x["amplitude"], conv["amplitude"], equal_nan=True)
        assert np.array_equal(x["speed"], conv["pattern_speed"], equal_nan=True)
        assert np.array_equal(x["com"], ranks[0]["com"]) and int(x["com_m"]) == 4
        assert np.array_equal(x["com_planes"], MR.modes(pos, vel, mass, x["com"], (0.0, 0.0), edges, 4, False)[0])
