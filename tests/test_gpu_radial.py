"""bh_radial_profile, bh_radial_max, bh_radial_deposit, bh_lagrangian_radii and bh_radial_select on the device, held to the
numpy twin tests/radial_ref.py: every comparison is np.array_equal on the int64 planes, the exponents, and the r2, count and
mass of the radii.

  * all four precisions x n in {0, 1, 63, 64, 65, 255, 256, 257, 4097} x nb in {1, 2, 33, 1022, 1023, 4096} (1,022 bins: the
    last whose 1,024 slots the workgroup keeps in LDS; 1,023: the first that falls back), 4,097 again with BH_RADIAL_BLOCKS=2
    (nine trips per workgroup), on the fixture of radial_ref.fixture (bodies on edges, at the centre, with a subnormal r2,
    mirror images, inside edges[0] and beyond edges[nb], a massless one);
  * bodies at rest: planes 1-4 are zero with exponent 0; plane 0 summed over the slots is W;
  * with more slots than LDS holds: a workgroup whose bodies span at most 1,024 slots, and one whose bodies span more;
  * the results do not depend on the order of the bodies in memory (a physical re-order, a permuted upload);
  * a call between two steps changes nothing of the run;
  * the errors of include/bhgpu.h;
  * the derived quantities on a hand-made ring with known rotation;
  * project.py --profile-file and --lagrange-file;
  * LetStepper.radial_profile and .lagrangian_radii over gloo, world 1 and 2."""
import ctypes as C
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
import quiet_case as Q  # noqa: E402
import radial_ref as R  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5
HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
BINS = [1, 2, 33, 1022, 1023, 4096]
ENV = ("BH_EXACT_BFS_MAX", "BH_EXACT_BPW", "BH_WALK_ASM", "BH_WALK_SPLIT", "BH_REORDER_EVERY", "BH_RADIAL_BLOCKS")


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def bodies(n, precision, nb=33, **kw):
    return R.state_of(*R.fixture(n, nb, **kw), precision_is_f32=precision == P.F32)


def profile_as_twin(e, pos, vel, mass, edges, what, centre=R.CENTRE, centre_vel=R.CENTRE_VEL):
    got = e.radial_profile(edges, centre, centre_vel, raw=True)
    planes, ex = R.profile(pos, vel, mass, centre, centre_vel, edges)
    assert got.planes.dtype == np.int64 and got.planes.shape == (6, len(edges) + 1)
    assert np.array_equal(got.exponents, ex), (what, got.exponents, ex)
    bad = np.argwhere(got.planes != planes)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ from the twin; first (plane, slot) = {bad[0].tolist()}: " \
                          f"{got.planes[tuple(bad[0])]} != {planes[tuple(bad[0])]}"
    assert int(got.planes[5].sum()) == len(mass)
    return got


def radii_as_twin(e, pos, mass, fractions, what, centre=R.CENTRE):
    got = e.lagrangian_radii(fractions, centre)
    r2, cnt, units, e0 = R.lagrangian(pos, mass, centre, fractions)
    assert got.exponent == e0, (what, got.exponent, e0)
    assert np.array_equal(got.r2, r2, equal_nan=True), (what, got.r2, r2)
    assert np.array_equal(got.count, cnt) and np.array_equal(got.mass_units, units), (what, got.count, cnt, got.mass_units, units)
    assert np.array_equal(got.r, np.sqrt(r2), equal_nan=True)
    return got


def tie_fraction(pos, mass, centre=R.CENTRE):
    """A fraction whose threshold falls inside the four mirror images of the fixture (equal r2, mass 8 each): the cumulative
    mass below them plus one and a half of theirs, over the total."""
    r2, w, _ = R.weights(pos, mass, centre)
    tie = r2 == r2[6]
    assert tie.sum() == 4 and (w[tie] == w[6]).all()
    return (float(w[r2 < r2[6]].sum()) + 1.5 * float(w[6])) / float(sum(int(x) for x in w))


def check_everything(e, precision, n, what):
    for nb in BINS:
        pos, vel, mass = bodies(n, precision, nb)
        e.upload(pos, vel, mass)
        edges = R.fixture_edges(nb)
        got = profile_as_twin(e, pos, vel, mass, edges, f"{what} nb={nb}")
        # plane 0 summed over the slots is W, in the exponent the radii use
        _, w, e0 = R.weights(pos, mass, R.CENTRE)
        assert got.exponents[0] == e0 and sum(int(v) for v in got.planes[0]) == sum(int(v) for v in w)
        if n > 64:
            assert got.planes[5, 0] > 0 and got.planes[5, -1] > 0 and got.planes[0].any() and got.planes[2].any()
    fractions = [0.01, 0.1, 0.5, 0.9, 1.0, 0.5, 1e-300]
    if n > 64:
        fractions.append(tie_fraction(pos, mass))
    got = radii_as_twin(e, pos, mass, fractions, what)
    if n > 64:                                                      # the tie: all four mirror images are inside together
        r2, _, _ = R.weights(pos, mass, R.CENTRE)
        assert got.r2[-1] == r2[6] and got.count[-1] == (r2 <= r2[6]).sum() == (r2 < r2[6]).sum() + 4
    if n == 0:
        assert np.isnan(got.r2).all() and not got.count.any()
    # the pieces: the maxima, a deposit with the caller's exponents, one select round
    mx = e.radial_max(R.CENTRE, R.CENTRE_VEL)
    assert np.array_equal(mx, R.maxima(pos, vel, mass, R.CENTRE, R.CENTRE_VEL))
    import torch
    ex = G.radial_exponents(mx, n) - 3                              # coarser than necessary: still exact integers
    ptr = e.radial_deposit(edges, R.CENTRE, R.CENTRE_VEL, ex)
    dev = wrap_device(ptr, 6 * (len(edges) + 1), "<i8", torch.device("cuda:0")).cpu().numpy().reshape(6, -1)
    assert np.array_equal(dev, R.deposit(pos, vel, mass, R.CENTRE, R.CENTRE_VEL, edges, ex))
    r2, w, e0 = R.weights(pos, mass, R.CENTRE)
    keys = sorted(set((r2.view(np.uint64) >> np.uint64(48)).tolist()))[:32] or [0]
    ptr = e.radial_select(R.CENTRE, e0, 2, keys)
    dev = wrap_device(ptr, len(keys) * 512, "<i8", torch.device("cuda:0")).cpu().numpy().reshape(len(keys), 256, 2)
    assert np.array_equal(dev, R.select_hist(r2, w, 2, keys))


# ---- the twin, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_planes_and_radii_equal_the_twin(monkeypatch, precision, n):
    monkeypatch.delenv("BH_RADIAL_BLOCKS", raising=False)
    with engine(n, precision) as e:
        check_everything(e, precision, n, f"{precision.name} n={n}")


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_nine_trips_per_workgroup(monkeypatch, precision):
    monkeypatch.setenv("BH_RADIAL_BLOCKS", "2")
    with engine(4097, precision) as e:
        check_everything(e, precision, 4097, f"{precision.name} two workgroups")


@pytest.mark.parametrize("precision", [P.F32, P.F64_EXACT], ids=lambda p: p.name)
def test_bodies_at_rest_leave_the_velocity_planes_zero(precision):
    n = 257
    pos, vel, mass = bodies(n, precision, at_rest=True)
    with engine(n, precision) as e:
        e.upload(pos, vel, mass)
        got = profile_as_twin(e, pos, vel, mass, R.fixture_edges(33), "at rest", centre_vel=(0.0, 0.0))
        assert list(got.exponents[1:]) == [0, 0, 0, 0] and not got.planes[1:5].any() and got.planes[0].any()
        moving = profile_as_twin(e, pos, vel, mass, R.fixture_edges(33), "at rest, moving centre")
        assert moving.planes[1].any() and moving.planes[4].any()


def test_thirty_two_fractions_take_four_launches_a_round():
    n = 4097
    pos, vel, mass = bodies(n, P.F64)
    with engine(n, P.F64) as e:
        e.upload(pos, vel, mass)
        got = radii_as_twin(e, pos, mass, np.arange(1, 33) / 32.0, "32 fractions")
        assert len(set(got.r2.tolist())) > 16
        radii_as_twin(e, pos, mass, [0.9, 0.1, 0.5], "unordered")


@pytest.mark.parametrize("span", [1000, 1024, 1025, 1100])
def test_more_slots_than_lds_holds(monkeypatch, span):
    """4,096 bins.  600 bodies in three workgroups: the first 256 lie within `span` consecutive bins -- 1,000: the workgroup sums
    them in LDS at an offset; 1,100: it deposits directly -- two bodies at the ends making sure of it; 1,024 and 1,025: the last
    range the 1,024 slots of the LDS histogram hold and the first they do not; the second 256 lie in one bin; the rest are
    spread over all bins, inside and outside."""
    monkeypatch.delenv("BH_RADIAL_BLOCKS", raising=False)
    rng = np.random.default_rng(span)
    nb = 4096
    edges = R.fixture_edges(nb)
    h = 2.0 / nb

    def at(bins):
        r = edges[0] + (bins + rng.uniform(0.3, 0.7, len(bins))) * h
        phi = rng.uniform(0.0, 2.0 * np.pi, len(bins))
        return np.array(R.CENTRE) + np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)

    a = at(np.concatenate([[700, 700 + span - 1], rng.integers(700, 700 + span, 254)]))
    b = at(np.full(256, 3000))
    c = at(rng.integers(-60, nb + 60, 88))
    pos = np.concatenate([a, b, c])
    n = len(pos)
    vel, mass = rng.normal(size=(n, 2)), 10.0 ** rng.uniform(-3.0, 3.0, n)
    r2, _ = R.moments(pos, vel, mass, R.CENTRE)
    slot = R.slots_of(r2[:256], R.squared_edges(edges))
    assert slot.max() - slot.min() + 1 == span
    with engine(n, P.F64) as e:
        e.upload(pos, vel, mass)
        profile_as_twin(e, pos, vel, mass, edges, f"span {span}")


# ---- the order of the bodies in memory ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F32, P.MIXED], ids=lambda p: p.name)
def test_a_physical_reorder_changes_nothing(monkeypatch, precision):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")
    n = 4097
    pos, vel, mass = bodies(n, precision, hand=False, decades=1.0)
    edges = R.fixture_edges(33)
    with engine(n, precision, dt=1e-3) as a, engine(n, precision, dt=1e-3) as b:
        a.upload(pos, vel, mass)
        a.step(3)
        p1, v1 = a.download()
        import torch
        ptr, _, _, _, eb = a.device_state()
        held = wrap_device(ptr, 2 * n, "<f4" if eb == 4 else "<f8", torch.device("cuda:0")).cpu().numpy().reshape(n, 2).astype(np.float64)
        assert not np.array_equal(held, p1)                       # the device order is not the caller's any more
        b.upload(p1, v1, mass)
        pa = profile_as_twin(a, p1, v1, mass, edges, "re-ordered")
        pb = b.radial_profile(edges, R.CENTRE, R.CENTRE_VEL, raw=True)
        assert np.array_equal(pa.planes, pb.planes) and np.array_equal(pa.exponents, pb.exponents)
        la, lb = radii_as_twin(a, p1, mass, (0.01, 0.1, 0.5, 0.9), "re-ordered"), b.lagrangian_radii(centre=R.CENTRE)
        assert np.array_equal(la.r2, lb.r2) and np.array_equal(la.count, lb.count) and np.array_equal(la.mass_units, lb.mass_units)


@pytest.mark.parametrize("precision", [P.F32, P.F64], ids=lambda p: p.name)
def test_a_permuted_upload_changes_nothing(precision):
    n = 4097
    pos, vel, mass = bodies(n, precision)
    perm = np.random.default_rng(1).permutation(n)
    edges = R.fixture_edges(1023)
    with engine(n, precision) as a, engine(n, precision) as b:
        a.upload(pos, vel, mass)
        b.upload(pos[perm], vel[perm], mass[perm])
        pa, pb = (x.radial_profile(edges, R.CENTRE, R.CENTRE_VEL, raw=True) for x in (a, b))
        assert np.array_equal(pa.planes, pb.planes) and np.array_equal(pa.exponents, pb.exponents)
        la, lb = (x.lagrangian_radii(centre=R.CENTRE) for x in (a, b))
        assert np.array_equal(la.r2, lb.r2) and np.array_equal(la.count, lb.count) and np.array_equal(la.mass_units, lb.mass_units)


# ---- the run is not perturbed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_a_call_between_two_steps_changes_nothing(monkeypatch, precision, n_threads):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")

    def plain(n):
        return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=precision, n_threads=n_threads))

    def calls(e):
        e.radial_profile(G.radial_edges(1e-3, 0.5, 64), (0.0, 0.0))
        e.radial_profile(G.radial_edges(0.0, 0.5, 2000, "linear"), (0.01, 0.0), (0.0, 1e-5))
        e.lagrangian_radii(centre=(0.0, 0.0))

    Q.check(precision, n_threads, calls)
    m, p, v = Q.bodies()
    with plain(Q.N) as e, plain(Q.N) as control:
        for x in (e, control):
            x.upload(p, v, m)
        e.step(3)
        calls(e)
        e.step(3)
        control.step(6)
        (x1, v1), (x0, v0) = e.download(), control.download()
        assert np.array_equal(x1, x0) and np.array_equal(v1, v0)
        s1, s0 = e.stats(), control.stats()
        for k in Q.KEPT:
            assert getattr(s1, k) == getattr(s0, k), (k, getattr(s0, k), getattr(s1, k))


# ---- errors ---------------------------------------------------------------------------------------------------------------
def code_and_text(call, *args, **kw):
    try:
        call(*args, **kw)
    except G.BhError as err:
        return err.code, str(err)
    return 0, ""


def test_errors():
    pos, vel, mass = bodies(65, P.F64)
    edges = R.fixture_edges(4)
    ctr = R.CENTRE
    nan, inf = float("nan"), float("inf")
    with engine(65, P.F64) as e:
        assert code_and_text(e.radial_profile, edges, ctr)[0] == ERR_STATE            # before any upload
        assert code_and_text(e.radial_max, ctr)[0] == ERR_STATE
        assert code_and_text(e.radial_deposit, edges, ctr, None, [0] * 5)[0] == ERR_STATE
        assert code_and_text(e.lagrangian_radii, (0.5,), ctr)[0] == ERR_STATE
        assert code_and_text(e.radial_select, ctr, 0, 0, [0])[0] == ERR_STATE
        e.upload(pos, vel, mass)
        assert code_and_text(e.radial_profile, edges, ctr)[0] == 0
        for bad in ([1.0], [], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, inf], [0.0, nan], [0.0, 1e200], [1e-200, 2e-200],
                    np.arange(4098.0)):
            assert code_and_text(e.radial_profile, bad, ctr)[0] == ERR_ARG, bad
            assert code_and_text(e.radial_deposit, bad, ctr, None, [0] * 5)[0] == ERR_ARG, bad
        assert code_and_text(e.radial_profile, np.arange(4097.0), ctr)[0] == 0       # BH_RADIAL_MAX_BINS itself
        for c in [(nan, 0.0), (0.0, inf)]:
            assert code_and_text(e.radial_profile, edges, c)[0] == ERR_ARG
            assert code_and_text(e.radial_profile, edges, ctr, c)[0] == ERR_ARG
            assert code_and_text(e.radial_max, c)[0] == ERR_ARG
            assert code_and_text(e.lagrangian_radii, (0.5,), c)[0] == ERR_ARG
            assert code_and_text(e.radial_select, c, 0, 0, [0])[0] == ERR_ARG
        for f in ([], [0.0], [-0.5], [1.5], [nan], [0.5] * 33):
            assert code_and_text(e.lagrangian_radii, f, ctr)[0] == ERR_ARG, f
        assert code_and_text(e.lagrangian_radii, [0.5] * 32, ctr)[0] == 0
        _, _, e0 = R.weights(pos, mass, ctr)
        for rnd, pre in [(-1, [0]), (8, [0]), (0, [1]), (0, [0, 1]), (1, []), (1, [3, 3]), (1, [256]), (2, list(range(33)))]:
            assert code_and_text(e.radial_select, ctr, e0, rnd, pre)[0] == ERR_ARG, (rnd, pre)
        assert code_and_text(e.radial_select, ctr, e0, 1, [3, 4])[0] == 0
        assert code_and_text(e.radial_select, ctr, e0 + 1, 0, [0])[0] == ERR_ARG     # a sum could leave int64
        # exponents that would let a sum leave int64 are refused
        good = G.radial_exponents(e.radial_max(ctr), 65)
        assert code_and_text(e.radial_deposit, edges, ctr, None, good)[0] == 0
        assert code_and_text(e.radial_deposit, edges, ctr, None, good + np.array([0, 0, 1, 0, 0], dtype=np.int32))[0] == ERR_ARG
        # null pointers, on the C-ABI itself
        lib, h = e._lib, e._h
        c2, ed = (C.c_double * 2)(*ctr), (C.c_double * 5)(*edges)
        planes, ex, dev = (C.c_int64 * 36)(), (C.c_int32 * 5)(), C.c_void_p()
        r2, cnt, ms, e1 = (C.c_double * 1)(), (C.c_int64 * 1)(), (C.c_int64 * 1)(), C.c_int32()
        fr, pre, mx = (C.c_double * 1)(0.5), (C.c_uint64 * 1)(0), (C.c_double * 5)()
        assert lib.bh_radial_profile(h, None, None, ed, 4, planes, ex) == ERR_ARG
        assert lib.bh_radial_profile(h, c2, None, None, 4, planes, ex) == ERR_ARG
        assert lib.bh_radial_profile(h, c2, None, ed, 4, None, ex) == ERR_ARG
        assert lib.bh_radial_profile(h, c2, None, ed, 4, planes, None) == ERR_ARG
        assert lib.bh_radial_profile(None, c2, None, ed, 4, planes, ex) == ERR_ARG
        assert lib.bh_radial_profile(h, c2, None, ed, 4, planes, ex) == 0            # (no centre velocity: 0)
        assert lib.bh_radial_max(h, c2, None, None) == ERR_ARG and lib.bh_radial_max(h, None, None, mx) == ERR_ARG
        assert lib.bh_radial_deposit(h, c2, None, ed, 4, None, C.byref(dev)) == ERR_ARG
        assert lib.bh_radial_deposit(h, c2, None, ed, 4, ex, None) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, None, fr, 1, r2, cnt, ms, C.byref(e1)) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, None, 1, r2, cnt, ms, C.byref(e1)) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, fr, 1, None, cnt, ms, C.byref(e1)) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, fr, 1, r2, None, ms, C.byref(e1)) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, fr, 1, r2, cnt, None, C.byref(e1)) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, fr, 1, r2, cnt, ms, None) == ERR_ARG
        assert lib.bh_lagrangian_radii(h, c2, fr, 1, r2, cnt, ms, C.byref(e1)) == 0
        assert lib.bh_radial_select(h, c2, e0, 0, None, 1, C.byref(dev)) == ERR_ARG
        assert lib.bh_radial_select(h, c2, e0, 0, pre, 1, None) == ERR_ARG
        assert lib.bh_radial_times(h, None, mx, None) == ERR_ARG and lib.bh_radial_times(h, mx, mx, None) == 0
        # a NaN velocity, an infinite position, an overflowing moment, an overflowing r2, a negative mass
        for arr, idx, val, radii_too in [("v", (7, 1), nan, False), ("p", (3, 0), inf, True), ("v", (9, 0), 1e200, False),
                                         ("p", (5, 1), 1e200, True), ("m", 11, nan, True)]:
            bp, bv, bm = pos.copy(), vel.copy(), mass.copy()
            {"p": bp, "v": bv, "m": bm}[arr][idx] = val
            e.upload(bp, bv, bm)
            code, text = code_and_text(e.radial_profile, edges, ctr)
            assert code == ERR_ARG and "non-finite" in text, (code, text)
            assert code_and_text(e.radial_max, ctr)[0] == ERR_ARG
            code, text = code_and_text(e.lagrangian_radii, (0.5,), ctr)
            assert (code == ERR_ARG and "non-finite" in text) if radii_too else code == 0, (arr, code, text)
            assert code_and_text(e.radial_select, ctr, 0, 0, [0])[0] == (ERR_ARG if radii_too else 0)
        bm = mass.copy()
        bm[4] = -1.0
        e.upload(pos, vel, bm)
        assert code_and_text(e.radial_profile, edges, ctr)[0] == 0                    # a profile takes a negative mass ...
        code, text = code_and_text(e.lagrangian_radii, (0.5,), ctr)
        assert code == ERR_ARG and "negative mass" in text                            # ... the radii do not
        code, text = code_and_text(e.radial_select, ctr, 0, 0, [0])
        assert code == ERR_ARG and "negative mass" in text
        e.upload(pos, vel, mass)
        assert code_and_text(e.lagrangian_radii, (0.5,), ctr)[0] == 0
        with pytest.raises(ValueError):
            e.radial_profile(edges, "centre of gravity")


# ---- the derived quantities -----------------------------------------------------------------------------------------------
def test_a_ring_with_known_rotation():
    """Four bodies of mass 1 at radius 1 on the axes about (3, -2), turning at angular speed 1/2 (vt = 1/2, vr = 0), four at radius
    2 moving radially, two outwards and two inwards at 1/4 (vr = 0 in the mean, sigma_r = 1/4), the centre itself moving at
    (0.5, 0.25).  Every number is a binary fraction: the expected values are exact."""
    c, u = np.array([3.0, -2.0]), np.array([0.5, 0.25])
    unit = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    tang = np.array([[0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [1.0, 0.0]])
    pos = np.concatenate([c + unit, c + 2.0 * unit])
    vel = np.concatenate([u + 0.5 * tang, u + 0.25 * unit * np.array([[1.0], [1.0], [-1.0], [-1.0]])])
    mass = np.ones(8)
    edges = np.array([0.5, 1.5, 2.5])
    with engine(8, P.F64) as e:
        e.upload(pos, vel, mass)
        got = e.radial_profile(edges, c, u)
        assert got.planes is None and got.exponents is None       # raw=False
        lr = e.lagrangian_radii((0.5, 0.51, 1.0), c)
    want = R.convert(*R.profile(pos, vel, mass, c, u, edges), edges)
    for k, w in want.items():
        assert np.array_equal(getattr(got, k), w, equal_nan=True), k
    assert list(got.count) == [4, 4] and list(got.mass) == [4.0, 4.0] and list(got.r_mid) == [1.0, 2.0]
    assert list(got.vt) == [0.5, 0.0] and list(got.vr) == [0.0, 0.0]
    assert list(got.sigma_t) == [0.0, 0.0] and list(got.sigma_r) == [0.0, 0.25]
    assert np.isnan(got.anisotropy[0]) and got.anisotropy[1] == 1.0
    assert list(got.sigma) == [4.0 / (np.pi * 2.0), 4.0 / (np.pi * 4.0)]
    assert list(got.enclosed) == [0.0, 4.0, 8.0] and got.mass_inside == 0.0 and got.mass_outside == 0.0
    assert got.centre == (3.0, -2.0) and got.centre_velocity == (0.5, 0.25)
    assert list(lr.r) == [1.0, 2.0, 2.0] and list(lr.count) == [4, 8, 8] and list(lr.mass) == [4.0, 8.0, 8.0]


def test_the_named_centres(init1024):
    m, p, v = init1024
    with engine(1024, P.F64_EXACT) as e:
        e.upload(p, v, m)
        dc, com = e.density_centre(6), np.array(e.energy().com)
        edges = G.radial_edges(1e-3, 0.2, 16)
        for name, c in (("density", dc), ("com", com)):
            a, b = e.radial_profile(edges, name, raw=True), e.radial_profile(edges, c, raw=True)
            assert a.centre == tuple(c) and np.array_equal(a.planes, b.planes)
            assert np.array_equal(e.lagrangian_radii(centre=name).r2, e.lagrangian_radii(centre=c).r2)
        assert list(e.lagrangian_radii().fractions) == [0.01, 0.1, 0.5, 0.9]
        t = e.radial_times()
        assert t[0] > 0.0 and t[1] > 0.0 and (t[2] > 0.0).all()


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def read_rows(path, head=True):
    lines = open(path).read().splitlines()
    rows = np.array([[float(t) for t in l.split(",")] for l in lines[1 if head else 0:]])
    return (lines[0], rows) if head else rows


def test_project_profile_and_lagrange_files(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", energy_file="energy.csv")
    fr = (0.1, 0.5, 0.9)
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), profile_file="profile.csv", profile_bins=16,
                                         lagrange_file="lagrange.csv", lagrange_fractions=fr, lagrange_every=1, **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flags nothing changes: every other output file is the same, byte for byte
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    assert not (b / "profile.csv").exists() and not (b / "lagrange.csv").exists()
    for name in ("pos.txt", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    head, rows = read_rows(a / "profile.csv")
    assert head == "# r_lo,r_hi,count,sigma,vr,vt,sigma_r,sigma_t" and rows.shape == (16, 8)
    lag = read_rows(a / "lagrange.csv", head=False)
    assert lag.shape == (3, 4 + len(fr)) and list(lag[:, 0]) == [0.0, 1.0, 2.0] and list(lag[:, 1]) == [0.0, 1.0, 2.0]
    # the API's numbers of the same states
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        c = e.density_centre(6)
        pr = e.radial_profile(project.profile_edges(16, None, "log", pa, c), c)
        lr = e.lagrangian_radii(fr, "density")
        e.upload(p, v, m)
        l0 = e.lagrangian_radii(fr, "density")
    cols = (pr.edges[:-1], pr.edges[1:], pr.count, pr.sigma, pr.vr, pr.vt, pr.sigma_r, pr.sigma_t)
    for k, col in enumerate(cols):
        assert np.array_equal(rows[:, k], col, equal_nan=True), k
    assert pr.count_inside + pr.count.sum() == 1024 and pr.count_outside == 0   # (the farthest body is just inside the last edge)
    assert np.array_equal(lag[2, 2:], [*lr.centre, *lr.r]) and np.array_equal(lag[0, 2:], [*l0.centre, *l0.r])
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--profile-file", "main.csv",
                             "--profile-bins", "8", "--profile-range", "0", "0.1", "--profile-spacing", "linear",
                             "--profile-centre", "com", "--lagrange-file", "lmain.csv", "--lagrange-centre", "0.01", "-0.02",
                             "--lagrange-fractions", "0.25", "0.75"]) == 0
    finally:
        os.chdir(cwd)
    head, rows = read_rows(tmp_path / "main.csv")
    lag = read_rows(tmp_path / "lmain.csv", head=False)
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        pr = e.radial_profile(G.radial_edges(0.0, 0.1, 8, "linear"), "com")
        lr = e.lagrangian_radii((0.25, 0.75), (0.01, -0.02))
    assert head == "# r_lo,r_hi,count,sigma,vr,vt,sigma_r,sigma_t"
    assert np.array_equal(rows[:, 2], pr.count) and np.array_equal(rows[:, 3], pr.sigma) and np.array_equal(rows[:, 5], pr.vt, equal_nan=True)
    assert lag.shape == (2, 6) and np.array_equal(lag[1, 2:], [0.01, -0.02, *lr.r])


# ---- distributed ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2])
def test_let_stepper_radial(tmp_path, world):
    """World processes over gloo on the one GPU (with this one: at most three with the device open), each with its own timeout.
    After two steps and a rebalance() every rank's profile and radii are the twin's of the gathered bodies."""
    port = _free_port()
    script = os.path.join(HERE, "radial_ranks.py")
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
    import radial_ranks as RR
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([x["ids"] for x in ranks])
    assert sorted(ids.tolist()) == list(range(RR.N))
    if world > 1:
        assert all(len(x["ids"]) > 0 for x in ranks)
    assert all(int(x["raised"]) == (3 if world > 1 else 1) for x in ranks)    # (one rank cannot disagree with itself)
    pos, vel, mass = (np.concatenate([x[k] for x in ranks]) for k in ("pos", "vel", "mass"))
    edges = R.fixture_edges(RR.NB)
    planes, ex = R.profile(pos, vel, mass, R.CENTRE, R.CENTRE_VEL, edges)
    r2, cnt, units, e0 = R.lagrangian(pos, mass, R.CENTRE, RR.FRACTIONS)
    assert planes[5, 1:-1].all()
    for r, x in enumerate(ranks):
        assert np.array_equal(x["planes"], planes) and np.array_equal(x["e"], ex), r
        assert np.array_equal(x["sigma"], R.convert(planes, ex, edges)["sigma"])
        assert np.array_equal(x["r2"], r2) and np.array_equal(x["count"], cnt) and np.array_equal(x["units"], units), r
        assert int(x["e0"]) == e0
        assert np.array_equal(x["com"], ranks[0]["com"])
        assert np.array_equal(x["com_planes"], R.profile(pos, vel, mass, x["com"], (0.0, 0.0), edges)[0])
