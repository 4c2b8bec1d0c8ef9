"""The definition of the azimuthal modes (include/bhgpu.h) checked without a GPU: the numpy twin tests/modes_ref.py against the
same definition body by body in exact arithmetic, against an independent trigonometric formulation, and on configurations with
known answers; the conversion of engine.azimuthal_modes_from_planes (amplitude, phase, pattern speed, total(),
pattern_speed_between()) on the twin's planes; the properties a distributed call relies on; the LDS selector."""
import math
import os
import subprocess

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
import modes_ref as MR

EDGES4 = np.array([0.0, 0.5, 1.0, 2.0, 8.0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-nbody-simulation_amd", "csrc")


def result(pos, vel, mass, centre, centre_vel, edges, M, rates, raw=True):
    planes, e = MR.modes(pos, vel, mass, centre, centre_vel, edges, M, rates)
    return G.azimuthal_modes_from_planes(planes, e, edges, M, rates, centre, centre_vel, raw)


@pytest.mark.parametrize("rates", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_the_twin_is_the_definition_body_by_body(n, rates):
    pos, vel, mass = MR.fixture(n, 8)
    edges = MR.fixture_edges(8)
    planes, e = MR.modes(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, 5, rates)
    slow, es = MR.slow_modes(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, 5, rates)
    assert list(e) == es
    assert planes.shape == (MR.n_planes(5, rates), 10) and planes.tolist() == slow
    assert int(planes[-1].sum()) == n


@pytest.mark.parametrize("n", [257, 5000])
def test_against_trigonometric_functions(n):
    """|A_k - sum m exp(i k atan2(dy, dx))| <= 1e-13 A_0 for every k <= 16, per bin and for the whole system (measured: about
    1e-16; the bound leaves room for atan2's own error)."""
    pos, _, mass = MR.rotator(n, seed=n)
    centre = (0.75, -0.5)
    planes, e = MR.modes(pos, None, mass, centre, (0.0, 0.0), EDGES4, 16, False)
    a, _ = MR.values(planes, e, 16, False)
    re, im = MR.trig_sums(pos, mass, centre, EDGES4, 16)
    worst = 0.0
    for sel in [slice(s, s + 1) for s in range(len(EDGES4) + 1)] + [slice(None)]:
        a0 = float(a[0, sel].real.sum())
        if a0 == 0.0:
            continue
        err = np.hypot(a[:, sel].real.sum(axis=1) - re[:, sel].sum(axis=1).astype(np.float64),
                       a[:, sel].imag.sum(axis=1) - im[:, sel].sum(axis=1).astype(np.float64))
        worst = max(worst, float(err.max()) / a0)
    print(f"n={n}: max |dA_k| / A_0 = {worst:.3e}")
    assert worst <= 1e-13


def test_four_bodies_on_a_square_are_exact():
    pos, vel, mass = MR.square(0.75)
    got = result(pos, vel, mass, MR.SQUARE_CENTRE, (0.0, 0.0), np.array([1.0, 4.0]), 16, True)
    want = np.array([3.0 if k % 4 == 0 else 0.0 for k in range(17)])
    assert np.array_equal(got.coeff[:, 0].real, want) and not got.coeff.imag.any()
    assert np.array_equal(got.amplitude[:, 0], want / 3.0) and list(got.count) == [4] and list(got.mass) == [3.0]
    assert not got.rate_coeff.any() and got.inside == 0.0 and got.beyond == 0.0
    # the integers themselves: plane 0 and the cosine planes of k = 4, 8, 12, 16 hold 4 m in units, every other plane nothing
    unit = int(np.ldexp(3.0, int(got.exponents[0])))
    for p in range(33):
        k, cosine = (p + 1) // 2, p % 2 == 1 or p == 0
        assert got.planes[p, 1] == (unit if (cosine and k % 4 == 0) else 0), p


def test_one_body_at_the_centre():
    pos, vel, mass = np.array([[0.5, 0.25]]), np.array([[1.0, -2.0]]), np.array([2.5])
    planes, e = MR.modes(pos, vel, mass, (0.5, 0.25), (0.0, 0.0), np.array([0.0, 1.0]), 3, True)
    assert list(e) == [62 - 2, 0]                                  # 2.5 < 2^2; no rate at all
    want = np.zeros_like(planes)
    want[0, 1], want[-1, 1] = int(np.ldexp(2.5, 60)), 1
    assert np.array_equal(planes, want)


@pytest.mark.parametrize("n", [257, 5000])
def test_rigid_rotation(n):
    centre, centre_vel = (0.75, -0.5), (0.125, -0.0625)
    pos, vel, mass = MR.rotator(n, centre=centre, centre_vel=centre_vel)
    got = result(pos, vel, mass, centre, centre_vel, EDGES4, 16, True)
    seen = 0
    for k in range(1, 17):
        t = got.total(k)
        if t.amplitude > 0.01:
            seen += 1
            print(f"n={n} k={k}: amplitude {t.amplitude:.4f}, pattern speed - Omega = {t.pattern_speed - MR.OMEGA:.3e}")
            assert abs(t.pattern_speed - MR.OMEGA) <= 1e-12, (k, t)
    assert seen >= 2 and got.total(2).amplitude > 0.3              # (the bar itself)
    assert math.isnan(got.total(0).pattern_speed) and got.total(0).amplitude == 1.0 and got.total(0).phase == 0.0
    mean = got.rate_coeff[0].real / got.mass
    assert np.abs(mean - MR.OMEGA).max() <= 1e-12 and not got.rate_coeff[0].imag.any()
    # per bin too, where the bin has a pattern: a rigid rotator turns at Omega everywhere
    strong = got.amplitude[1:] > 0.01
    assert np.abs(got.pattern_speed[1:][strong] - MR.OMEGA).max() <= 1e-12
    assert np.isnan(got.pattern_speed[0]).all()
    assert np.array_equal(got.amplitude[0], np.ones(4)) and not got.phase[0].any()


def binary_bodies(n, seed=3):
    """Offsets, velocities on a binary grid about a binary-fraction centre: a quarter turn is exact."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-4096, 4097, size=(n, 2)) / 4096.0 * np.array([2.0, 0.5])
    d[0] = [0.0, 0.0]                                              # one body at the centre
    vel = rng.integers(-512, 513, size=(n, 2)) / 256.0
    return np.array(MR.SQUARE_CENTRE) + d, vel, rng.integers(1, 64, n) / 16.0


def test_a_quarter_turn_moves_the_phase_and_permutes_the_planes():
    pos, vel, mass = binary_bodies(257)
    c = MR.SQUARE_CENTRE
    p2, v2 = MR.quarter_turn(pos, vel, c)
    assert np.array_equal(p2 - np.array(c), np.stack([-(pos - np.array(c))[:, 1], (pos - np.array(c))[:, 0]], axis=1))
    M = 6
    a, b = (result(p, v, mass, c, (0.0, 0.0), EDGES4, M, True) for p, v in ((pos, vel), (p2, v2)))
    assert np.array_equal(a.exponents, b.exponents)
    n_a = 1 + 2 * M
    for first in (0, n_a):                                         # (c_k, s_k) -> i^k (c_k + i s_k), and w is unchanged
        assert np.array_equal(b.planes[first], a.planes[first])
        for k in range(1, M + 1):
            ck, sk = a.planes[first + 2 * k - 1], a.planes[first + 2 * k]
            want = [(ck, sk), (-sk, ck), (-ck, -sk), (sk, -ck)][k % 4]
            assert np.array_equal(b.planes[first + 2 * k - 1], want[0]) and np.array_equal(b.planes[first + 2 * k], want[1]), k
    assert np.array_equal(b.planes[-1], a.planes[-1])
    d = b.total(2).phase - a.total(2).phase
    assert abs(math.remainder(d - 0.5 * math.pi, math.pi)) <= 1e-15
    per_bin = np.remainder(b.phase[2] - a.phase[2] - 0.5 * np.pi + 0.5 * np.pi, np.pi) - 0.5 * np.pi
    assert np.abs(per_bin).max() <= 1e-15
    assert np.array_equal(a.pattern_speed[[2, 4]], b.pattern_speed[[2, 4]], equal_nan=True)


def turned(pos, centre, angle):
    c, s = math.cos(angle), math.sin(angle)
    d = pos - np.array(centre)
    return np.array(centre) + np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]], axis=1)


def test_pattern_speed_between():
    centre = (0.75, -0.5)
    pos, vel, mass = MR.rotator(257, centre=centre)
    base = result(pos, None, mass, centre, (0.0, 0.0), EDGES4, 4, False)
    between = G.BhAzimuthalModes.pattern_speed_between
    for angle in (0.3, -0.4, 1.5):                                 # k = 2: below pi / 2, so followed
        other = result(turned(pos, centre, angle), None, mass, centre, (0.0, 0.0), EDGES4, 4, False)
        assert abs(between(base, other, 0.5, 2) - angle / 0.5) <= 1e-12
        assert abs(between(other, base, 0.5, 2) + angle / 0.5) <= 1e-12
    # a difference that wraps: the phase of k = 2 lives in (-pi/2, pi/2]; the bar's long axis lies along x (phase ~ 0), so
    # turning it by +1.2 and by -1.2 gives phases whose plain difference is -2.4: unwrapped, pi - 2.4
    plus, minus = (result(turned(pos, centre, a), None, mass, centre, (0.0, 0.0), EDGES4, 4, False) for a in (1.2, -1.2))
    assert abs((minus.total(2).phase - plus.total(2).phase) + 2.4) <= 1e-12
    assert abs(between(plus, minus, 1.0, 2) - (math.pi - 2.4)) <= 1e-12
    assert abs(between(minus, plus, 2.0, 2) + (math.pi - 2.4) / 2.0) <= 1e-12
    # a range of bins
    assert abs(between(base, plus, 1.0, 2, 0.5, 2.0) - 1.2) <= 1e-12
    with pytest.raises(ValueError):
        between(base, plus, 1.0, 0)
    with pytest.raises(ValueError):
        base.total(5)


def test_total_adds_the_integers_of_the_bins_in_range():
    pos, vel, mass = MR.rotator(257)
    centre = (0.75, -0.5)
    got = result(pos, vel, mass, centre, (0.125, -0.0625), EDGES4, 3, True)
    inner = got.total(2, 0.5, 2.0)                                 # bins 1 and 2
    a, d = MR.values(got.planes[:, 2:4].sum(axis=1, keepdims=True), got.exponents, 3, True)
    assert inner.amplitude == abs(a[2, 0]) / a[0, 0].real and inner.phase == math.atan2(a[2, 0].imag, a[2, 0].real) / 2
    assert inner.pattern_speed == (d[2, 0].real * a[2, 0].real + d[2, 0].imag * a[2, 0].imag) / (a[2, 0].real ** 2 + a[2, 0].imag ** 2)
    assert abs(inner.pattern_speed - MR.OMEGA) <= 1e-12
    none = got.total(2, 3.0, 4.0)                                  # no bin lies in the range
    assert math.isnan(none.amplitude) and math.isnan(none.pattern_speed)
    plain = result(pos, vel, mass, centre, (0.0, 0.0), EDGES4, 3, False, raw=False)
    assert plain.planes is None and plain.exponents is None and plain.rate_coeff is None and plain.pattern_speed is None
    assert math.isnan(plain.total(2).pattern_speed) and plain.total(2).amplitude == got.total(2).amplitude


def test_the_conversion_is_the_twins():
    pos, vel, mass = MR.fixture(300, 8)
    edges = MR.fixture_edges(8)
    planes, e = MR.modes(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, 4, True)
    got = G.azimuthal_modes_from_planes(planes, e, edges, 4, True, MR.CENTRE, MR.CENTRE_VEL)
    for k, w in MR.convert(planes, e, 4, True).items():
        assert np.array_equal(getattr(got, k), w, equal_nan=True), k
    assert np.array_equal(G.modes_exponents(MR.maxima(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, 4, True), 300), e)
    with pytest.raises(ValueError):
        G.azimuthal_modes_from_planes(planes[:-1], e, edges, 4, True, MR.CENTRE)


@pytest.mark.parametrize("rates", [False, True])
def test_order_and_splitting(rates):
    n = 300
    pos, vel, mass = MR.fixture(n, 8)
    edges = MR.fixture_edges(8)
    planes, e = MR.modes(pos, vel, mass, MR.CENTRE, MR.CENTRE_VEL, edges, 7, rates)
    perm = np.random.default_rng(2).permutation(n)
    p2, e2 = MR.modes(pos[perm], vel[perm], mass[perm], MR.CENTRE, MR.CENTRE_VEL, edges, 7, rates)
    assert np.array_equal(planes, p2) and np.array_equal(e, e2)
    # two "ranks": MAX of the maxima, SUM of the counts, the whole system's exponents, integer sum of the planes
    halves = [np.arange(n) < 113, np.arange(n) >= 113]
    mx = np.max([MR.maxima(pos[h], vel[h], mass[h], MR.CENTRE, MR.CENTRE_VEL, 7, rates) for h in halves], axis=0)
    assert np.array_equal(G.modes_exponents(mx, n), e)
    parts = [MR.deposit(pos[h], vel[h], mass[h], MR.CENTRE, MR.CENTRE_VEL, edges, 7, rates, e) for h in halves]
    assert np.array_equal(parts[0] + parts[1], planes)


def test_what_the_first_pass_refuses():
    pos, vel, mass = MR.fixture(65, 8)
    args = (MR.CENTRE, MR.CENTRE_VEL, 4)
    bad_v = vel.copy()
    bad_v[7, 1] = np.nan
    MR.maxima(pos, bad_v, mass, *args, False)                      # without rates the velocities are not read
    with pytest.raises(ValueError):
        MR.maxima(pos, bad_v, mass, *args, True)
    far = pos.copy()
    far[5, 0] = 1e200
    for rates in (False, True):
        with pytest.raises(ValueError):
            MR.maxima(far, vel, mass, *args, rates)
    close = pos.copy()
    close[9] = [MR.CENTRE[0] + 1e-150, MR.CENTRE[1]]               # r2 = 1e-300 is normal, b = 1e10 is finite:
    fast = vel.copy()
    fast[9] = [0.0, 1e160]                                         # w = b / r2 = 1e310 overflows
    MR.maxima(close, fast, mass, *args, False)
    MR.maxima(close, vel, mass, *args, True)
    with pytest.raises(ValueError):
        MR.maxima(close, fast, mass, *args, True)
    neg = mass.copy()
    neg[3] = -2.0
    MR.maxima(pos, vel, neg, *args, True)                          # a negative mass is allowed


def test_the_lds_selector():
    assert MR.n_planes(0, False) == 2 and MR.n_planes(2, False) == 6 and MR.n_planes(2, True) == 11 and MR.n_planes(16, True) == 67
    assert G.modes_planes(16, True) == 67 and G.modes_planes(4, False) == 10
    for M, rates in [(0, False), (2, False), (2, True), (4, True), (16, False), (16, True)]:
        P = MR.n_planes(M, rates)
        nb = MR.largest_private_nb(P)
        if nb <= MR.MAX_BINS:
            tile, size = MR.plan(P, nb)
            assert tile == 0 and size == 8 * P * (nb + 2) + 8 * (nb + 1) <= 65536
        if nb + 1 <= MR.MAX_BINS:
            tile, size = MR.plan(P, nb + 1)
            assert tile == 65536 // (8 * P) and size == 8 * P * tile <= 65536 and tile >= 1
            assert 8 * P * (nb + 3) + 8 * (nb + 2) > 65536
    assert MR.largest_private_nb(6) == 1168 and MR.largest_private_nb(67) == 118
    assert MR.plan(6, 1169) == (1365, 65520) and MR.plan(67, 119) == (122, 65392) and MR.plan(2, 4096) == (4096, 65536)


def test_the_host_selector_is_the_twins(tmp_path):
    """csrc/bh_query_host.hpp's modes_plan, compiled on its own, against modes_ref.plan around every boundary."""
    exe = tmp_path / "modes_plan_replay"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "modes_plan_replay.cpp")])
    rows = [[int(t) for t in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) > 17 * 2 * 5
    paths = set()
    for M, rates, nb, P, tile, size in rows:
        assert P == MR.n_planes(M, bool(rates)) and (tile, size) == MR.plan(P, nb), (M, rates, nb)
        paths.add(tile == 0)
    assert paths == {True, False}
