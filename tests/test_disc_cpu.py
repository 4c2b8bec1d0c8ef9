"""The disc without a GPU: the twin's sampler and deviates (tests/disc_ref.py) have the distributions they claim, and the host
recipes of engine.py -- rotation_curve_from_planes, toomre_q_from, resonances_from, disc_velocity_table_from -- give the
analytic numbers of a Kuzmin-Toomre disc back from planes made of them."""
import math

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
import disc_ref as D

SEED, N, A, RMAX = 1, 4099, 0.02, 0.2


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_max", [RMAX, 0.02, 0.006, math.inf])
def test_every_radius_is_inside_the_truncation(r_max):
    R = D.disc_radii(N, SEED, A, r_max)
    assert np.isfinite(R).all() and (R >= 0.0).all()
    if math.isfinite(r_max):
        assert (R <= r_max * (1.0 + 2.0 ** -50)).all(), R.max() / r_max - 1.0


def test_the_direction_loop_rejects_and_never_exhausts():
    c, z, tries = D.disc_directions(N, SEED)
    print("most tries", tries.max())
    assert tries.max() >= 3 and tries.max() < D.DIR_TRIES and tries.min() == 1
    assert np.abs(c * c + z * z - 1.0).max() <= 4.0 * np.finfo(np.float64).eps
    # both half planes and both signs are taken
    assert (c > 0).any() and (c < 0).any() and (z > 0).any() and (z < 0).any()


def test_the_mass_inside_the_scale_length_is_the_kuzmin_fraction():
    R = D.disc_radii(N, SEED, A, RMAX)
    want = D.kuzmin_fraction_inside(A, A, RMAX)
    assert want == pytest.approx((1.0 - 1.0 / math.sqrt(2.0)) / D.truncation_factor(A, RMAX), rel=1e-15)
    got = (R <= A).mean()
    sigmas = (got - want) / math.sqrt(want * (1.0 - want) / N)
    print("fraction inside a:", got, "expected", want, "sigmas", sigmas)
    assert abs(sigmas) <= 4.0


def test_disc_is_a_function_of_seed_and_index():
    m, pos, vel, _ = D.disc(257, 7, 3.0, A, RMAX)
    m2, pos2, _, _ = D.disc(100, 7, 3.0, A, RMAX)
    assert np.array_equal(pos[:100], pos2) and m[0] == 3.0 / 257 and m2[0] == 3.0 / 100 and not vel.any()
    assert not np.array_equal(pos, D.disc(257, 8, 3.0, A, RMAX)[1])
    assert D.disc(0, 1, 1.0, A, RMAX)[1].shape == (0, 2)


# ---- the deviates ------------------------------------------------------------------------------------------------------------
def test_the_deviates_are_standard_bounded_and_uncorrelated():
    n = 65536
    g1, g2 = D.deviates(np.arange(n), SEED)
    lim = 4.0 / math.sqrt(n)
    for g in (g1, g2):
        print("mean", g.mean(), "variance", g.var())
        assert abs(g.mean()) < lim and abs(g.var() - 1.0) < 0.02 and np.abs(g).max() <= 6.0
        assert np.array_equal(g * 4294967296.0, np.rint(g * 4294967296.0))        # exact multiples of 2^-32
    corr = float(np.corrcoef(g1, g2)[0, 1])
    print("correlation", corr)
    assert abs(corr) < lim
    assert not np.array_equal(g1, D.deviates(np.arange(n), SEED + 1)[0])


# ---- the host recipes on analytic Kuzmin tables --------------------------------------------------------------------------------
GM, MASS, SCALE, NB = 1.0, 1.0, 1.0, 64
EDGES = np.geomspace(0.1, 10.0, NB + 1)
H = math.log(100.0) / NB                     # the spacing of ln radius: the bin radii below are the geometric means of the edges


def kuzmin_planes(empty=()):
    """int64 planes (5, nb + 2) and exponents of a Kuzmin disc binned at the geometric mean of every bin's edges."""
    R = np.sqrt(EDGES[:-1] * EDGES[1:])
    mass = D.kuzmin_sigma(R, MASS, SCALE) * np.pi * (EDGES[1:] ** 2 - EDGES[:-1] ** 2)
    mass[list(empty)] = 0.0
    q = np.zeros((4, NB + 2))
    q[0, 1:-1], q[1, 1:-1], q[2, 1:-1] = mass, mass * R, -mass * D.kuzmin_vc2(R, GM, SCALE)
    q[3, 1:-1] = mass * 1e-3 * np.sin(np.arange(NB))
    q[0, 0], q[0, -1] = 0.25, 0.125
    ex = G.radial_exponents(np.abs(q).max(axis=1), 1 << 20)
    planes = np.zeros((5, NB + 2), dtype=np.int64)
    for p in range(4):
        planes[p] = np.rint(np.ldexp(q[p], int(ex[p])))
    planes[4, 1:-1] = np.where(mass > 0, 100, 0)
    planes[4, 0], planes[4, -1] = 3, 2
    return planes, ex, R, mass


def test_curve_from_planes_gives_the_kuzmin_frequencies():
    planes, ex, R, mass = kuzmin_planes()
    c = G.rotation_curve_from_planes(planes, ex, EDGES, (0.5, -0.25), raw=True)
    fixed = 2.0 ** -38                       # a plane's rounding: half a unit of 2^-e against a maximum of 2^(62 - 20 - e) at least
    assert np.allclose(c.mass, mass, rtol=0, atol=fixed * mass.max()) and np.array_equal(c.count, np.full(NB, 100))
    assert np.allclose(c.radius, R, rtol=1e-9) and np.allclose(c.vc2, D.kuzmin_vc2(R, GM, SCALE), rtol=1e-8)
    assert np.allclose(c.vc, np.sqrt(c.vc2)) and np.allclose(c.omega, c.vc / c.radius)
    assert (c.mass_inside, c.mass_outside, c.count_inside, c.count_outside) == (0.25, 0.125, 3, 2)
    assert c.centre == (0.5, -0.25)
    assert np.array_equal(c.planes, planes) and np.array_equal(c.exponents, ex)
    assert c.torque_cumulative.shape == (NB + 1,) and c.torque_cumulative[0] == 0.0
    assert np.allclose(np.diff(c.torque_cumulative), c.torque, rtol=0, atol=1e-12)
    # kappa^2 / omega^2 = (R^2 + 4 a^2) / (R^2 + a^2).  f = ln omega^2 over x = ln R has f' = -3 s, s = R^2 / (R^2 + a^2),
    # f'' = -6 s (1 - s), f''' = -12 s (1 - s)(1 - 2 s): |f''| <= 3/2, |f'''| <= 2 / sqrt(3).  np.gradient's central difference
    # errs by h^2 / 6 |f'''| at most inside and its one-sided difference by h / 2 |f''| at the two ends.
    ratio = (c.kappa / c.omega) ** 2
    want = (R * R + 4.0 * SCALE ** 2) / (R * R + SCALE ** 2)
    err = np.abs(ratio - want)
    print("kappa^2 / omega^2: worst inside", err[1:-1].max(), "at the ends", err[0], err[-1])
    assert err[1:-1].max() <= H * H / 6.0 * 2.0 / math.sqrt(3.0) + 1e-7
    assert max(err[0], err[-1]) <= H / 2.0 * 1.5 + 1e-7


def test_empty_and_outward_bins_have_no_kappa():
    planes, ex, R, _ = kuzmin_planes(empty=(5, 6))
    planes[2, 11] = -planes[2, 11]           # the force points outwards in bin 10: vc2 < 0
    c = G.rotation_curve_from_planes(planes, ex, EDGES, (0.0, 0.0))
    assert np.isnan(c.kappa[[5, 6, 10]]).all() and np.isnan(c.radius[[5, 6]]).all() and c.vc2[10] < 0 and c.vc[10] == 0.0
    rest = np.ones(NB, bool)
    rest[[5, 6, 10]] = False
    assert np.isfinite(c.kappa[rest]).all() and c.planes is None
    lone = np.zeros_like(planes)
    lone[:, 3] = planes[:, 3]
    assert np.isnan(G.rotation_curve_from_planes(lone, ex, EDGES, (0.0, 0.0)).kappa).all()
    with pytest.raises(ValueError):
        G.rotation_curve_from_planes(planes[:, :-1], ex, EDGES, (0.0, 0.0))


def profile_with(mass, sigma_r):
    planes = np.zeros((6, NB + 2), dtype=np.int64)
    q = [mass, 0 * mass, 0 * mass, mass * sigma_r ** 2, 0 * mass]
    ex = G.radial_exponents([np.abs(v).max() for v in q], 1 << 20)
    for p in range(5):
        planes[p, 1:-1] = np.rint(np.ldexp(q[p], int(ex[p])))
    planes[5, 1:-1] = np.where(mass > 0, 100, 0)
    return G.radial_profile_from_planes(planes, ex, EDGES, (0.0, 0.0))


def test_toomre_q_and_the_velocity_table_agree():
    planes, ex, R, mass = kuzmin_planes(empty=(0,))
    c = G.rotation_curve_from_planes(planes, ex, EDGES, (0.0, 0.0))
    radii, vt, sr, st = G.disc_velocity_table_from(c, profile_with(mass, np.full(NB, 0.1)), GM, 1.5)
    assert len(radii) == NB - 1 and np.array_equal(radii, c.radius[1:])
    assert (sr > 0).all() and (st > 0).all() and (vt >= 0).all()
    # the table's dispersion, fed back as the measured one, gives the Q it was made for
    s = np.zeros(NB)
    s[1:] = sr
    q = G.toomre_q_from(c, profile_with(mass, s), GM)
    assert np.isnan(q[0]) and np.allclose(q[1:], 1.5, rtol=1e-6), q
    # the epicyclic ratio, and the asymmetric drift of a disc whose Sigma sigma_r^2 falls outwards: vt below vc
    omega, kappa = c.omega[1:], G.epicyclic_from(c.radius[1:], c.omega[1:])
    assert np.allclose(st / sr, kappa / (2.0 * omega), rtol=1e-12)
    assert (vt[8:] < c.vc[1:][8:]).all()
    # a colder disc drifts less
    vt_cold = G.disc_velocity_table_from(c, profile_with(mass, s), GM, 0.5)[1]
    assert (np.abs(c.vc[1:] - vt_cold) <= np.abs(c.vc[1:] - vt) + 1e-15).all()
    with pytest.raises(ValueError):
        G.disc_velocity_table_from(c, profile_with(mass, s), GM, 1.5, min_count=101)
    with pytest.raises(ValueError):
        other = G.radial_profile_from_planes(np.zeros((6, 3), dtype=np.int64), np.zeros(5, dtype=np.int32), [0.0, 1.0], (0.0, 0.0))
        G.toomre_q_from(c, other, GM)


def test_resonances_are_found_where_they_were_planted():
    planes, ex, R, _ = kuzmin_planes()
    c = G.rotation_curve_from_planes(planes, ex, EDGES, (0.0, 0.0))
    # on a bin: exactly its radius
    res = G.resonances_from(c, c.omega[20])
    assert np.array_equal(res.corotation, [c.radius[20]])
    # between two bins: inside the bracket, and as close as a chord of omega allows.  Over one spacing dR = H R the chord
    # errs by dR^2 / 8 |omega''|, which moves the crossing by that over |omega'|; |omega'' / omega'| <= 4 / R on this curve.
    Rc = math.sqrt(R[30] * R[31])
    p = math.sqrt(D.kuzmin_vc2(Rc, GM, SCALE)) / Rc
    res = G.resonances_from(c, p)
    assert len(res.corotation) == 1 and R[30] < res.corotation[0] < R[31]
    assert abs(res.corotation[0] - Rc) <= (H * Rc) ** 2 / 8.0 * 4.0 / Rc + 1e-6 * Rc
    # omega + kappa / 2 falls outwards: one outer Lindblad resonance beyond corotation; omega - kappa / 2 of this disc peaks
    # inside, so a slow pattern has two inner ones or none
    assert len(res.outer) == 1 and res.outer[0] > res.corotation[0]
    assert len(res.inner) in (0, 2) and all(r < res.corotation[0] for r in res.inner)
    planted = c.omega[40] + c.kappa[40] / 2.0
    assert np.array_equal(G.resonances_from(c, planted).outer, [c.radius[40]])
    assert G.resonances_from(c, planted, m=4).outer[0] != c.radius[40]
    assert len(G.resonances_from(c, 1e6).corotation) == 0
