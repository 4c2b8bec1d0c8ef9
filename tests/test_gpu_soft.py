"""Plummer softening on the device (bh_set_softening): the two-body law, the unchanged term set, values against the
softened numpy walks (tests/soft_ref.py), agreement of the kernel variants, eps = 0 being the unsoftened engine bit for
bit, a trajectory twin, the force error, the distributed (LET) step, errors and state.

Tolerances: 1e-12 relative in BH_PRECISION_F64 (F64_TOL of tests/test_gpu_energy.py, TOL of tests/test_gpu_f64.py); in F32 /
MIXED the forward model of tests/test_gpu_field.py, 2^-24 ((1.5 sqrt(count) + 8) sum |a_j| + 4 coord), and F32_TOL_ALL of
tests/test_gpu_energy.py for the potential -- every softened term is no larger than its unsoftened one, so the unsoftened
bounds hold.  The two-body law: 4 * 2^-23 relative in F32 / MIXED."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import _lib, initial_conditions as IC  # noqa: E402
from gpu_nbody_simulation_amd.distributed import partition_orb  # noqa: E402
from gpu_nbody_simulation_amd.engine import (FLAG_LDS_STACK, FLAG_WALK_NO_SPLIT, FLAG_WALK_PORTABLE,  # noqa: E402
                                             FLAG_WALK_STATS)
from direct_ref import same_bits  # noqa: E402
import field_ref as FR  # noqa: E402
import soft_ref as SR  # noqa: E402
import quiet_case as QC  # noqa: E402
from let_ranks import EmulatedRanks  # noqa: E402

P = G.Precision
SOFT_PRECISIONS = [P.F32, P.MIXED, P.F64]
GC = 6.67e-11
F64_TOL = 1e-12
F32_LAW_TOL = 4.0 * 2.0 ** -23
F32_TOL_ALL = 5e-4                # tests/test_gpu_energy.py
FOREST_TOL = 2e-7                 # tests/test_gpu_let_energy.py
# The LET forces' criterion: tests/test_gpu_let_parity.py's, unsoftened, for its "plummer-orb4" case (median, 99.9 %, max of
# the relative error of the bodies whose term counts are the reference's).  Two things to know about it.  What it is applied
# to: that file compares the forest walk with a FOREST reference (each rank's tree under the global box, walked whole), and
# so does the test here, with the softened one -- the same terms, so the difference is fp32 rounding, which is what these
# figures bound.  One context holding the union walks one tree, other cells and other terms: it differs from the forest by the
# Barnes-Hut error (1e-3 .. 1e-2 at theta 0.5), no rounding criterion can hold between the two, and that comparison is
# bounded only as two Barnes-Hut sums of one law are (median < 1e-2, below).  Where it comes from: a 65,536-body, 4-rank
# case, where it is <= 2 x the measured error; the state here is the same Plummer model with 4,096 bodies on 2 ranks, whose
# walks are shorter (fewer terms per body, so no more rounding), and every softened term is no larger than its unsoftened
# one: the borrowed figures are a bound for this shape too, and were not taken from what this test measures.
FOREST_FORCE_TOL = (3.3e-7, 3.6e-5, 2.7e-4)
ERR_ARG, ERR_STATE = -1, -5
EPS = 1e-3                        # init1024 spans 0.2, the Plummer samples have the scale radius 0.02


def engine(n, **kw):
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), **kw))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def rel(a, ref):
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)


def clumped(n):
    rng = np.random.default_rng(5)
    p = f32(np.concatenate([rng.normal(0, 1e-3, (n // 2, 2)), rng.uniform(-1, 1, (n - n // 2, 2))]))
    return f32(rng.uniform(0.1, 0.5, n)), p, f32(rng.uniform(-1e-9, 1e-9, (n, 2)))


def make(kind, n, seed=3):
    return clumped(n) if kind == "clumped" else IC.make(kind, n, seed, quasi_static=True)


# ---- 1. the two-body law -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", SOFT_PRECISIONS)
@pytest.mark.parametrize("ratio", [10.0, 1.0, 0.01])
def test_two_body_law(prec, ratio):
    """Masses 0.3 and 0.5 at separation r = ratio * eps: |F| = G m1 m2 r / (r^2 + eps^2)^(3/2), phi_i = -G m_j / sqrt(r^2 + eps^2).
    The closed form is taken at the values the walk holds (fp32-rounded in F32 / MIXED, whose second body stands at an fp32
    number r from the first at the origin, so dx is exact).  Measured maxima on MI355X: DESIGN.md section 16."""
    eps = 2.0 ** -6
    r = ratio * eps
    m = np.array([0.3, 0.5])
    p = np.array([[0.0, 0.0], [r, 0.0]])
    with engine(2, precision=prec, max_depth=32, reference_compat=False, softening=eps) as e:
        e.upload(p, np.zeros((2, 2)), m)
        assert e.softening == eps
        e.compute_forces()
        fw = e.forces() if prec == P.F64 else e.accelerations()
        phi = e.potential()
        fd = e.direct_forces()
    mw, rw = (m, r) if prec == P.F64 else (f32(m), float(f32(r)))
    s2 = rw * rw + eps * eps
    tol = F64_TOL if prec == P.F64 else F32_LAW_TOL
    # F64 returns the force; F32 / MIXED the acceleration, the force over the body's own mass: the same relative error
    mag = GC * rw / s2 ** 1.5 * (np.array([mw[0] * mw[1]] * 2) if prec == P.F64 else mw[::-1])
    err_f = max(abs(fw[0, 0] - mag[0]) / mag[0], abs(fw[1, 0] + mag[1]) / mag[1])
    phi_ref = -GC * mw[::-1] / np.sqrt(s2)
    err_p = np.max(np.abs(phi - phi_ref) / np.abs(phi_ref))
    print(f"two-body {prec.name} r/eps {ratio}: force rel err {err_f:.3e}, potential rel err {err_p:.3e} (tol {tol:.3e})")
    assert fw[0, 1] == 0.0 and fw[1, 1] == 0.0
    assert err_f <= tol and err_p <= tol
    # the direct sum: fp64 on the state the device holds (fp32-rounded in F32 only), a dozen roundings
    md, rd = (f32(m), float(f32(r))) if prec == P.F32 else (m, r)
    magd = GC * md[0] * md[1] * rd / (rd * rd + eps * eps) ** 1.5
    assert max(abs(fd[0, 0] - magd), abs(fd[1, 0] + magd)) <= 16 * 2.0 ** -53 * magd and fd[0, 1] == 0.0 and fd[1, 1] == 0.0


# ---- 2. the term set does not depend on eps ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plummer4096():
    return IC.make("plummer", 4096, 2)


@pytest.mark.parametrize("prec", SOFT_PRECISIONS)
@pytest.mark.parametrize("compat,md", [(True, 10), (False, 21), (False, 14), (False, 4)])
@pytest.mark.parametrize("name", ["init1024", "plummer4096"])
def test_term_set_is_unchanged(init1024, plummer4096, name, compat, md, prec):
    """Per-body interaction counts of the force walk and term counts of the potential and the field, eps > 0 against eps = 0
    on the same state.  max_depth 14 is the sibling's bucket case (test_bucket_mode_matches_uncapped_oracle); 4 makes
    multi-body depth-cap cells of either input for sure (checked on the oracle's trees)."""
    m, p, v = init1024 if name == "init1024" else plummer4096
    if md == 4:
        assert len(O.build_tree(p, m, 4)) < len(O.build_tree(p, m, 0))
    n = len(m)
    pts = FR.points_around(p, 1024, 3)
    got = []
    with engine(n, precision=prec, reference_compat=compat, max_depth=md, flags=FLAG_WALK_STATS) as e:
        e.upload(p, v, m)
        for eps in (0.0, EPS, 0.0, 30 * EPS):
            e.set_softening(eps)
            e.compute_forces()
            fc = e.interaction_counts().copy()
            phi, pc = e.potential(with_counts=True)
            acc, fphi, cc = e.field(pts, with_counts=True)
            got.append((fc, pc, cc, e.accelerations() if prec != P.F64 else e.forces(), phi, acc, fphi))
    base = got[0]
    assert np.array_equal(base[0], base[1]) and base[0].sum() > 0
    for g in got[1:]:
        for k in range(3):
            assert np.array_equal(g[k], base[k]), k
    # eps = 0 again is eps = 0; eps > 0 is something else.  (same_bits: an fp64 body that coincides with an aggregate it
    # takes has the reference's NaN force without softening, and NaN equals NaN here)
    for k in range(3, 7):
        assert same_bits(got[2][k], base[k]), k
        assert not same_bits(got[1][k], base[k]), k
    # softening only weakens: |phi| term by term, so body by body
    fin = np.isfinite(base[4])
    assert (np.abs(got[1][4]) <= np.abs(base[4]))[fin].all() and (np.abs(got[3][4]) <= np.abs(got[1][4]))[fin].all()


# ---- 3. values against the softened reference walks --------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref1024(init1024):
    """Softened references of init1024 (eps = EPS, theta 0.5), computed once: fp64 inputs for F64 (compat on, cap 10) and
    fp32-rounded inputs for F32 / MIXED (compat on cap 10; compat off cap 4: bucket leaves)."""
    m, p, v = init1024
    pts = FR.points_around(p, 1024, 3)
    out = {"pts": pts}
    n = len(m)
    t = O.build_tree(p, m, 10)
    out["f64"] = (SR.soft_field_walk(t, p, eps=EPS, self_of=np.arange(n), compat=True),
                  SR.soft_potential_walk(t, p, compat=True, eps=EPS), SR.soft_field_walk(t, pts, eps=EPS))
    pr, mr = f32(p), f32(m)
    ptr = f32(pts)
    for key, (tree, compat, cap) in {"f32-compat": (O.build_tree(pr, mr, 10), True, 0),
                                     "f32-bucket": (O.build_tree(pr, mr, 0), False, 4)}.items():
        out[key] = (SR.soft_field_walk(tree, pr, eps=EPS, self_of=np.arange(n), compat=compat, cap_depth=cap),
                    SR.coord_scale(tree, pr, self_of=np.arange(n), compat=compat) if cap == 0 else None,
                    SR.soft_field_walk(tree, ptr, eps=EPS, cap_depth=cap),
                    SR.coord_scale(tree, ptr) if cap == 0 else None)
    return out


def test_fp64_values_against_the_softened_reference(init1024, ref1024):
    m, p, v = init1024
    body, (phi_ref, phi_cnt), at = ref1024["f64"]
    with engine(1024, precision=P.F64, flags=FLAG_WALK_STATS, softening=EPS) as e:
        e.upload(p, v, m)
        f = e.compute_forces()
        fc = e.interaction_counts()
        phi, pc = e.potential(with_counts=True)
        acc, fphi, cc = e.field(ref1024["pts"], with_counts=True)
    assert np.array_equal(fc, body.counts) and np.array_equal(pc, phi_cnt) and np.array_equal(cc, at.counts)
    ef = rel(f, body.accel * m[:, None]).max()
    ep = np.max(np.abs(phi - phi_ref) / np.abs(phi_ref))
    ea = rel(acc, at.accel).max()
    eq = np.max(np.abs(fphi - at.phi) / np.abs(at.phi))
    print(f"F64 softened: forces {ef:.3e} potential {ep:.3e} field accel {ea:.3e} field phi {eq:.3e}")
    assert ef <= F64_TOL and ep <= F64_TOL and ea <= F64_TOL and eq <= F64_TOL


def fp32_model(r, coord):
    return 2.0 ** -24 * ((1.5 * np.sqrt(r.counts) + 8.0) * r.abs_sum + 4.0 * coord)


@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
@pytest.mark.parametrize("case", ["f32-compat", "f32-bucket"])
def test_fp32_values_against_the_softened_reference(init1024, ref1024, prec, case):
    """Accelerations, potential and field() on the bodies / points whose term count is the reference's (an fp32 acceptance
    that turned gives another sum).  The bucket case has no coord scale of its own (the reference walk there is the uncapped
    tree's): it takes the compat case's form with the unsoftened sums of the same walk, a superset of what it needs."""
    m, p, v = init1024
    body, coord_b, at, coord_p = ref1024[case]
    compat, md = (True, 10) if case == "f32-compat" else (False, 4)
    with engine(1024, precision=prec, reference_compat=compat, max_depth=md, flags=FLAG_WALK_STATS, softening=EPS) as e:
        e.upload(f32(p), f32(v), f32(m))
        e.compute_forces()
        a = e.accelerations()
        fc = e.interaction_counts()
        phi, pc = e.potential(with_counts=True)
        acc, fphi, cc = e.field(f32(ref1024["pts"]), with_counts=True)
    assert np.array_equal(pc, fc)
    if coord_b is None:                                       # bucket case: the unsoftened walk's scales bound the softened one
        tree = O.build_tree(f32(p), f32(m), 0)
        d = O.compute_forces_diag(tree, f32(p), f32(m), compat_self_skip=False, pos_rounded=True, cap_depth=md)
        coord_b = d.coord / f32(m)
        dp = FR.oracle_at_points(tree, f32(p), f32(m), f32(ref1024["pts"]), compat=False, pos_rounded=True, cap_depth=md)
        coord_p = dp.coord
    same_b, same_p = fc == body.counts, cc == at.counts
    assert same_b.mean() >= 0.99 and same_p.mean() >= 0.99, (same_b.mean(), same_p.mean())
    eb = np.linalg.norm(a - body.accel, axis=1) / fp32_model(body, coord_b)
    ept = np.linalg.norm(acc - at.accel, axis=1) / fp32_model(at, coord_p)
    eph = np.abs(phi - body.phi) / np.abs(body.phi)
    eqh = np.abs(fphi - at.phi) / np.abs(at.phi)
    print(f"{prec.name} {case}: accel err/model {eb[same_b].max():.3f}, field err/model {ept[same_p].max():.3f}, "
          f"potential rel {eph[same_b].max():.3e}, field phi rel {eqh[same_p].max():.3e}")
    assert eb[same_b].max() <= 1.0 and ept[same_p].max() <= 1.0
    assert eph[same_b].max() <= F32_TOL_ALL and eqh[same_p].max() <= F32_TOL_ALL


# ---- 4. the variants agree ---------------------------------------------------------------------------------------------
def run_variant(m, p, v, n, steps=3, **kw):
    with engine(n, softening=EPS, **kw) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a = e.forces() if kw.get("precision") == P.F64 else e.accelerations()
        e.step(steps)
        return (a,) + e.download()


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("kind,n,md,compat", [("uniform", 20001, 16, False), ("clumped", 30000, 8, False),
                                              ("clumped", 30000, 8, True), ("uniform", 1000, 16, False),
                                              ("uniform", 65, 16, False)])
def test_softened_asm_walk_equals_the_softened_portable_walk(kind, n, md, compat):
    m, p, v = make(kind, n)
    res = [run_variant(m, p, v, n, precision=P.F32, max_depth=md, reference_compat=compat, flags=fl)
           for fl in (FLAG_WALK_NO_SPLIT, FLAG_WALK_NO_SPLIT | FLAG_WALK_PORTABLE)]
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0
    assert same(res[0], res[1])
    with engine(n, precision=P.F32, max_depth=md, reference_compat=compat, flags=FLAG_WALK_NO_SPLIT) as e:   # (and it IS softened)
        e.upload(p, v, m)
        e.compute_forces()
        assert not np.array_equal(e.accelerations(), res[0][0])


@pytest.mark.parametrize("kind,n,md,compat", [("uniform", 130, 4, False), ("plummer", 20000, 21, False),
                                              ("clumped", 30000, 8, False), ("clumped", 30000, 8, True),
                                              ("uniform", 1000, 16, False), ("uniform", 65, 16, False)])
def test_softened_asm_list_walk_equals_the_softened_portable_level_walk(kind, n, md, compat):
    m, p, v = make(kind, n)
    res = [run_variant(m, p, v, n, precision=P.F32, max_depth=md, reference_compat=compat, flags=fl)
           for fl in (0, FLAG_WALK_PORTABLE)]
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0
    assert same(res[0], res[1])


def test_softened_lds_and_register_stacks_agree_bitwise(gold):
    g = gold("ref_project_40960")
    m, p, v = f32(g["mass"]), f32(g["pos"]), f32(g["vel"])
    res = [run_variant(m, p, v, 40960, precision=P.F32, max_depth=16, flags=fl) for fl in (FLAG_WALK_NO_SPLIT, FLAG_LDS_STACK)]
    assert same(res[0], res[1])


@pytest.mark.parametrize("name,n,md,compat", [("gold", 40960, 10, True), ("gold", 40960, 32, False), ("uniform", 1000, 10, True),
                                              ("uniform", 65, 32, False)])
def test_softened_fp64_asm_loop_equals_the_cpp_loop(gold, name, n, md, compat):
    """walk64_asm against its C++ statement (BH_FLAG_WALK_PORTABLE; the counting variant is the C++ loop too), one and two
    stack tiers, reference_compat on and off, a ragged and a single partly filled wavefront."""
    if name == "gold":
        g = gold("ref_project_40960")
        m, p, v = g["mass"], g["pos"], g["vel"]
    else:
        m, p, v = IC.make(name, n, 5, quasi_static=True)
    res = [run_variant(m, p, v, n, precision=P.F64, max_depth=md, reference_compat=compat, flags=fl)
           for fl in (0, FLAG_WALK_PORTABLE, FLAG_WALK_STATS)]
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 0
    assert same(res[0], res[1]) and same(res[0], res[2])


@pytest.mark.parametrize("split", [4, 8])
@pytest.mark.parametrize("kind,n,md", [("plummer", 65536, 21), ("clumped", 30000, 8)])
def test_softened_split_walk_equals_the_softened_one_wave_walk(monkeypatch, split, kind, n, md):
    """The criterion of test_split_walk_equals_the_one_wave_walk: the same node set, accelerations equal to fp32 summation order."""
    m, p, v = clumped(n) if kind == "clumped" else tuple(f32(x) for x in IC.make(kind, n, 3))
    res = []
    for sp, flags in ((1, FLAG_WALK_NO_SPLIT), (split, 0)):
        monkeypatch.setenv("BH_WALK_SPLIT", str(sp))
        with engine(n, precision=P.F32, max_depth=md, reference_compat=False, flags=flags | FLAG_WALK_STATS, softening=EPS) as e:
            e.upload(p, v, m)
            e.compute_forces()
            res.append((e.accelerations(), e.stats(), e.interaction_counts().copy()))
    (a1, s1, c1), (a2, s2, c2) = res
    assert (s1.interactions, s1.visits) == (s2.interactions, s2.visits) and np.array_equal(c1, c2)
    r = rel(a2, a1)
    assert np.median(r) < 5e-7 and r.max() < 1e-4
    assert not np.array_equal(a1, a2)                         # the split really ran


# ---- 5. eps = 0 is the engine as it was --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", SOFT_PRECISIONS)
def test_eps_zero_is_bit_for_bit_the_unsoftened_engine(init1024, prec):
    m, p, v = init1024
    out = []
    for calls in ((), (0.0,), (0.1, 0.0)):
        with engine(1024, precision=prec) as e:
            e.upload(p, v, m)
            for eps in calls:
                e.set_softening(eps)
            assert e.softening == 0.0
            e.step(8)
            out.append(e.download() + (e.forces() if prec == P.F64 else e.accelerations(),))
    assert same(out[0], out[1]) and same(out[0], out[2])
    assert np.isfinite(out[0][2]).all() and np.abs(out[0][2]).max() > 0


# ---- 6. a trajectory twin ----------------------------------------------------------------------------------------------
R0, TWIN_EPS, TWIN_M, TWIN_DT, TWIN_STEPS = 1.0, 0.1, np.array([0.3, 0.5]), 2.5e-3, 6000
# G = 1: the relative acceleration is -0.8 x / (x^2 + eps^2)^(3/2); an unsoftened fall from rest at r0 takes
# (pi / 2) sqrt(r0^3 / (2 G M)) = 1.24, so the bodies pass through each other and come back in about 4 x 1.24 / dt = 2,000 steps


def twin(steps, every):
    """The engine's kick-drift (v += a dt, p += v dt) with the softened pair force; 1 / d carries the walk's 1e-15 offset."""
    x, u = np.array([0.0, R0]), np.zeros(2)
    rows = []
    for k in range(1, steps + 1):
        dx = x[::-1] - x
        s2 = dx * dx + TWIN_EPS * TWIN_EPS
        y = 1.0 / np.sqrt(s2)
        a = TWIN_M[::-1] * (y * y) * (y - 1e-15 * y * y) * dx
        u = u + a * TWIN_DT
        x = x + u * TWIN_DT
        if k % every == 0:
            rows.append(x.copy())
    return np.array(rows)


def test_two_bodies_pass_through_each_other_like_their_numpy_twin():
    """Only leaf terms occur (two bodies), so the twin is exact up to rounding: positions within 1e-9 r0 at every 100th of
    6,000 steps (three oscillations).  The energy with the softened potential stays finite; its excursion is printed
    (DESIGN.md section 16)."""
    ref = twin(TWIN_STEPS, 100)
    p = np.array([[0.0, 0.0], [R0, 0.0]])
    worst, sep, en = 0.0, 0.0, []
    with engine(2, precision=P.F64, G=1.0, dt=TWIN_DT, max_depth=32, reference_compat=False, softening=TWIN_EPS) as e:
        e.upload(p, np.zeros((2, 2)), TWIN_M)
        en.append(e.energy().total)
        for row in ref:
            e.step(100)
            x, _ = e.download()
            worst = max(worst, np.abs(x[:, 0] - row).max())
            sep = max(sep, abs(x[1, 0] - x[0, 0]))
            assert (x[:, 1] == 0.0).all()
            en.append(e.energy().total)
    en = np.array(en)
    signs = np.sign(ref[:, 1] - ref[:, 0])
    print(f"twin: max |x - twin| {worst:.3e} r0, max separation {sep:.6f} r0, passes {int((np.diff(signs) != 0).sum())}, "
          f"energy {en[0]:.6e}, excursion {np.max(np.abs(en - en[0]) / abs(en[0])):.3e}")
    assert (np.diff(signs) != 0).sum() >= 5                    # they went through each other, three oscillations
    assert worst <= 1e-9 * R0
    assert np.isfinite(en).all() and sep <= 1.05 * R0


@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
def test_two_bodies_stay_bound_in_fp32(prec):
    p = np.array([[0.0, 0.0], [R0, 0.0]])
    with engine(2, precision=prec, G=1.0, dt=TWIN_DT, max_depth=21, reference_compat=False, softening=TWIN_EPS) as e:
        e.upload(p, np.zeros((2, 2)), TWIN_M)
        e.step(TWIN_STEPS)
        x, u = e.download()
        en = e.energy()
        e.build_tree()
        root = e.export_tree()[0][0]
    assert np.isfinite(x).all() and np.isfinite(u).all() and np.isfinite(en.total)
    assert abs(x[1, 0] - x[0, 0]) <= 1.05 * R0
    # the root box is the bodies' bounding box padded by a tenth of its extent on each side; the centre of mass (0.625 r0
    # from the first body's start) does not move, and no body is ever further from it than 0.625 x 1.05 r0
    assert root["xmax"] - root["xmin"] <= 1.2 * 1.05 * R0
    assert 0.625 * R0 - 1.05 * R0 <= root["xmin"] and root["xmax"] <= 0.625 * R0 + 1.05 * R0


# ---- 7. the force error ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", SOFT_PRECISIONS)
def test_force_error_with_softening_is_finite_and_no_larger_at_the_maximum(plummer4096, prec):
    m, p, v = plummer4096
    with engine(4096, precision=prec, max_depth=21, reference_compat=False) as e:
        e.upload(p, v, m)
        r0 = e.force_error(sample=4096)
        e.set_softening(EPS)
        r1 = e.force_error(sample=4096)
    print(f"force_error {prec.name}: eps 0 median {r0.median:.3e} p99 {r0.p99:.3e} max {r0.max:.3e} | "
          f"eps {EPS} median {r1.median:.3e} p99 {r1.p99:.3e} max {r1.max:.3e}")
    assert r1.n + r1.n_zero == 4096 and r1.n_nonfinite == 0
    assert all(np.isfinite(x) for x in (r1.median, r1.p90, r1.p99, r1.p999, r1.max, r1.rms))
    assert r1.max <= r0.max


# ---- 8. the distributed (LET) step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [P.F32, P.MIXED])
def test_let_forest_walk_and_potential_take_the_softened_terms(prec):
    """Two ranks on one device, the same eps on both contexts, against the softened forest reference (soft_ref.soft_forest_field:
    every rank's tree under the global box, walked whole) on the bodies whose counts are the reference's; let_potential's
    counts are the forest force walk's."""
    n = 4096
    m, p, v = IC.make("plummer", n, 1, quasi_static=True)
    m, p = f32(m), f32(p)
    parts = partition_orb(p, 2)
    ref = SR.soft_forest_field(m, p, parts, eps=EPS)
    phi_ref, phi_cnt = SR.soft_forest_potential(m, p, parts, eps=EPS)
    assert np.array_equal(phi_cnt, ref.counts)
    er = EmulatedRanks(m, p, v, 2, None, partition=lambda pp, w: parts, theta=0.5, precision=prec, max_depth=21,
                       reference_compat=False, flags=FLAG_WALK_STATS, softening=EPS)
    try:
        er.step(integrate=False)
        a = er.gather(lambda e: e.accelerations())
        fc = er.gather1(lambda e: e.interaction_counts())
        out = [e.let_potential(with_counts=True) for e in er.engs]
        phi = er.gather1(lambda e: out[er.engs.index(e)][0], dtype=np.float64)
        pc = er.gather1(lambda e: out[er.engs.index(e)][1])
        for e in er.engs:
            e.let_counts()
            assert e.softening == EPS
        # the single context's softened forces of the union: the same law through one tree
        with engine(n, precision=prec, max_depth=21, reference_compat=False, softening=EPS) as one:
            one.upload(p, v, m)
            one.compute_forces()
            a_one = one.accelerations()
        er.engs[0].set_softening(0.0)                         # (phi is another law's now)
        dp = (C.c_double * n)()
        assert _lib.load().bh_let_get_potential(er.engs[0]._h, dp, None) == ERR_STATE
    finally:
        er.close()
    assert np.array_equal(pc, fc)
    ok = fc == ref.counts
    r = rel(a, ref.accel)
    print(f"LET softened {prec.name}: {ok.mean():.5f} with the reference's terms; accel median {np.median(r[ok]):.3e} "
          f"q999 {np.quantile(r[ok], 0.999):.3e} max {r[ok].max():.3e}; vs one context median {np.median(rel(a, a_one)):.3e}")
    assert ok.mean() >= 0.99
    assert np.median(r[ok]) <= FOREST_FORCE_TOL[0] and np.quantile(r[ok], 0.999) <= FOREST_FORCE_TOL[1] and r[ok].max() <= FOREST_FORCE_TOL[2]
    ep = np.abs(phi - phi_ref) / np.abs(phi_ref)
    assert ep[ok].max() <= FOREST_TOL
    # one tree or two: the same softened law, different cells -- the Barnes-Hut error, not a rounding error
    # (the median bound of tests/test_gpu_fp32.py::test_bucket_mode_matches_uncapped_oracle for two such sums)
    assert np.median(rel(a, a_one)) < 1e-2 and np.median(rel(a_one, ref.accel)) < 1e-2


# ---- 9. errors and state -----------------------------------------------------------------------------------------------
def test_errors_and_state(init1024):
    m, p, v = init1024
    lib = _lib.load()
    dp = (C.c_double * 1024)()
    out = C.c_double(-1.0)
    for prec in (P.F64, P.F32, P.MIXED, P.F64_EXACT):
        with engine(1024, precision=prec) as e:
            h = e._h
            assert lib.bh_get_softening(h, C.byref(out)) == 0 and out.value == 0.0
            for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
                assert lib.bh_set_softening(h, bad) == ERR_ARG
            assert lib.bh_get_softening(h, None) == ERR_ARG
            assert lib.bh_set_softening(h, 0.0) == 0
            if prec == P.F64_EXACT:
                assert lib.bh_set_softening(h, 1e-3) == ERR_ARG
                assert b"no softening" in lib.bh_last_error(h)
                assert e.softening == 0.0
                continue
            e.upload(p, v, m)
            assert lib.bh_compute_potential(h) == 0 and lib.bh_get_potential(h, dp, None) == 0
            assert lib.bh_set_softening(h, 1e-3) == 0 and e.softening == 1e-3
            assert lib.bh_get_potential(h, dp, None) == ERR_STATE            # another law's potential
            assert lib.bh_compute_potential(h) == 0 and lib.bh_get_potential(h, dp, None) == 0
            assert lib.bh_set_softening(h, 1e-3) == 0                        # any setter call
            assert lib.bh_get_potential(h, dp, None) == ERR_STATE
    with pytest.raises(G.BhError) as ei:
        engine(16, softening=0.5)                              # the default precision is the bit-exact one
    assert ei.value.code == ERR_ARG
    with pytest.raises(G.BhError):
        engine(16, precision=P.F32, softening=-1.0)


@pytest.mark.parametrize("prec", [P.F32, P.F64])
def test_softened_diagnostics_do_not_perturb_the_trajectory(prec):
    m, p, v = IC.make("plummer", 4096, 4, quasi_static=True)
    pts = FR.points_around(p, 256, 1)
    runs = []
    for diag in (False, True):
        with engine(4096, precision=prec, softening=EPS) as e:
            e.upload(p, v, m)
            for _ in range(8):
                e.step(1)
                if diag:
                    e.energy()
                    e.field(pts)
                    e.force_check(np.arange(0, 4096, 64))
            runs.append(e.download() + (e.stats().walk_launches,))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


# (BH_PRECISION_F64_EXACT takes no softening length: bh_set_softening refuses it, test_errors_and_state)
@pytest.mark.parametrize("prec,n_threads", [c for c in QC.CASES if c[0] != P.F64_EXACT], ids=[i for i in QC.IDS if "EXACT" not in i])
def test_softened_diagnostics_do_not_perturb_the_stats_of_the_last_step(prec, n_threads):
    """tests/quiet_case.py: a first build by the LSD passes, the three quiet builds by the bucket sort."""
    pts = FR.points_around(QC.bodies()[1], 256, 1)

    def diagnostics(e):
        e.energy()
        e.field(pts)
        e.force_check(np.arange(0, QC.N, 64))
    QC.check(prec, n_threads, diagnostics, softening=EPS)
