"""GPU parity, BH_PRECISION_MIXED (BASELINE config "fp64 positions / fp32 forces"): the state is kept
and integrated in fp64, tree keys and centres of mass come from the fp64 positions, the theta-walk runs
in fp32 on rounded copies.

Stated tolerances, per body, against the fp64 oracle on the SAME fp64 inputs (not fp32-representable,
so rounding the walk's copies is part of the error): relative acceleration error
    median <= 5e-6 ; 99.9 % <= 5e-4 ; every body <= 2e-2
(the oracle here is the uncapped tree + per-body MAC; the tail is MAC flips as in test_gpu_fp32.py).
Displacements over k quasi-static steps (|dx| << fp32 resolution of x) track the oracle's fp64 run to
1e-5 relative, where BH_PRECISION_F32 cannot move the bodies at all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd import initial_conditions as IC  # noqa: E402
from test_gpu_let import EmulatedRanks, rel  # noqa: E402
from nodes_ref import Twin  # noqa: E402


def engine(n, precision=G.Precision.MIXED, **kw):
    kw.setdefault("max_depth", 21)
    kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=precision, **kw))


@pytest.mark.parametrize("kind,n", [("uniform", 40000), ("plummer", 65536)])
def test_mixed_accelerations_and_tree(kind, n):
    m, p, v = IC.make(kind, n, 5)
    p = p * (1.0 + 3e-9 * np.random.default_rng(1).standard_normal(p.shape))   # not fp32-representable
    assert not np.array_equal(p, p.astype(np.float32).astype(np.float64))
    t = O.build_tree(p, m, 0)
    ref = O.compute_forces(t, p, m, compat_self_skip=False) / m[:, None]
    with engine(n) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a = e.accelerations()
        f = e.forces()
        nodes, depth = e.export_tree()
        pd, vd = e.download()
        md = e.masses()
    # state is held in fp64: what went in comes back bit for bit
    assert np.array_equal(pd, p) and np.array_equal(vd, v) and np.array_equal(md, m)
    r = rel(a, ref)
    assert np.median(r) <= 5e-6 and np.quantile(r, 0.999) <= 5e-4 and r.max() <= 2e-2
    np.testing.assert_allclose(f, a * m[:, None], rtol=1e-12)
    # the tree is the tree of the fp64 positions (keys are computed from them)
    t21 = O.build_tree(p, m, 21)
    assert len(nodes) == len(t21)
    root = nodes[0]
    lo, hi = p.min(0), p.max(0)
    ex = max(hi - lo)
    np.testing.assert_allclose([root["xmin"], root["xmax"], root["ymin"], root["ymax"]],
                               [lo[0] - 0.1 * ex, hi[0] + 0.1 * ex, lo[1] - 0.1 * ex, hi[1] + 0.1 * ex], rtol=1e-14)
    np.testing.assert_allclose(root["mass"], m.sum(), rtol=1e-6)


@pytest.mark.parametrize("precision", [G.Precision.MIXED, G.Precision.F32, G.Precision.F64_EXACT, G.Precision.F64])
def test_fast_keys_equal_the_bisection_keys(precision):
    """keys_kernel takes a body's cell from one multiply per axis when the body is provably clear of every
    grid line and falls back to the reference's bisection otherwise.  Bodies placed EXACTLY on the
    bisection's own (rounded) midpoints, one ulp below and one ulp above them, on both axes, at every depth,
    and on the box corners: the exported tree is the oracle's, cell by cell and occupant by occupant.
    (Round 4: the exact modes take the same look-up, with child-index digits instead of curve digits; there the
    centres of mass and masses are the reference's bit for bit as well.  Precision.F32 sees the same points rounded to
    float32; there and in MIXED mass and centre of every node are held to the bound derived in tests/nodes_ref.py.)"""
    rng = np.random.default_rng(17)
    corners = np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]])
    lo, hi = corners.min(0), corners.max(0)
    span = max(hi - lo)
    pad = 0.1 * span
    box = (lo[0] - pad, hi[0] + pad, lo[1] - pad, hi[1] + pad)               # bounds_final's formula

    def midpoint(a, b, depth):
        for _ in range(depth):                                                # a random path of the bisection
            mid = (a + b) / 2
            if rng.random() < 0.5:
                a = mid
            else:
                b = mid
        return (a + b) / 2

    pts = [corners, rng.uniform(-0.999, 0.999, (6000, 2))]
    for _ in range(1500):
        d = int(rng.integers(0, 20))
        bx, by = midpoint(box[0], box[1], d), midpoint(box[2], box[3], d)
        if not (-0.999 < bx < 0.999 and -0.999 < by < 0.999):
            continue
        xs = [bx, np.nextafter(bx, -np.inf), np.nextafter(bx, np.inf)]
        ys = [by, np.nextafter(by, -np.inf), np.nextafter(by, np.inf)]
        free = rng.uniform(-0.999, 0.999, 6)
        pts.append(np.array([[xs[0], free[0]], [xs[1], free[1]], [xs[2], free[2]],
                             [free[3], ys[0]], [free[4], ys[1]], [free[5], ys[2]],
                             [xs[0], ys[0]], [xs[1], ys[2]], [xs[2], ys[1]]]))
    p = np.concatenate(pts)
    n = len(p)
    m = rng.uniform(0.5, 1.0, n) * 1e-12
    v = np.zeros((n, 2))
    if precision == G.Precision.F32:
        p, m = (a.astype(np.float32).astype(np.float64) for a in (p, m))
    with engine(n, precision=precision) as e:
        e.upload(p, v, m)
        e.build_tree()
        nodes, depth = e.export_tree()
    rn, rd = O.canonical_tree(O.build_tree(p, m, 21))
    assert len(nodes) == len(rn) and np.array_equal(depth, rd)
    exact = precision not in (G.Precision.MIXED, G.Precision.F32)
    for f in ("xmin", "xmax", "ymin", "ymax", "particle") + (("comx", "comy", "mass") if exact else ()):
        assert np.array_equal(nodes[f], rn[f]), f
    assert np.array_equal(nodes["child"] == -1, rn["child"] == -1)
    if not exact:
        res = Twin(p, m, 21).check(nodes, depth, mixed=precision == G.Precision.MIXED)
        print(res)
        assert res["nodes"] == len(rn) and res["undecided"] == 0 and res["unresolved"] == 0


def test_mixed_keeps_displacements_below_fp32_resolution():
    n, steps = 20000, 5
    m, p, v = IC.make("uniform", n, 8, quasi_static=True)   # |v| <= 1e-9 per step against |x| ~ 0.1
    p = p * (1.0 + 3e-9 * np.random.default_rng(2).standard_normal(p.shape))
    # oracle run: uncapped tree, per-body MAC, fp64 state
    pos, vel = p.copy(), v.copy()
    for _ in range(steps):
        t = O.build_tree(pos, m, 0)
        f = O.compute_forces(t, pos, m, compat_self_skip=False)
        _, vel, pos = O.integrate(f, m, vel, pos)
    d_ref = pos - p
    assert np.abs(d_ref).max() < 1e-7                      # far below the fp32 spacing of coordinates ~0.1 (7e-9)...
    out = {}
    for prec in (G.Precision.MIXED, G.Precision.F32):
        with engine(n, precision=prec) as e:
            e.upload(p, v, m)
            e.step(steps)
            out[prec] = e.download()
    d_mixed = out[G.Precision.MIXED][0] - p
    r = np.linalg.norm(d_mixed - d_ref, axis=1) / np.linalg.norm(d_ref, axis=1)
    assert np.median(r) < 1e-5 and np.quantile(r, 0.999) < 1e-3
    dv = out[G.Precision.MIXED][1] - v
    rv = np.linalg.norm(dv - (vel - v), axis=1) / np.linalg.norm(vel - v, axis=1)
    assert np.median(rv) < 1e-5
    # fp32 state: the same run cannot resolve these displacements
    p32 = p.astype(np.float32).astype(np.float64)
    d_f32 = out[G.Precision.F32][0] - p32
    r32 = np.linalg.norm(d_f32 - d_ref, axis=1) / np.linalg.norm(d_ref, axis=1)
    assert np.median(r32) > 0.1


def test_mixed_let_forest_and_refusals():
    n = 30000
    m, p, v = IC.make("plummer", n, 6)
    idx = np.arange(0, n, 53)
    sub = np.zeros((len(idx), 2))
    for k, i in enumerate(idx):
        d = p - p[i]
        r2 = (d ** 2).sum(1)
        r2[i] = np.inf
        sub[k] = (6.67e-11 * m[:, None] * d / (r2 ** 1.5)[:, None]).sum(0)
    er = EmulatedRanks(m, p, v, 3, let_cap=8192, precision=G.Precision.MIXED, max_depth=21, reference_compat=False)
    er.step(integrate=False)
    a = er.gather(lambda e: e.accelerations())
    er.step()                                              # integrates the fp64 state
    pn = er.gather(lambda e: e.download()[0])
    er.close()
    with engine(n) as e:
        e.upload(p, v, m)
        e.compute_forces()
        a1 = e.accelerations()
        with pytest.raises(G.BhError) as ei:
            e.step_local()
        assert ei.value.code == -5
        with pytest.raises(G.BhError):
            e.device_sorted()
    assert np.median(rel(a[idx], sub)) <= 1.2 * np.median(rel(a1[idx], sub)) + 1e-6
    assert np.isfinite(pn).all() and not np.array_equal(pn, p)
