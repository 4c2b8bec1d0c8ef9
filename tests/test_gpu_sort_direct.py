"""The bucket sort's direct input (csrc/bh_sort.hpp) on the device: bit for bit the counting pass, bit for
bit the LSD passes.

Every case runs the same bodies three times -- BH_SORT_BUCKET=2 with the direct input under test, BH_SORT_BUCKET=2 with
BH_SORT_DIRECT=0 (the counting pass every time) and BH_SORT_BUCKET=0 (the LSD passes) -- and compares the exported tree of a
later build and the downloaded positions and velocities with ==.  N is between 8,200 and 20,000, so with 256 buckets a range
holds 33 to 79 keys and every workgroup of bucket_sort_kernel has work.

The bodies sit on a jittered lattice with tiny masses: they do not move by themselves ("frozen"), and the state order the
first build leaves (the state is re-ordered at build 0) can be read back slot by slot.  The cases therefore know which bodies
stand at range starts, move only others -- the range keys stay in order, the direct path is taken for as long as the crosser
list holds -- and know which bucket a mover lands in: it is sent next to the body of a chosen slot."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402

NB = 256


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def lattice(n, seed):
    """n bodies on a jittered square lattice in [-1, 1]^2 (one body per lattice cell: positions identify bodies), masses that
    move nobody within a few steps"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cells = rng.permutation(side * side)[:n]
    h = 2.0 / side
    p = np.stack([(cells % side + 0.5) * h - 1.0, (cells // side + 0.5) * h - 1.0], axis=1) + rng.uniform(-0.2 * h, 0.2 * h, (n, 2))
    return f32(rng.uniform(1e-9, 2e-9, n)), f32(p), np.zeros((n, 2)), side


def engine(n, precision=G.Precision.F32, **kw):
    kw.setdefault("max_depth", 21)
    kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=precision, **kw))


def state_order(m, p, side, precision=G.Precision.F32):
    """slot -> caller index after the first build of these bodies at rest (read from the device's state arrays)"""
    import ctypes
    n = len(m)
    with engine(n, precision=precision) as e:
        e.upload(p, np.zeros((n, 2)), m)
        e.step(1)
        e.sync()
        ptr = e.device_state()[0]
        sp = np.empty((n, 2), dtype=np.float32 if precision == G.Precision.F32 else np.float64)
        hip = ctypes.CDLL("libamdhip64.so")                         # (already in the process: libbhgpu links it)
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip.hipMemcpy(sp.ctypes.data, ptr, sp.nbytes, 2) == 0  # 2 = device to host
        sp = sp.astype(np.float64)
    cell = lambda q: (np.floor((q[:, 1] + 1.0) * side / 2.0).astype(np.int64) * side + np.floor((q[:, 0] + 1.0) * side / 2.0).astype(np.int64))
    where = {c: i for i, c in enumerate(cell(p))}
    assert len(where) == n
    order = np.array([where[c] for c in cell(sp)])
    assert np.array_equal(np.sort(order), np.arange(n))
    return order


def run(monkeypatch, env, m, p, v, steps, precision=G.Precision.F32, **kw):
    for k in ("BH_SORT_BUCKET", "BH_SORT_DIRECT", "BH_SORT_DIRECT_MAX", "BH_REORDER_EVERY"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    n = len(m)
    with engine(n, precision=precision, **kw) as e:
        e.upload(p, v, m)
        e.step(steps)
        e.build_tree()
        nodes, depth = e.export_tree()
        e.step(1)
        pos, vel = e.download()[:2]
        st = e.stats()
    return nodes, depth, pos, vel, st


def compare(monkeypatch, m, p, v, steps, direct="1", extra=None, **kw):
    extra = extra or {}
    new = run(monkeypatch, dict(BH_SORT_BUCKET="2", BH_SORT_DIRECT=direct, **extra), m, p, v, steps, **kw)
    reorder = {k: val for k, val in extra.items() if k == "BH_REORDER_EVERY"}
    old = run(monkeypatch, dict(BH_SORT_BUCKET="2", BH_SORT_DIRECT="0", **reorder), m, p, v, steps, **kw)
    lsd = run(monkeypatch, dict(BH_SORT_BUCKET="0", **reorder), m, p, v, steps, **kw)
    for other in (old, lsd):
        for x, y in zip(new[:4], other[:4]):
            if x.dtype.names:
                for f in x.dtype.names:
                    assert np.array_equal(x[f], y[f], equal_nan=True), f
            else:
                assert np.array_equal(x, y)
    assert np.isfinite(new[2]).all() and np.isfinite(new[3]).all()
    return new[4], old[4]


def send(p, v, order, movers, targets, steps):
    """the bodies of the slots `movers` travel to just beside the bodies of the slots `targets` in `steps` steps (dt = 1)"""
    v = v.copy()
    for a, b in zip(movers, targets):
        v[order[a]] = f32((p[order[b]] + 1e-4 - p[order[a]]) / steps)
    return v


def off_starts(slots, L):
    """the slots, each moved on by one where it is a range start"""
    return [s + 1 if s % L == 0 else s for s in slots]


def test_frozen_bodies_have_no_crosser(monkeypatch):
    m, p, v, _ = lattice(9001, 1)
    new, old = compare(monkeypatch, m, p, v, 3)
    assert new.sort_spill_buckets == 0 and old.sort_spill_buckets == 0


def test_a_dozen_bodies_cross_the_domain(monkeypatch):
    """Twelve bodies travel across the box in three steps: four into one bucket (two of them from below, two from above it),
    two into bucket 0, two into the last bucket that has a range (n = 10,000: 250 ranges of 40, six empty ones behind, which
    no key can reach -- their range key is above every key), the rest to scattered places; one of them leaves a range whose
    neighbours it will pass again.  Every build after the first meets them somewhere else."""
    n = 10000
    m, p, v, side = lattice(n, 2)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    movers = off_starts([7, 3 * L + 5, 180 * L + 9, 200 * L + 11, 100 * L + 3, 101 * L + 4, 5 * L + 6, 6 * L + 7, 40 * L + 1, 77 * L + 2,
                         150 * L + 13, 249 * L + 3], L)
    targets = [120 * L + 4, 120 * L + 9, 120 * L + 14, 120 * L + 19, 2, 5, n - 3, n - 6, 230 * L + 8, 20 * L + 8, 60 * L + 8, 9 * L + 8]
    v = send(p, v, order, movers, targets, 3)
    compare(monkeypatch, m, p, v, 3)
    compare(monkeypatch, m, p, v, 1)                            # (the build that is compared is the first with crossers)


@pytest.mark.parametrize("movers", [8, 9])
def test_both_sides_of_the_capacity(monkeypatch, movers):
    """BH_SORT_DIRECT_MAX=8: eight bodies away from home fit the list, with the ninth the counter passes the capacity and the
    build takes the counting pass.  (The movers are away from their ranges at every build after the first.)"""
    n = 8200
    m, p, v, side = lattice(n, 3)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    src = off_starts([11 + 25 * L * k for k in range(movers)], L)
    dst = [(s + 120 * L) % n for s in src]
    v = send(p, v, order, src, dst, 4)
    compare(monkeypatch, m, p, v, 3, extra=dict(BH_SORT_DIRECT_MAX="8"))


def test_a_third_of_the_bodies_cross_with_the_list_sized_for_all(monkeypatch):
    """BH_SORT_DIRECT=2: every third body that is not at a range start trades places with another one over four steps, so
    from the second build on thousands of keys are listed and most buckets merge dozens of arrivals from both sides."""
    n = 15000
    m, p, v, side = lattice(n, 4)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    rng = np.random.default_rng(5)
    src = np.array([s for s in range(n) if s % 3 == 1 and s % L != 0])
    dst = rng.permutation(src)
    v = send(p, v, order, src, dst, 4)
    compare(monkeypatch, m, p, v, 3, direct="2")
    compare(monkeypatch, m, p, v, 1, direct="2")


def test_a_body_flung_far_moves_the_root_box(monkeypatch):
    """One body leaves at 40 box widths per step: the root box jumps, every key changes and so does the order along the curve --
    range keys out of order or crossers by the thousand, the builds take the counting pass, whatever the list holds; the same
    body coming to rest inside the hull (second run: it only crosses the box) leaves the later builds on the direct path."""
    n = 12000
    m, p, v, side = lattice(n, 6)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    far = v.copy()
    far[order[50 * L + 3]] = [80.0, 55.0]
    compare(monkeypatch, m, p, far, 4)
    compare(monkeypatch, m, p, far, 4, direct="2")
    compare(monkeypatch, m, p, send(p, v, order, [50 * L + 3], [200 * L + 3], 2), 4)


def test_coincident_bodies_on_a_range_boundary(monkeypatch):
    """Five bodies at one point astride a range start (equal keys: body order decides, and two range keys may be equal), with
    Plummer softening so that their mutual forces are finite; some of them then drift apart, one travels away."""
    n = 9000
    m, p, v, side = lattice(n, 7)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    p = p.copy()
    for s in (60 * L - 2, 60 * L - 1, 60 * L + 1, 60 * L + 2):
        p[order[s]] = p[order[60 * L]]
    # (also a whole range and its neighbour's start at one point: range keys 90 and 91 equal)
    for s in range(90 * L + 1, 91 * L + 1):
        p[order[s]] = p[order[90 * L]]
    v2 = send(p, v, order, [60 * L + 2, 90 * L + 5], [10 * L + 5, 200 * L + 7], 3)
    for direct in ("1", "2"):
        compare(monkeypatch, m, p, v, 3, direct=direct, softening=1e-3)
        compare(monkeypatch, m, p, v2, 3, direct=direct, softening=1e-3)


def test_reordering_every_second_build(monkeypatch):
    n = 11000
    m, p, v, side = lattice(n, 8)
    order = state_order(m, p, side)
    L = (n + NB - 1) // NB
    src = off_starts([9 + 13 * L * k for k in range(15)], L)
    v = send(p, v, order, src, [(s + 97 * L) % n for s in src], 6)
    compare(monkeypatch, m, p, v, 5, extra=dict(BH_REORDER_EVERY="2"))
    compare(monkeypatch, m, p, v, 5, direct="2", extra=dict(BH_REORDER_EVERY="2"))


def test_ranges_of_unequal_length(monkeypatch):
    """N = 8,191 + 4 x 64 + 1 = 8,448 fills 256 ranges of 33 exactly; one body more or less leaves a shorter last range
    (8,447) or 249 ranges of 34 with seven empty ones behind (8,449)."""
    for n in (8191 + 4 * 64 + 1, 8447, 8449):
        m, p, v, side = lattice(n, 9)
        order = state_order(m, p, side)
        L = (n + NB - 1) // NB
        last = ((n - 1) // L) * L
        src = off_starts([5, last + 1, 100 * L + 2, n - 1], L)
        v = send(p, v, order, src, [last + 2, 3, n - 2, 30 * L + 2], 3)
        compare(monkeypatch, m, p, v, 3)


def test_mixed_precision(monkeypatch):
    n = 9500
    m, p, v, side = lattice(n, 10)
    order = state_order(m, p, side, precision=G.Precision.MIXED)
    L = (n + NB - 1) // NB
    src = off_starts([4, 33 * L + 2, 99 * L + 7, 170 * L + 1, 240 * L + 9], L)
    v = send(p, v, order, src, [200 * L + 3, 1, 98 * L + 1, 171 * L + 4, 12 * L + 2], 3)
    compare(monkeypatch, m, p, v, 3, precision=G.Precision.MIXED)
    compare(monkeypatch, m, p, v, 3, direct="2", precision=G.Precision.MIXED)
