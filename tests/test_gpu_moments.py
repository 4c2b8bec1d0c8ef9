"""bh_moment_map, bh_moment_map_max and bh_moment_map_deposit on the device, held to the numpy twin tests/moments_ref.py:
every comparison is np.array_equal on the int64 planes, the exponents and n_deposited.

  * all four precisions x both schemes x n in {1, 65, 4097} (one lane, a wave plus one, 16 workgroups plus one) x grids
    1 x 1, 3 x 5, 64 x 64, 257 x 130, on the fixture of moments_ref.fixture (clumps + hand-placed bodies on edges, half a cell
    outside, far outside, coincident; masses over 18 decades; velocities of both signs and zero);
  * bodies at rest: planes 1-3 are zero with exponent 0;
  * a workgroup at the largest cell box it sums in LDS and at the smallest it deposits directly;
  * the planes do not depend on the order of the bodies in memory (a physical re-order, a permuted upload);
  * a map between two steps changes nothing of the run;
  * the errors of include/bhgpu.h;
  * the derived maps of BarnesHutEngine.moment_map;
  * project.py --density-file;
  * LetStepper.moment_map over gloo, world 1 and 2: every rank's planes are one engine's map of the gathered bodies."""
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
import moments_ref as M  # noqa: E402
import quiet_case as Q  # noqa: E402

P = G.Precision
ERR_ARG, ERR_STATE = -1, -5
HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = [P.F32, P.MIXED, P.F64, P.F64_EXACT]
GRIDS = [(1, 1), (3, 5), (64, 64), (257, 130)]
SIZES = [1, 65, 4097]
ENV = ("BH_EXACT_BFS_MAX", "BH_EXACT_BPW", "BH_WALK_ASM", "BH_WALK_SPLIT", "BH_REORDER_EVERY")


def engine(n, precision, **kw):
    if precision in (P.F32, P.MIXED):
        kw.setdefault("max_depth", 21)
        kw.setdefault("reference_compat", False)
    return G.BarnesHutEngine(G.BhConfig(capacity=max(n, 1), precision=precision, **kw))


def bodies(n, precision, nx=64, ny=64, **kw):
    """The fixture as `precision` holds it: an fp32 state cannot hold 1e300, its far bodies stand at 1e38."""
    f32 = precision == P.F32
    return M.state_of(*M.fixture(n, M.BOX, nx, ny, far=1e38 if f32 else 1e300, **kw), precision_is_f32=f32)


def same_as_twin(e, pos, vel, mass, box, nx, ny, scheme, what):
    got = e.moment_map(box, nx, ny, scheme, raw=True)
    planes, ex, n_dep = M.moment_map(pos, vel, mass, box, nx, ny, M.SCHEMES[scheme])
    assert got.planes.dtype == np.int64 and got.planes.shape == (4, ny, nx)
    assert np.array_equal(got.exponents, ex), (what, got.exponents, ex)
    assert got.n_deposited == n_dep, (what, got.n_deposited, n_dep)
    bad = np.argwhere(got.planes != planes)
    assert len(bad) == 0, f"{what}: {len(bad)} cells differ from the twin; first (plane, iy, ix) = {bad[0].tolist()}: " \
                          f"{got.planes[tuple(bad[0])]} != {planes[tuple(bad[0])]}"
    return got


# ---- the twin, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: p.name)
def test_planes_equal_the_twin(precision, n):
    with engine(n, precision) as e:
        for nx, ny in GRIDS:
            pos, vel, mass = bodies(n, precision, nx, ny)
            e.upload(pos, vel, mass)
            for scheme in ("ngp", "cic"):
                got = same_as_twin(e, pos, vel, mass, M.BOX, nx, ny, scheme, f"{precision.name} n={n} {nx}x{ny} {scheme}")
                if n > 1:
                    assert 0 < got.n_deposited < n and got.planes[0].any()
        # the pieces: the maxima, and a deposit with the caller's exponents
        mx = e.moment_map_max()
        assert np.array_equal(mx, M.maxima(pos, vel, mass))
        ex = G.engine.moment_exponents(mx, n) - 3                  # coarser than necessary: still exact integers
        ptr, n_dep = e.moment_map_deposit(M.BOX, nx, ny, "cic", ex)
        planes, n_ref = M.deposit(pos, vel, mass, M.BOX, nx, ny, M.CIC, ex)
        import torch
        got = wrap_device(ptr, 4 * ny * nx, "<i8", torch.device("cuda:0")).cpu().numpy().reshape(4, ny, nx)
        assert np.array_equal(got, planes) and n_dep == n_ref


@pytest.mark.parametrize("precision", [P.F32, P.F64_EXACT], ids=lambda p: p.name)
def test_bodies_at_rest_leave_the_velocity_planes_zero(precision):
    n = 65
    pos, vel, mass = bodies(n, precision, at_rest=True)
    with engine(n, precision) as e:
        e.upload(pos, vel, mass)
        for scheme in ("ngp", "cic"):
            got = same_as_twin(e, pos, vel, mass, M.BOX, 64, 64, scheme, f"at rest {scheme}")
            assert list(got.exponents[1:]) == [0, 0, 0] and not got.planes[1:].any() and got.planes[0].any()
            assert not got.px.any() and not got.k2.any()


def test_no_bodies():
    with engine(4, P.F32) as e:
        e.upload(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        got = e.moment_map(M.BOX, 3, 5, raw=True)
        assert not got.planes.any() and list(got.exponents) == [0, 0, 0, 0] and got.n_deposited == 0
        assert np.array_equal(e.moment_map_max(), np.zeros(4))


@pytest.mark.parametrize("scheme", ["ngp", "cic"])
@pytest.mark.parametrize("width", [32, 33])
def test_the_workgroup_tile_and_its_fallback(scheme, width):
    """A workgroup whose bodies touch at most 1,024 cells sums them in LDS first, one that touches more deposits directly.
    600 bodies (three workgroups, the last partial) on a 64 x 64 grid: the first 256 span exactly 32 x 32 cells (NGP; the
    largest tile) or 33 x 32 (the smallest box that falls back; with CIC one cell more each way), two bodies on opposite
    corners making sure of it; the second 256 sit in one cell; the rest are spread over the whole grid."""
    rng = np.random.default_rng(width)
    nx = ny = 64
    xmin, xmax, ymin, ymax = M.BOX
    hx, hy = (xmax - xmin) / nx, (ymax - ymin) / ny

    def cells(ix, iy):
        return np.stack([xmin + (ix + rng.uniform(0.3, 0.7, len(ix))) * hx, ymin + (iy + rng.uniform(0.3, 0.7, len(iy))) * hy], axis=1)

    a = cells(rng.integers(8, 8 + width, 256), rng.integers(8, 40, 256))
    a[0], a[1] = cells(np.array([8]), np.array([8]))[0], cells(np.array([8 + width - 1]), np.array([39]))[0]
    b = cells(np.full(256, 50), np.full(256, 3))
    c = cells(rng.integers(0, 64, 88), rng.integers(0, 64, 88))
    pos = np.concatenate([a, b, c])
    n = len(pos)
    vel, mass = rng.normal(size=(n, 2)), 10.0 ** rng.uniform(-6.0, 6.0, n)
    ix = np.floor((pos[:256, 0] - xmin) / hx)
    assert ix.max() - ix.min() + 1 == width
    with engine(n, P.F64) as e:
        e.upload(pos, vel, mass)
        got = same_as_twin(e, pos, vel, mass, M.BOX, nx, ny, scheme, f"tile width {width} {scheme}")
        assert got.n_deposited == n


# ---- the order of the bodies in memory ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [P.F32, P.MIXED], ids=lambda p: p.name)
def test_a_physical_reorder_changes_nothing(monkeypatch, precision):
    """BH_REORDER_EVERY=2: three steps re-order the state in memory.  The map of that state equals the map of the same bodies
    uploaded afresh in caller order, and the twin's."""
    import torch
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")
    n = 4097
    pos, vel, mass = bodies(n, precision, hand=False)             # (no body at 1e300: the steps build trees)
    with engine(n, precision, dt=1e-3) as a, engine(n, precision, dt=1e-3) as b:
        a.upload(pos, vel, mass)
        a.step(3)
        p1, v1 = a.download()
        ptr, _, _, _, eb = a.device_state()
        held = wrap_device(ptr, 2 * n, "<f4" if eb == 4 else "<f8", torch.device("cuda:0")).cpu().numpy().reshape(n, 2).astype(np.float64)
        assert not np.array_equal(held, p1)                       # the device order is not the caller's any more ...
        assert np.array_equal(held[np.lexsort(held.T)], p1[np.lexsort(p1.T)])      # ... but the same bodies
        b.upload(p1, v1, mass)
        for scheme in ("ngp", "cic"):
            ma = same_as_twin(a, p1, v1, mass, M.BOX, 64, 64, scheme, f"re-ordered {scheme}")
            mb = b.moment_map(M.BOX, 64, 64, scheme, raw=True)
            assert np.array_equal(ma.planes, mb.planes) and np.array_equal(ma.exponents, mb.exponents)
            assert ma.n_deposited == mb.n_deposited


@pytest.mark.parametrize("precision", [P.F32, P.F64], ids=lambda p: p.name)
def test_a_permuted_upload_changes_nothing(precision):
    n = 4097
    pos, vel, mass = bodies(n, precision)
    perm = np.random.default_rng(1).permutation(n)
    with engine(n, precision) as a, engine(n, precision) as b:
        a.upload(pos, vel, mass)
        b.upload(pos[perm], vel[perm], mass[perm])
        for scheme in ("ngp", "cic"):
            ma, mb = (x.moment_map(M.BOX, 257, 130, scheme, raw=True) for x in (a, b))
            assert np.array_equal(ma.planes, mb.planes) and np.array_equal(ma.exponents, mb.exponents)
            assert ma.n_deposited == mb.n_deposited


# ---- the run is not perturbed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n_threads", Q.CASES, ids=Q.IDS)
def test_a_map_between_two_steps_changes_nothing(monkeypatch, precision, n_threads):
    """quiet_case: bh_stats' record of the last build and walk is the same after the map, and the run goes on bit for bit; then
    step(3); moment_map(); step(3) against step(6) with a physical re-order inside, statistics included."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BH_REORDER_EVERY", "2")

    def plain(n):
        return G.BarnesHutEngine(G.BhConfig(capacity=n, precision=precision, n_threads=n_threads))

    def maps(e):
        for scheme in ("ngp", "cic"):
            e.moment_map((-0.05, 0.05, -0.05, 0.05), 64, 64, scheme)

    Q.check(precision, n_threads, maps)
    m, p, v = Q.bodies()
    with plain(Q.N) as e, plain(Q.N) as control:
        for x in (e, control):
            x.upload(p, v, m)
        e.step(3)
        maps(e)
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
    with engine(65, P.F64) as e:
        assert code_and_text(e.moment_map, M.BOX, 4, 4)[0] == ERR_STATE          # before any upload
        assert code_and_text(e.moment_map_max)[0] == ERR_STATE
        assert code_and_text(e.moment_map_deposit, M.BOX, 4, 4, "cic", [0, 0, 0, 0])[0] == ERR_STATE
        e.upload(pos, vel, mass)
        assert code_and_text(e.moment_map, M.BOX, 4, 4)[0] == 0
        for nx, ny in [(0, 4), (4, 0), (-1, 4), (4, -3), (4097, 4096), (1 << 30, 1 << 30)]:
            assert code_and_text(e.moment_map, M.BOX, nx, ny)[0] == ERR_ARG, (nx, ny)
        good = G.engine.moment_exponents(e.moment_map_max(), 65)
        assert code_and_text(e.moment_map_deposit, M.BOX, 4096, 4096, "ngp", good)[0] == 0      # BH_MAP_MAX_CELLS itself
        nan, inf = float("nan"), float("inf")
        for box in [(1.0, 1.0, 0.0, 1.0), (2.0, 1.0, 0.0, 1.0), (0.0, 1.0, 1.0, 1.0), (0.0, 1.0, 1.0, 0.0), (nan, 1.0, 0.0, 1.0),
                    (0.0, 1.0, 0.0, nan), (-inf, 1.0, 0.0, 1.0), (0.0, inf, 0.0, 1.0), (-1e308, 1e308, 0.0, 1.0)]:
            assert code_and_text(e.moment_map, box, 4, 4)[0] == ERR_ARG, box
        # null pointers and an unknown scheme, on the C-ABI itself
        lib, h = e._lib, e._h
        box = (C.c_double * 4)(*M.BOX)
        planes, ex, nd = (C.c_int64 * 64)(), (C.c_int32 * 4)(), C.c_int64()
        dev = C.c_void_p()
        assert lib.bh_moment_map(h, None, 4, 4, 1, planes, ex, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, 1, None, ex, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, 1, planes, None, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, 1, planes, ex, None) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, 2, planes, ex, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, -1, planes, ex, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(None, box, 4, 4, 1, planes, ex, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map_max(h, None) == ERR_ARG
        assert lib.bh_moment_map_deposit(h, box, 4, 4, 1, None, C.byref(dev), C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map_deposit(h, box, 4, 4, 1, ex, None, C.byref(nd)) == ERR_ARG
        assert lib.bh_moment_map(h, box, 4, 4, 1, planes, ex, C.byref(nd)) == 0
        # exponents that would let a sum leave int64 are refused
        assert code_and_text(e.moment_map_deposit, M.BOX, 4, 4, "cic", good)[0] == 0
        assert code_and_text(e.moment_map_deposit, M.BOX, 4, 4, "cic", good + np.array([0, 1, 0, 0], dtype=np.int32))[0] == ERR_ARG
        # a NaN velocity, an infinite position, an overflowing moment
        for arr, idx, val in [(vel, (7, 1), nan), (pos, (3, 0), inf), (vel, (9, 0), 1e200)]:
            bad_p, bad_v = pos.copy(), vel.copy()
            (bad_v if arr is vel else bad_p)[idx] = val
            e.upload(bad_p, bad_v, mass)
            code, text = code_and_text(e.moment_map, M.BOX, 4, 4)
            assert code == ERR_ARG and "non-finite" in text, (code, text)
            assert code_and_text(e.moment_map_max)[0] == ERR_ARG
        e.upload(pos, vel, mass)
        assert code_and_text(e.moment_map, M.BOX, 4, 4)[0] == 0
    with pytest.raises(ValueError):
        G.BarnesHutEngine._map_args(M.BOX, "tsc")


# ---- the derived maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["ngp", "cic"])
def test_derived_maps(scheme):
    n, nx, ny = 4097, 64, 64
    pos, vel, mass = bodies(n, P.F64)
    with engine(n, P.F64) as e:
        e.upload(pos, vel, mass)
        got = e.moment_map(M.BOX, nx, ny, scheme)
        assert got.planes is None and got.exponents is None       # raw=False
    planes, ex, n_dep = M.moment_map(pos, vel, mass, M.BOX, nx, ny, M.SCHEMES[scheme])
    want = M.convert(planes, ex, M.BOX, nx, ny)
    for k, w in want.items():
        g = getattr(got, k)
        assert g.dtype == np.float64 and g.shape == (ny, nx)
        assert np.array_equal(g, w, equal_nan=True), k
    empty = want["mass"] == 0.0
    assert empty.any() and not empty.all()
    for k in ("vx", "vy", "dispersion"):
        assert np.isnan(getattr(got, k)[empty]).all() and np.isfinite(getattr(got, k)[~empty]).all()
    assert (got.sigma[empty] == 0.0).all()
    assert got.box == M.BOX and got.scheme == scheme and got.n_deposited == n_dep


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def read_rows(path):
    lines = open(path).read().splitlines()
    return lines[0], np.array([[float(t) for t in l.split(",")] for l in lines[1:]])


def test_project_density_file(tmp_path, init1024):
    m, p, v = init1024
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    kw = dict(positions_file="pos.txt", field_file="field.csv", field_grid=(16, 16), energy_file="energy.csv")
    pa, va, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(a), density_file="density.csv", density_grid=(16, 16), **kw)
    pb, vb, _ = project.runSimulationGpu(m, p, v, 2, out_dir=str(b), **kw)
    # without the flag nothing changes: every other output file is the same, byte for byte
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)
    assert not (b / "density.csv").exists()
    for name in ("pos.txt", "field.csv", "energy.csv", "quadtree_init_gpu.txt", "quadtree_final_gpu.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    head, rows = read_rows(a / "density.csv")
    assert head == "# x,y,sigma,vx,vy,dispersion" and rows.shape == (256, 6)
    # the same points as the field file, cell for cell
    _, frows = read_rows(a / "field.csv")
    assert np.array_equal(rows[:, :2], frows[:, :2])
    # the API's map of the same state
    box = (pa[:, 0].min(), pa[:, 0].max(), pa[:, 1].min(), pa[:, 1].max())
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        mm = e.moment_map(box, 16, 16, "cic")
    for col, k in enumerate(("sigma", "vx", "vy", "dispersion"), start=2):
        assert np.array_equal(rows[:, col], getattr(mm, k).reshape(-1), equal_nan=True), k
    assert mm.n_deposited == 1024 and np.isfinite(rows[:, 2]).all()
    # through main(): the flags reach runSimulationGpu
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        from gpu_nbody_simulation_amd.textio import save_init_files
        save_init_files(m, p, v, exact=True)
        assert project.main(["-DN_BODIES=1024", "--n-simulations", "2", "--init", "files", "--density-file", "main.csv",
                             "--density-grid", "16", "16", "--density-scheme", "ngp", "--density-box", "-0.1", "0.1", "-0.1", "0.1"]) == 0
    finally:
        os.chdir(cwd)
    head, rows = read_rows(tmp_path / "main.csv")
    with engine(1024, P.F64_EXACT) as e:
        e.upload(pa, va, m)
        mm = e.moment_map((-0.1, 0.1, -0.1, 0.1), 16, 16, "ngp")
    assert head == "# x,y,sigma,vx,vy,dispersion"
    assert np.array_equal(rows[:, 2], mm.sigma.reshape(-1)) and np.array_equal(rows[:, 5], mm.dispersion.reshape(-1), equal_nan=True)


# ---- distributed ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2])
def test_let_stepper_moment_map(tmp_path, world):
    """World processes over gloo on the one GPU (with this one: at most three with the device open).  After two steps and a
    rebalance() every rank's planes are the same, and the same as one engine's map of the gathered bodies."""
    port = _free_port()
    script = os.path.join(HERE, "moments_ranks.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), str(tmp_path)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{o[-3000:]}"
    import moments_ranks as MR
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ids = np.concatenate([x["ids"] for x in ranks])
    assert sorted(ids.tolist()) == list(range(MR.N))
    if world > 1:
        assert all(len(x["ids"]) > 0 for x in ranks) and all(bool(x["raised"]) for x in ranks)
    pos, vel, mass = (np.concatenate([x[k] for x in ranks]) for k in ("pos", "vel", "mass"))
    with engine(MR.N, P.F32) as e:
        e.upload(pos, vel, mass)
        for scheme in ("ngp", "cic"):
            one = same_as_twin(e, pos, vel, mass, MR.BOX, MR.NX, MR.NY, scheme, f"gathered {scheme}")
            assert 0 < one.n_deposited < MR.N
            for r, x in enumerate(ranks):
                assert np.array_equal(x[scheme + "_planes"], one.planes), (r, scheme)
                assert np.array_equal(x[scheme + "_e"], one.exponents) and int(x[scheme + "_n"]) == one.n_deposited
                assert np.array_equal(x[scheme + "_sigma"], one.sigma)
