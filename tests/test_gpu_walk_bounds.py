"""The root box every integrating walk leaves for the next build.

A walk over all bodies that integrates folds the min / max of the NEW positions into the bounds slot records
(bh_bounds.hpp), and the next keys_kernel pads them into the next tree's root box.  That box is an output of every walk
kernel, in every precision and launch shape, and the trajectory comparisons hardly see it: a record off by a * dt^2 moves
every node's size / threshold by ~1e-8 relative and almost never a cell boundary.  So here the box is checked directly:
step once, download the positions, step once more, export the tree that step built -- its root box must be
ComputeRootBounds (tests/box_ref.py) of the downloaded positions, bit for bit.  A back-to-back leg without the downloads
and exports must end on the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bh_oracle as O  # noqa: E402
import gpu_nbody_simulation_amd as G  # noqa: E402
from gpu_nbody_simulation_amd.engine import FLAG_LDS_STACK, FLAG_WALK_PORTABLE  # noqa: E402
from box_ref import box_ref, root_box  # noqa: E402
from direct_ref import same_bits  # noqa: E402
from test_gpu_exact import _same_tree  # noqa: E402

K = 3                       # (step, download, step, export) rounds per case
ENV = ("BH_EXACT_BFS_MAX", "BH_EXACT_BPW", "BH_WALK_ASM", "BH_WALK_SPLIT", "BH_REORDER_EVERY")


def _bodies(n, seed, kind="mixed"):
    """Positions ~1, masses 0.1-0.5 everywhere (the extreme bodies are real bodies), velocities ~1e-7: with G = 6.67e-11 and
    dt = 1 an edge body moves by a * dt^2 ~ 1e-8 per step, ~1e8 ulps of its coordinate."""
    r = np.random.default_rng(seed)
    if kind == "mixed":
        p = np.concatenate([r.normal(0, 5e-2, (n // 2, 2)), r.uniform(-1, 1, (n - n // 2, 2))])
    elif kind == "dense":                         # a few tight clusters: a deep tree, wide breadth-first frontiers
        c = r.uniform(-1, 1, (4, 2))
        p = c[r.integers(0, 4, n)] + r.normal(0, 1e-3, (n, 2))
        p[: n // 8] = r.uniform(-1, 1, (n // 8, 2))
    else:
        raise ValueError(kind)
    return p, r.uniform(-1e-7, 1e-7, (n, 2)), r.uniform(0.1, 0.5, n)


def _env(monkeypatch, **kw):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def _check_boxes(cfg, p, v, m, oracle=False):
    """K rounds of step / download / step / export_tree: the exported root box is box_ref of the downloaded positions, bit for
    bit.  oracle (exact mode): the exported tree is also the oracle's tree of those positions, and the second step's positions
    are O.integrate of the oracle's forces.  Then the same 2K steps back to back on a fresh context end on the same bits."""
    with G.BarnesHutEngine(cfg) as e:
        e.upload(p, v, m)
        for k in range(K):
            e.step(1)
            pos, vel = e.download()
            e.step(1)
            nodes, _ = e.export_tree()
            assert np.isfinite(pos).all()
            got, want = root_box(nodes), box_ref(pos)
            assert same_bits(got, want), (k, "root box", got, want, got - want)
            if oracle:
                t = O.build_tree(pos, m, cfg.max_depth)
                _same_tree(e, t)
                f = O.compute_forces(t, pos, m, theta=cfg.theta, G=cfg.G, compat_self_skip=cfg.reference_compat)
                _, _, po = O.integrate(f, m, vel, pos, dt=cfg.dt)
                assert same_bits(e.download()[0], po), k
        last = e.download()
    with G.BarnesHutEngine(cfg) as e:
        e.upload(p, v, m)
        e.step(2 * K)
        again = e.download()
    assert same_bits(last[0], again[0]) and same_bits(last[1], again[1])


# ---- exact mode, breadth-first walk (walk_exact_bfs_kernel) ------------------------------------------------------------

def _bfs_grid(n, capacity):
    """launch_walk_exact_bfs (bh_engine.hip): max(min(ceil(n / 4), max(1,024, ceil(capacity / 64))), ceil(n / 256)) workgroups
    of four wavefronts; sorted body s is taken by wave s % 4 of workgroup (s // 4) % grid in turn s // (4 * grid), and that
    turn's lane records the body's new position for the workgroup's bounds."""
    max_groups = max(1024, -(-capacity // 64))
    return max(min(-(-n // 4), max_groups), -(-n // 256))


def _sorted_rank(p, max_depth):
    """Rank of every body in the build's sort: keys of max_depth - 1 DetermineChild digits in the root box, child index
    ascending (key_of, bh_tree.hpp: child 0 = x < mid and y < mid ... child 3 first-digit-largest), ties in body order."""
    x0, x1, y0, y1 = (np.full(len(p), b) for b in box_ref(p))
    key = np.zeros(len(p), dtype=np.uint64)
    for _ in range(max_depth - 1):
        mx, my = (x0 + x1) / 2, (y0 + y1) / 2
        c = np.where(p[:, 0] < mx, 0, 1) + np.where(p[:, 1] < my, 0, 2)
        key = (key << np.uint64(2)) | c.astype(np.uint64)
        x0, x1 = np.where(c & 1, mx, x0), np.where(c & 1, x1, mx)
        y0, y1 = np.where(c & 2, my, y0), np.where(c & 2, y1, my)
    rank = np.empty(len(p), dtype=np.int64)
    rank[np.lexsort((np.arange(len(p)), key))] = np.arange(len(p))
    return rank


REFLECT = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
# (a weaker G: the closest pairs of these sets would otherwise fly apart within the checked steps; an edge body still
# moves by a * dt^2 ~ 1e-11 per step, ~1e5 ulps of its coordinate)
GC = 1e-14

# (n, capacity, BH_EXACT_BFS_MAX or None, distribution, max_depth): the launch shapes of the breadth-first walk
# (deep enough that no body sits alone in a depth-cap cell: without reference_compat the reference does not skip such a
# body's own term, and its position turns NaN)
BFS_SHAPES = {
    "turn0": (4000, 4000, None, "mixed", 24),               # one turn; the 256-term list
    "turns2": (6000, 6000, None, "mixed", 24),              # turns 0, 1; the 384-term list
    "turns3": (12288, 12288, None, "mixed", 24),            # turns 0 .. 2, the default limit
    "uncapped": (6000, 131072, None, "mixed", 24),          # grid not capped: one turn
    "max20k": (20000, 20000, 20000, "mixed", 24),           # turns 0 .. 4
    "dense": (6000, 6000, None, "dense", 32),               # deep clustered tree: long term lists and wide queues
}


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("theta", [0.5, 0.2, 1e-3])
@pytest.mark.parametrize("shape", list(BFS_SHAPES))
def test_breadth_first_walk_leaves_the_root_box(monkeypatch, shape, theta, compat):
    """walk_exact_bfs_kernel: one wavefront per body, up to 64 bodies per wave one after the other (`turn`); lane `turn` keeps
    the body's new position for the workgroup's bounds record.  A body whose term list or queue overflows is walked again by
    lane 0 alone (walk_exact_asm) -- every lane must still integrate lane 0's sums, or a body of turn >= 1 records p + v * dt
    without the force term.  theta 1e-3: every body spills; every shape in its four reflections, so that the extreme bodies
    come late in key order (turn >= 1) in at least one of them."""
    n, cap, bfs_max, kind, md = BFS_SHAPES[shape]
    _env(monkeypatch, **({"BH_EXACT_BFS_MAX": bfs_max} if bfs_max else {}))
    assert n <= (bfs_max or 12288)
    grid = _bfs_grid(n, cap)
    terms = 256 if n <= 4096 else 384
    turns = -(-n // (4 * grid))
    assert turns == {"turn0": 1, "turns2": 2, "turns3": 3, "uncapped": 1, "max20k": 5, "dense": 2}[shape]
    p0, v, m = _bodies(n, 11 + n, kind)
    reached = []
    for rx, ry in REFLECT:
        p = p0 * np.array([rx, ry])
        cfg = G.BhConfig(capacity=cap, theta=theta, max_depth=md, reference_compat=compat, G=GC)
        if theta == 1e-3 and turns > 1:
            # the faulty path: an extreme body taken in turn >= 1 whose walk overflows the term list
            rank = _sorted_rank(p, md)
            t = O.build_tree(p, m, md)
            for b in {int(np.argmin(p[:, 0])), int(np.argmax(p[:, 0])), int(np.argmin(p[:, 1])), int(np.argmax(p[:, 1]))}:
                cnt = int(O.compute_forces_diag(t, p, m, theta=theta, compat_self_skip=compat, lo=b, hi=b + 1).counts[b])
                assert cnt > terms
                reached.append(rank[b] // (4 * grid) >= 1)
        # the oracle's O(N^2) steps: one reflection of the two-turn shape
        oracle = theta > 0.1 or (shape == "turns2" and (rx, ry) == (1, 1))
        _check_boxes(cfg, p, v, m, oracle=oracle)
    if theta == 1e-3 and turns > 1:
        assert any(reached), "no extreme body came in turn >= 1"


# ---- exact mode, cooperative walk (walk_exact_kernel) ------------------------------------------------------------------

@pytest.mark.parametrize("case", ["bpw_default", "bpw1", "bpw4", "bpw64", "portable", "no_asm", "n_threads"])
def test_cooperative_exact_walk_leaves_the_root_box(monkeypatch, case):
    """walk_exact_kernel: BH_EXACT_BFS_MAX=0 keeps every launch on it; bodies per wavefront from the default to 64, the
    hand-written loop against the portable walk and the C++ loop, and passes of n_threads bodies with an uneven last pass
    (every pass folds its records into the same slots)."""
    n, nt, flags = 5000, 0, 0
    env = {"BH_EXACT_BFS_MAX": 0}
    if case.startswith("bpw") and case != "bpw_default":
        env["BH_EXACT_BPW"] = case[3:]
    elif case == "portable":
        flags = FLAG_WALK_PORTABLE
    elif case == "no_asm":
        env["BH_WALK_ASM"] = 0
    elif case == "n_threads":
        n, nt = 40001, 4096
    _env(monkeypatch, **env)
    p, v, m = _bodies(n, 21 + n)
    cfg = G.BhConfig(capacity=n, max_depth=14, n_threads=nt, flags=flags)
    _check_boxes(cfg, p, v, m, oracle=n <= 5000)


# ---- fp64 throughput walk (walk_f64_kernel) ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["n1024", "n16384", "n40000", "bpw1", "no_asm", "deep", "n_threads"])
def test_f64_walk_leaves_the_root_box(monkeypatch, case):
    """walk_f64_kernel: the default bodies per wavefront at three sizes, BH_EXACT_BPW=1, the C++ loop, the two-tier stack of
    trees deeper than 21 levels, and n_threads with an uneven last pass."""
    n, md, nt, env = 16384, 14, 0, {}
    if case.startswith("n") and case[1:].isdigit():
        n = int(case[1:])
    elif case == "bpw1":
        env["BH_EXACT_BPW"] = 1
    elif case == "no_asm":
        env["BH_WALK_ASM"] = 0
    elif case == "deep":
        md = 26
    elif case == "n_threads":
        n, nt = 40001, 4096
    _env(monkeypatch, **env)
    p, v, m = _bodies(n, 31 + n, "dense" if case == "deep" else "mixed")
    _check_boxes(G.BhConfig(capacity=n, max_depth=md, n_threads=nt, precision=G.Precision.F64), p, v, m)


# ---- fp32 and mixed walks (walk_fast_kernel) ---------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [G.Precision.F32, G.Precision.MIXED])
@pytest.mark.parametrize("case", ["split1", "split2", "split4", "split8", "no_asm", "lds_stack", "n_threads", "odd_n",
                                  "reorder2"])
def test_fast_walk_leaves_the_root_box(monkeypatch, precision, case):
    """walk_fast_kernel: BH_WALK_SPLIT 1 to 8 (SPLIT > 1: wave 0 writes one record per 64-body group), the C++ loop, the LDS
    stack, n_threads passes, N a multiple of neither 64 nor 256, and BH_REORDER_EVERY=2 (the bodies are physically
    re-ordered inside the checked steps)."""
    n, nt, flags, env = 5000, 0, 0, {}
    if case.startswith("split"):
        env["BH_WALK_SPLIT"] = case[5:]
    elif case == "no_asm":
        env["BH_WALK_ASM"] = 0
    elif case == "lds_stack":
        flags = FLAG_LDS_STACK
    elif case == "n_threads":
        n, nt = 40001, 4096
    elif case == "odd_n":
        n = 5037
    elif case == "reorder2":
        env["BH_REORDER_EVERY"] = 2
    _env(monkeypatch, **env)
    p, v, m = _bodies(n, 41 + n)
    if precision == G.Precision.F32:
        p, v, m = (x.astype(np.float32).astype(np.float64) for x in (p, v, m))
    _check_boxes(G.BhConfig(capacity=n, max_depth=16, n_threads=nt, flags=flags, precision=precision), p, v, m)
