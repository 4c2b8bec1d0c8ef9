"""The harness of tests/test_gpu_sort_direct.py and tests/test_gpu_sort_direct_edges.py: bodies that do not move by themselves,
sent where a case wants them, run three times, and the build under test pinned to the numpy twin through the engine's snapshot.

Every case runs the same bodies three times -- BH_SORT_BUCKET=2 with the direct input under test, BH_SORT_BUCKET=2 with
BH_SORT_DIRECT=0 (the counting pass every time) and BH_SORT_BUCKET=0 (the LSD passes) -- and compares the exported tree of a
later build and the downloaded positions and velocities with ==.

The bodies sit on a jittered lattice with tiny masses: they do not move by themselves ("frozen"), and the state order the
first build leaves (the state is re-ordered at build 0) can be read back slot by slot.  The cases therefore know which bodies
stand at range starts, move only others -- the range keys stay in order -- and know where a mover lands: it is sent next to the
body of a chosen slot.

The build whose tree is exported is also snapshotted (BarnesHutEngine.sort_snapshot), and check_snapshot runs the twin
(tests/sort_direct_ref.py) on the keys THE DEVICE formed: the decision the device took is the twin's, on the direct path the list
counters add up to the twin's crossers, the listed words are the twin's crossers and the range keys the twin's, and on either
path the sort's output is numpy's stable sort of those keys."""
import ctypes
from types import SimpleNamespace

import numpy as np

import gpu_nbody_simulation_amd as G
import sort_direct_ref as R

NB = 256
U64 = np.uint64


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
    mine = cell(p)
    by_cell = np.argsort(mine)
    assert (np.diff(mine[by_cell]) > 0).all()                      # one body per lattice cell
    at = np.searchsorted(mine[by_cell], cell(sp))
    assert (at < n).all() and np.array_equal(mine[by_cell][at], cell(sp))
    order = by_cell[at]
    assert np.array_equal(np.sort(order), np.arange(n))
    return order


def hull_slots(p, order):
    """the slots of the bodies that carry the root box (least and greatest x and y).  While they stay, the box stays, every body
    that does not move keeps its key, and the crossers of a later build are movers only; let one of them leave and the box
    shrinks, the cells shift, and a handful of bodies next to range boundaries change sides"""
    at = {int(f(p[:, a])) for a in (0, 1) for f in (np.argmin, np.argmax)}
    return {int(s) for s in np.flatnonzero(np.isin(order, list(at)))}


def check_snapshot(s, path=None, k=None, why=None):
    """the snapshot of a build that was offered direct input against the twin on the device's own keys -> the Twin"""
    assert s.offered and s.keys_in is not None
    n = s.n
    assert np.array_equal(s.keys_in >> U64(R.PACK_SHIFT), np.arange(n, dtype=U64))      # slot i holds body i's word
    assert s.nb == (256 if n <= 1 << 20 else 1024) and s.L == (n + s.nb - 1) // s.nb
    tw = R.direct_sort_fast(s.keys_in, s.nb, s.cap, s.subcap, s.nsub)
    assert s.L == tw.L
    held = s.decision[1:1 + s.nsub].astype(np.int64)
    print(f"snapshot n {n} nb {s.nb} L {s.L} T {s.cap} room {s.subcap} lists {s.nsub}: device word0 {s.decision[0]} listed {held.sum()} "
          f"most in a list {held.max()} -> {'counting' if s.counting else 'direct'}; twin {tw.path} {tw.why} crossers {tw.k}")
    assert s.counting == (tw.path == "counting"), (s.decision[0], held.sum(), held.max(), tw.path, tw.why, tw.k)
    if path is not None:
        assert tw.path == path, (tw.path, tw.why, tw.k)
    if k is not None:
        assert tw.k == k, (tw.k, k)
    if why is not None:
        assert tw.why == why, (tw.why, why)
    if tw.path == "direct":
        # (on the counting path the counters stop being exact once the fall-back word is set: only the decision is compared)
        assert s.decision[0] == 0 and not s.decision[1 + s.nsub:].any()
        assert held.sum() == tw.k
        want = np.bincount((tw.crossers >> 6) & (s.nsub - 1), minlength=s.nsub)
        assert np.array_equal(held, want)                                             # every wave queued at its own list
        listed = np.concatenate([s.lists[j, :held[j]] for j in range(s.nsub)]) if tw.k else np.zeros(0, dtype=U64)
        assert np.array_equal(np.sort(listed), np.sort(s.keys_in[tw.crossers]))
        assert np.array_equal(s.range_keys, tw.rk)
    assert np.array_equal(s.keys_sorted | (s.perm.astype(U64) << U64(R.PACK_SHIFT)), R.expect(s.keys_in))
    return tw


def run(monkeypatch, env, m, p, v, steps, precision=G.Precision.F32, **kw):
    for k in ("BH_SORT_BUCKET", "BH_SORT_DIRECT", "BH_SORT_DIRECT_MAX", "BH_REORDER_EVERY"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    n = len(m)
    with engine(n, precision=precision, **kw) as e:
        e.upload(p, v, m)
        e.step(steps)
        s0 = e.stats()
        e.build_tree()
        snap = e.sort_snapshot()
        s1 = e.stats()
        nodes, depth = e.export_tree()
        e.step(1)
        pos, vel = e.download()[:2]
        st = e.stats()
    rise = SimpleNamespace(spills=s1.sort_spill_buckets - s0.sort_spill_buckets, reruns=s1.sort_rerun_buckets - s0.sort_rerun_buckets)
    return nodes, depth, pos, vel, st, snap, rise


def compare(monkeypatch, m, p, v, steps, direct="1", extra=None, path=None, k=None, why=None, lsd=True, **kw):
    """-> new, old: bh_stats of the run under test and of the counting run; snap, twin: the snapshot of the build under test
    and the twin's answer for its keys; rise, rise_old: what that build added to the spill and re-run counters in either run"""
    extra = extra or {}
    new = run(monkeypatch, dict(BH_SORT_BUCKET="2", BH_SORT_DIRECT=direct, **extra), m, p, v, steps, **kw)
    reorder = {k_: val for k_, val in extra.items() if k_ == "BH_REORDER_EVERY"}
    old = run(monkeypatch, dict(BH_SORT_BUCKET="2", BH_SORT_DIRECT="0", **reorder), m, p, v, steps, **kw)
    others = [old] + ([run(monkeypatch, dict(BH_SORT_BUCKET="0", **reorder), m, p, v, steps, **kw)] if lsd else [])
    for other in others:
        for x, y in zip(new[:4], other[:4]):
            if x.dtype.names:
                for f in x.dtype.names:
                    assert np.array_equal(x[f], y[f], equal_nan=True), f
            else:
                assert np.array_equal(x, y)
        assert not other[5].offered
    assert np.isfinite(new[2]).all() and np.isfinite(new[3]).all()
    twin = check_snapshot(new[5], path, k, why)
    # (the counting run's bucket sort writes the same plain keys and slots, whatever its splitters were)
    assert np.array_equal(old[5].keys_sorted, new[5].keys_sorted) and np.array_equal(old[5].perm, new[5].perm)
    return SimpleNamespace(new=new[4], old=old[4], snap=new[5], twin=twin, rise=new[6], rise_old=old[6])


def send(p, v, order, movers, targets, steps):
    """the bodies of the slots `movers` travel to just beside the bodies of the slots `targets` in `steps` steps (dt = 1)"""
    v = v.copy()
    for a, b in zip(movers, targets):
        v[order[a]] = f32((p[order[b]] + 1e-4 - p[order[a]]) / steps)
    return v


def send_each(p, v, order, movers, targets, steps=1, step=5e-5, grid=32):
    """send for many movers per target: the k-th visitor of a target lands (1 + k % grid, 1 + k // grid) * step beside it --
    every mover a landing point of its own (fp32 tells points 5e-5 apart from each other anywhere in the box), at most
    1.6e-3 from the target: inside its lattice cell for every n up to 40,000 (the jitter leaves 0.3 h >= 3e-3 to the edge)"""
    movers, targets = np.asarray(movers, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    assert len(movers) == len(targets) == len(set(movers.tolist()))
    by_target = np.argsort(targets, kind="stable")
    first = np.searchsorted(targets[by_target], targets[by_target], side="left")
    visit = np.empty(len(targets), dtype=np.int64)
    visit[by_target] = np.arange(len(targets)) - first
    assert visit.max(initial=0) < grid * grid
    land = p[order[targets]] + np.stack([1.0 + visit % grid, 1.0 + visit // grid], axis=1) * step
    v = v.copy()
    v[order[movers]] = f32((land - p[order[movers]]) / steps)
    return v


def off_starts(slots, L):
    """the slots, each moved on by one where it is a range start"""
    return [s + 1 if s % L == 0 else s for s in slots]
