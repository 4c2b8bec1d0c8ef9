"""Model-based call sequences over the whole single-GPU API: seeded sequences of movers, diagnostics and
readers run on ONE context and are held, bit for bit, to three oracles that share no code with the engine -- a helper of
tests/test_gpu_sequences.py and tests/test_sequence_cpu.py, not a test file and not a conftest.

Operations.  MOVERS may change the run (upload, step, step_kdk, build_tree, compute_forces, kick, drift, set_softening); WALK
observers build a quiet tree (potential, energy, field, force_error, force_check); FREE observers read the state only (direct sum,
moment map, radial profile, Lagrangian radii, neighbours, radius counts, pair counts, groups, spanning tree, binaries); READERS
copy something out.  An operation is a record of its name, its arguments and a callable on a BarnesHutEngine.

The twin (Twin) is the model: six facts, one method per mover that applies the rows of section 18's table, one predicate that says
which return code a call must give.  The runner (run) executes a sequence on a SUBJECT (every operation), a CONTROL (the movers
only) and WITNESSES (fresh per occurrence: the movers so far, then that single call), and asserts

1. refusals: every return code is the twin's; a refused mover is refused by the control too, and the state is unchanged after it;
2. non-perturbation: after every mover download(), masses(), forces() where current, the KEPT fields of stats() and n_nodes (see
   run) are those of the control;
3. a walk observer's result is the witness's: it does not depend on the diagnostics before it;
4. a free observer's result is that of the same call on a fresh context that has only uploaded the subject's downloaded state;
   direct_forces also equals tests/direct_ref.py on that state;
5. nothing is skipped: compared operations + observed refusals == the sequence's length.

A call that fails with anything but BH_ERR_ARG or BH_ERR_STATE -- a device error -- ends the whole pytest session at once
(execute: pytest.exit), on purpose: after a fault nothing more is to be started on a GPU that others share.

Body sets, all quasi-static and of float32 values, in contexts of capacity 4,353: A the 4,353 Plummer bodies of tests/quiet_case.py
(above one sort bucket: LSD passes first, the splitter path after), B 1,000 uniform bodies, C 257 uniform bodies of which 5 and 200
coincide (equal keys, a depth-cap leaf, non-finite terms in the fp64 field and the direct sum).  The fp64 trees take C with body
200 at 2^-20 beside body 5 instead of on it: their force walks, like the reference's, divide by the distance to a coincident body,
so the first step makes the state itself non-finite, the position queries then refuse it (BH_ERR_ARG) and every comparison
after it compares NaN with NaN.  The close pair still shares its cell down to the depth cap, the 65th field point still lies on
body 5 (non-finite in the fp64 field), and F32 and MIXED, whose walks skip a coincident body, keep the exact pair."""
import dataclasses
import functools
import itertools
import os

import numpy as np
import pytest

import gpu_nbody_simulation_amd as G
from gpu_nbody_simulation_amd import initial_conditions as IC
from quiet_case import KEPT

P = G.Precision
PRECISIONS = (P.F64_EXACT, P.F32, P.MIXED, P.F64)
CAPACITY = 4353
DT = 1.0                                   # BhConfig.dt
OK, ERR_ARG, ERR_STATE = 0, -1, -5         # BH_OK, BH_ERR_ARG, BH_ERR_STATE (include/bhgpu.h)
SEQ_LEN = 30
N_RANDOM = 6

SETS = ("A", "B", "C")
BOX = (-0.1, 0.1, -0.08, 0.12)
CENTRE, CENTRE_VEL = (0.003, -0.002), (1e-10, -2e-10)
EDGES = G.radial_edges(0.001, 0.15, 12)
FRACTIONS = (0.01, 0.1, 0.5, 0.5, 0.9, 1.0)
LINKING, RADIUS, MAX_SEPARATION = 0.006, 0.01, 0.01
TARGETS = np.array([0, 5, 200, 256, 31, 5], dtype=np.int64)     # (below 257; the coincident pair of C; one index twice)
ETA, LENGTH = 0.1, 0.05


@functools.lru_cache(maxsize=None)
def bodies(name, coincide=True):
    """(masses, positions, velocities) of set A, B or C, read-only; coincide = False: C's pair 2^-20 apart (module docstring)"""
    if name == "A":
        m, p, v = IC.make("plummer", CAPACITY, 4, quasi_static=True)        # quiet_case.bodies()
    elif name == "B":
        m, p, v = IC.make("uniform", 1000, 11, quasi_static=True)
    else:
        m, p, v = IC.make("uniform", 257, 12, quasi_static=True)
        p[200], v[200] = p[5], v[5]
        if not coincide:
            p[200, 0] = np.float32(p[5, 0] + 2.0 ** -20)
    for a in (m, p, v):
        a.setflags(write=False)
    return m, p, v


@functools.lru_cache(maxsize=None)
def points():
    """65 points: 64 in the box of B and C (inside A's sphere as well) and the place of C's coincident pair"""
    q = np.random.default_rng(65).uniform(-0.12, 0.12, (64, 2))
    q = np.concatenate([q, bodies("C")[1][5:6]])
    q.setflags(write=False)
    return q


# ---- operations ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Op:
    name: str
    args: tuple
    call: object = dataclasses.field(compare=False, repr=False)

    def __str__(self):
        return f"{self.name}({', '.join(repr(a) for a in self.args)})"


def _upload(e, name):
    m, p, v = bodies(name, e.cfg.precision in (P.F32, P.MIXED))
    e.upload(p, v, m)


def _moment_map(e):
    m = e.moment_map(BOX, 7, 5, "cic", raw=True)
    return m.planes, m.exponents, m.n_deposited


def _radial_profile(e):
    p = e.radial_profile(EDGES, CENTRE, CENTRE_VEL, raw=True)
    return p.planes, p.exponents


def _lagrangian(e):
    r = e.lagrangian_radii(FRACTIONS, CENTRE)
    return r.r2, r.count, r.mass_units, r.exponent


def _groups(e):
    g = e.groups(LINKING, 2, raw=True)
    return g.label, g.n_groups, g.id, g.count, g.sums, g.exponents


def _spanning_tree(e):
    t = e.spanning_tree()
    return t.lo, t.hi, t.d2


def _binaries(e):
    b = e.binaries(MAX_SEPARATION)
    return (b.partner, b.eps) + tuple(getattr(b, f) for f in G.engine.BINARIES_COLUMNS)


def _energy(e):
    x = e.energy()
    return x.kinetic, x.potential, x.total, x.momentum, x.angular_momentum, x.com, x.mass, x.n_bodies


def _timestep(e, eta, length):
    t = e.timestep(eta, length)
    return t.dt, t.a_max, t.worst, t.n_bodies


def _stats(e):
    s = e.stats()
    return tuple(getattr(s, k) for k in KEPT) + (s.n_bodies,)


def _sort_snapshot(e):
    """the sort's output only: the decision words and crosser lists describe how far the bodies moved since the build before, and
    after a diagnostic that is the quiet build (section 18, kept as they are: perm and keys_sorted are the quiet build's)"""
    s = e.sort_snapshot()
    return s.n, s.keys_sorted, s.perm


def _export_tree(e):
    nodes, depth = e.export_tree()
    return nodes.view(np.uint8), depth


MOVERS = {
    "upload": ([(s,) for s in SETS], lambda e, s: _upload(e, s)),
    "step": ([(1,), (2,), (3,)], lambda e, k: e.step(k)),
    "step_kdk": ([(1,), (2,), (0,)], lambda e, k: e.step_kdk(k)),
    "build_tree": ([()], lambda e: e.build_tree()),
    "compute_forces": ([()], lambda e: (e.compute_forces(),)),
    "kick": ([(DT,), (DT / 2,), (0.0,)], lambda e, h: e.kick(h)),
    "drift": ([(DT,), (DT / 2,), (0.0,)], lambda e, h: e.drift(h)),
    "set_softening": ([(1e-3,), (1e-3,), (0.0,), (0.0,)], lambda e, eps: e.set_softening(eps)),
}
WALK = {
    "potential": ([()], lambda e: e.potential(with_counts=True)),
    "energy": ([()], _energy),
    "field": ([()], lambda e: e.field(points(), with_counts=True)),
    "force_error": ([()], lambda e: dataclasses.astuple(e.force_error(sample=64))),
    "force_check": ([()], lambda e: e.force_check(TARGETS)),
}
FREE = {
    "direct_forces": ([()], lambda e: (e.direct_forces(np.arange(8)),)),
    "moment_map": ([()], _moment_map),
    "radial_profile": ([()], _radial_profile),
    "lagrangian_radii": ([()], _lagrangian),
    "neighbours": ([()], lambda e: e.neighbours(8)),
    "count_within": ([()], lambda e: (e.count_within(RADIUS),)),
    "pair_counts": ([()], lambda e: (e.pair_counts_raw(EDGES)[0],)),
    "pair_counts_points": ([()], lambda e: (e.pair_counts_raw(EDGES, points())[0],)),
    "groups": ([()], _groups),
    "spanning_tree": ([()], _spanning_tree),
    "binaries": ([()], _binaries),
}
READERS = {
    "download": ([()], lambda e: e.download()),
    "masses": ([()], lambda e: (e.masses(),)),
    "forces": ([()], lambda e: (e.forces(),)),
    "accelerations": ([()], lambda e: (e.accelerations(),)),
    "export_tree": ([()], _export_tree),
    "timestep": ([(ETA, LENGTH), (ETA, None)], _timestep),
    "stats": ([()], _stats),
    "sort_snapshot": ([()], _sort_snapshot),
    "sync": ([()], lambda e: e.sync()),
}
TABLES = {"mover": MOVERS, "walk": WALK, "free": FREE, "reader": READERS}
KIND = {name: kind for kind, table in TABLES.items() for name in table}
OBSERVERS = tuple(WALK) + tuple(FREE)
REFUSABLE = ("kick", "timestep", "export_tree", "sort_snapshot")      # what the twin can refuse once a body set is there


def op(name, *args):
    call = TABLES[KIND[name]][name][1]
    return Op(name, tuple(args), lambda e: call(e, *args))


def mover_kinds(precision):
    """F64_EXACT refuses every softening but 0: it has no set_softening in these sequences"""
    return tuple(k for k in MOVERS if not (k == "set_softening" and precision == P.F64_EXACT))


def pool(precision):
    """every operation with every argument it takes here"""
    names = mover_kinds(precision) + tuple(WALK) + tuple(FREE) + tuple(READERS)
    return [op(n, *a) for n in names for a in dict.fromkeys(TABLES[KIND[n]][n][0])]


def frozen(result):
    """a call's result as (dtype, shape, bytes) per item: equal means bit for bit, NaN and the sign of zero included
    (test_gpu_queries_interleaved.frozen)"""
    if result is None:
        return ()
    return tuple((a.dtype.str, a.shape, a.tobytes()) for a in (np.asarray(x) for x in result))


# ---- the twin -----------------------------------------------------------------------------------------------------------
class Twin:
    """What bh_run_state.hpp holds of a single-GPU context with n > 0 bodies, as far as a return code depends on it."""

    def __init__(self, precision):
        self.fp32_tree, self.exact = precision in (P.F32, P.MIXED), precision == P.F64_EXACT
        self.uploaded = self.tree_valid = self.forces_current = self.phi_current = False
        self.n, self.softening, self.set = 0, 0.0, None

    def flags(self):
        return tuple(int(x) for x in (self.uploaded, self.tree_valid, self.forces_current, self.phi_current))

    def builds(self, o):
        """this call completes a build (build_completed: tree_valid set)"""
        n, k = o.name, o.args[0] if o.args else None
        return (n in ("step", "step_kdk") and k > 0) or n in ("build_tree", "compute_forces", "potential", "field", "force_error",
                                                              "force_check") or (n == "energy" and not self.phi_current)

    def predict(self, o):
        n = o.name
        if n == "set_softening":
            return ERR_ARG if self.exact and o.args[0] != 0.0 else OK               # bh_engine.hip:1119
        if n in ("upload", "stats", "sync", "forces", "accelerations"):
            return OK                                  # bh_engine.hip:1148, 1840, 1231, 1485, 1491: no state is asked for
        if n in ("export_tree", "sort_snapshot"):
            # (1908 also asks for sort_rec.valid: every build sets it, and only a build sets tree_valid, so the twin needs no
            # fact of its own for it)
            return OK if self.tree_valid else ERR_STATE                              # bh_engine.hip:1711, 1908
        if not self.uploaded:
            return ERR_STATE      # need_upload, bh_engine.hip:866 (movers 1245-1315, split_check 1328, diag_check 876;
                                  # bh_queries_host.hpp:138, 281, 485, 712)
        if n == "timestep" and o.args[1] is None and not self.softening > 0.0:
            return ERR_ARG                                                           # bh_engine.hip:1412-1414, before need_forces
        if n in ("kick", "timestep"):
            return OK if self.forces_current else ERR_STATE                          # need_forces, bh_engine.hip:1392, 1415
        return OK

    def apply(self, o):
        """an accepted call; section 18's rows"""
        n, k = o.name, o.args[0] if o.args else None
        if self.builds(o):
            self.tree_valid = True                                                   # build_completed
        if n == "upload":                                                            # new_bodies
            self.uploaded, self.tree_valid, self.forces_current, self.phi_current = True, False, False, False
            self.set, self.n = k, len(bodies(k)[0])
        elif n == "step":                                                            # positions_moved_by_walk
            self.forces_current = self.phi_current = False
        elif n == "step_kdk" and k > 0:                                              # positions_moved_by_drift, forces_computed
            self.phi_current, self.forces_current = False, True
        elif n == "build_tree":                                                      # forces_outdated
            self.forces_current = False
        elif n == "compute_forces":                                                  # forces_computed
            self.forces_current = True
        elif n == "drift":                                                           # positions_moved_by_drift, whatever h
            self.tree_valid = self.forces_current = self.phi_current = False
        elif n == "set_softening":                                                   # law_changed(value_changed)
            self.forces_current = self.forces_current and k == self.softening
            self.phi_current, self.softening = False, k
        elif n in ("potential", "energy"):                                           # potential_computed
            self.phi_current = True


# ---- op -> the events it fires (section 18, "where it fires"), for tests/run_state_events.cpp ------------------------------
def _build(t):
    return [f"build_completed {t.n} 0"]


def _walk(t, integrate):
    return (["walk_begins 0"] + (["positions_moved_by_walk 1"] if integrate else []) + ["walk_launched"] +
            (["group_costs_written"] if t.fp32_tree else []))


def _quiet(events):
    return ["quiet_begin"] + events + ["quiet_end"]


def _kdk(o, t):
    k = o.args[0]
    if k == 0:
        return []
    first = [] if t.forces_current else _build(t) + _walk(t, False)
    steps = [e for s in range(k) for e in _build(t) + _walk(t, s < k - 1)]
    return first + ["positions_moved_by_drift"] + steps + ["forces_computed 1"]


def _potential(o, t):
    return _quiet(_build(t)) + ["potential_computed 1"]


EVENTS = {
    "upload": lambda o, t: ["new_bodies"],
    "step": lambda o, t: (_build(t) + _walk(t, True)) * o.args[0],
    "step_kdk": _kdk,
    "build_tree": lambda o, t: ["forces_outdated"] + _build(t),
    "compute_forces": lambda o, t: _build(t) + _walk(t, False) + ["forces_computed 1"],
    "drift": lambda o, t: ["positions_moved_by_drift"],
    "set_softening": lambda o, t: [f"law_changed {int(o.args[0] != t.softening)}"],
    "potential": _potential,
    "energy": lambda o, t: [] if t.phi_current else _potential(o, t),
    "field": lambda o, t: _quiet(_build(t)),
    "force_error": lambda o, t: _quiet(_build(t) + _walk(t, False)),
    "force_check": lambda o, t: _quiet(_build(t) + _walk(t, False)),
    "export_tree": lambda o, t: ["all_node_records_written"] if t.fp32_tree else [],
}


def events(o, twin):
    """the events of bh_run_state.hpp this call fires on a context in the twin's state (before the call); none when refused"""
    if twin.predict(o) != OK:
        return []
    return EVENTS.get(o.name, lambda o, t: [])(o, twin)


# ---- sequences ----------------------------------------------------------------------------------------------------------
class _Args:
    """the next argument tuple of every mover kind, in turn; an upload never repeats the set that is there"""
    UPLOADS = ("B", "C", "A", "C", "B", "A")           # from A: every set after every other set

    def __init__(self):
        self.it = {k: itertools.cycle(v[0]) for k, v in MOVERS.items() if k != "upload"}
        self.up = itertools.cycle(self.UPLOADS)

    def mover(self, kind, twin):
        if kind != "upload":
            return op(kind, *next(self.it[kind]))
        s = next(self.up)
        while s == twin.set:
            s = next(self.up)
        return op("upload", s)


def _blocks(precision, args):
    """the pair-coverage blocks, each a function of the twin at its start (an upload looks at the set that is there)"""
    kinds = mover_kinds(precision)

    def pair(kind, obs):
        return lambda t: ([op("compute_forces")] if kind == "kick" else []) + [args.mover(kind, t), op(obs), op("step", 1)]

    def then_step(kind):
        return lambda t: ([op("compute_forces")] if kind == "kick" else []) + [args.mover(kind, t), op("step", 1)]

    out = [pair(k, o) for k in kinds for o in OBSERVERS]
    out += [then_step(k) for k in kinds]
    # every observer directly after another one; the second half first, so that each is also a second
    out.append(lambda t: [op(o) for o in OBSERVERS] + [op(OBSERVERS[0]), op("step", 1)])
    # a leapfrog step by hand with a diagnostic in every gap: after the forces, between kick and drift, after the drift (in
    # front of the closing walk), after the closing forces
    for a, b, c, d in (("potential", "field", "force_check", "energy"), ("force_error", "groups", "potential", "neighbours"),
                       ("field", "force_check", "energy", "force_error")):
        out.append(lambda t, a=a, b=b, c=c, d=d: [op("compute_forces"), op(a), op("kick", DT / 2), op(b), op("drift", DT), op(c),
                                                 op("compute_forces"), op(d), op("kick", DT / 2), op("step", 1)])
    # every reader where it is accepted, and every refusable call where it is refused: right after an upload
    out.append(lambda t: [op("step", 1), op("download"), op("masses"), op("forces"), op("accelerations"), op("export_tree"),
                          op("sort_snapshot"), op("stats"), op("sync"), op("potential"), op("export_tree"), op("sort_snapshot"),
                          op("compute_forces"), op("timestep", ETA, LENGTH), op("stats"), op("step", 1)])
    out.append(lambda t: [args.mover("upload", t), op("kick", DT), op("timestep", ETA, LENGTH), op("timestep", ETA, None),
                          op("export_tree"), op("sort_snapshot"), op("drift", DT / 2), op("potential"), op("export_tree"),
                          op("kick", DT / 2), op("step", 1)])
    return out


def _advance(twin, ops):
    for o in ops:
        if twin.predict(o) == OK:
            twin.apply(o)


@functools.lru_cache(maxsize=None)
def pair_sequences(precision):
    """the pair-coverage sequences of a precision: at most SEQ_LEN operations each, every one starting with upload(A)"""
    args = _Args()
    seqs, cur, twin = [], None, None
    for block in _blocks(precision, args):
        if cur is None:
            cur, twin = [op("upload", "A")], Twin(precision)
            _advance(twin, cur)
        ops = block(twin)
        if len(cur) + len(ops) > SEQ_LEN:
            seqs.append(tuple(cur))
            cur, twin = [op("upload", "A")], Twin(precision)
            _advance(twin, cur)
            if any(o == op("upload", "A") for o in ops):                         # (A is there again: the next set in turn)
                ops = block(twin)
        cur += ops
        _advance(twin, ops)
    seqs.append(tuple(cur))
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def random_sequence(precision, index):
    """SEQ_LEN operations from numpy.random.default_rng((precision, index)): a mover with probability 0.4, a call the twin refuses
    with probability 0.1, at least one upload of another set, and step(2); download() at the end"""
    rng = np.random.default_rng((int(precision), int(index)))
    everything = pool(precision)
    twin = Twin(precision)
    seq = [op("upload", "A")]
    _advance(twin, seq)
    must_upload_at = int(rng.integers(5, 21))
    while len(seq) < SEQ_LEN - 2:
        refused = [o for o in everything if twin.predict(o) != OK]
        legal = [o for o in everything if twin.predict(o) == OK]
        reupload = [o for o in legal if o.name == "upload" and o.args[0] != twin.set]
        if len(seq) == must_upload_at and not any(o.name == "upload" for o in seq[1:]):
            o = reupload[int(rng.integers(len(reupload)))]
        elif rng.random() < 0.1 and refused:
            o = refused[int(rng.integers(len(refused)))]
        else:
            want_mover = rng.random() < 0.4
            some = [o for o in legal if (KIND[o.name] == "mover") == want_mover]
            o = some[int(rng.integers(len(some)))]
        seq.append(o)
        _advance(twin, [o])
    return tuple(seq + [op("step", 2), op("download")])


def sequences(precision):
    """(id, sequence) of every committed sequence of a precision"""
    out = [(f"pair{i}", s) for i, s in enumerate(pair_sequences(precision))]
    return out + [(f"random{i}", random_sequence(precision, i)) for i in range(N_RANDOM)]


# ---- the runner ---------------------------------------------------------------------------------------------------------
def execute(e, o):
    """(return code, frozen result) of one call"""
    try:
        return OK, frozen(o.call(e))
    except G.BhError as err:
        if err.code not in (ERR_ARG, ERR_STATE):                 # a device error: nothing more is started on this GPU
            pytest.exit(f"{o}: {err}", returncode=3)
        return err.code, None


def _engine(precision, n_threads, flags=0):
    return G.BarnesHutEngine(G.BhConfig(capacity=CAPACITY, precision=precision, n_threads=n_threads, flags=flags))


WALK_STATS = G.engine.FLAG_WALK_STATS
COUNTERS = tuple(KEPT.index(k) for k in ("visits", "interactions", "wave_nodes", "wave_quads", "wave_accepts"))


def _stats_differ(mine, theirs, both_trees, zeroed):
    """the first field of the frozen KEPT + n_bodies tuples that differs where it is promised equal, or None.  build_bytes,
    walk_launches, steps_done and n_bodies always are.  The five walk counters (counted under BH_FLAG_WALK_STATS only) are
    compared where both contexts report them -- bh_stats reads them as zero without tree_valid, and "a quiet build leaves
    tree_valid ... as the quiet build made [it]" (section 18, kept as they are), so after drift; field the subject reports the
    last walk's counters and the control zeros -- and where no potential has been computed since the last real build:
    "bh_stats after a potential on a BH_FLAG_WALK_STATS context reads zero walk counters (the potential's scope keeps none)"
    (the same list); there the subject's must BE zero."""
    for k, name in enumerate(KEPT + ("n_bodies",)):
        if k in COUNTERS and zeroed:
            if both_trees and int(np.frombuffer(mine[k][2], dtype=mine[k][0])[0]) != 0:
                return name + " (not zero after a potential)"
        elif (k not in COUNTERS or both_trees) and mine[k] != theirs[k]:
            return name
    return None


def _state(e):
    """what oracle 2 compares after a mover, frozen"""
    s = e.stats()
    return {"download": frozen(e.download()), "masses": frozen((e.masses(),)), "stats": frozen(tuple(getattr(s, k) for k in KEPT) + (s.n_bodies,)),
            "forces": frozen((e.forces(),)), "accelerations": frozen((e.accelerations(),)), "n_nodes": s.n_nodes}


def _direct_reference(pos, mass, softening):
    from direct_ref import direct_ref
    from soft_ref import soft_direct_ref
    t = np.arange(8)
    return direct_ref(pos, mass, t) if softening == 0.0 else soft_direct_ref(pos, mass, t, eps=softening)


def run(precision, sequence, env, n_threads, flags=0, log=print):
    """Runs one sequence against the three oracles (module docstring); returns (compared, refused).  `env` is what the caller has
    put into the environment (the contexts read it when they are created); `flags` are every context's BhConfig.flags."""
    from direct_ref import same_bits
    for k, v in env.items():
        assert os.environ.get(k) == str(v), f"{k} is not set"
    names = [str(o) for o in sequence]

    def where(i):
        return f"operation {i}, {names[i]}, after {names[:i]}"

    def witness(i, also=None):
        """a fresh context: the movers before i (and the call at `also`), then call i"""
        with _engine(precision, n_threads, flags) as w:
            for j, o in enumerate(sequence[:i]):
                if KIND[o.name] == "mover" or j == also:
                    execute(w, o)
            return execute(w, sequence[i])

    compared = refused = 0
    with _engine(precision, n_threads, flags) as subject, _engine(precision, n_threads, flags) as control:
        twin, ctwin = Twin(precision), Twin(precision)
        cache = None                # the control's state after its last mover
        quiet_tree = None           # the diagnostic whose quiet build made the tree in the subject's buffers, if one did
        zeroed = False              # a potential's quiet build has cleared the walk counters since the last real build
        for i, o in enumerate(sequence):
            kind, want = KIND[o.name], twin.predict(o)
            building = want == OK and twin.builds(o)
            code, got = execute(subject, o)
            assert code == want, f"oracle 1: return code {code}, the twin says {want}: {where(i)}"
            if want != OK:
                if kind == "mover":
                    assert execute(control, o)[0] == want, f"oracle 1: the control accepts what the subject refused: {where(i)}"
                if cache is not None:
                    assert frozen(subject.download()) == cache["download"], f"oracle 1: a refused call changed the state: {where(i)}"
                refused += 1
                continue
            twin.apply(o)
            if kind == "mover":
                assert execute(control, o)[0] == OK, f"the control refuses: {where(i)}"
                ctwin.apply(o)
                assert ctwin.flags()[0::2] == twin.flags()[0::2]
                if building or not twin.tree_valid:
                    quiet_tree = None
                if building:
                    zeroed = False
                cache, mine = _state(control), _state(subject)
                for k in ("download", "masses"):
                    assert mine[k] == cache[k], f"oracle 2: {k} differs from the control's: {where(i)}"
                bad = _stats_differ(mine["stats"], cache["stats"], twin.tree_valid and ctwin.tree_valid, zeroed)
                assert bad is None, f"oracle 2: stats().{bad} differs from the control's: {where(i)}"
                if twin.forces_current:
                    assert mine["forces"] == cache["forces"], f"oracle 2: forces differ from the control's: {where(i)}"
                # n_nodes is the count of the build that is in the buffers, and "a quiet build leaves tree_valid, aux_full, perm
                # and keys_sorted as the quiet build made them" (section 18, kept as they are): after a diagnostic the subject
                # reports the quiet build's count, of positions the control's last build may not have seen.  Compared where the
                # last build of both is the same real one.
                if twin.tree_valid and ctwin.tree_valid and quiet_tree is None:
                    assert mine["n_nodes"] == cache["n_nodes"], f"oracle 2: n_nodes differs from the control's: {where(i)}"
            elif kind == "walk":
                if building:
                    quiet_tree = i
                    zeroed = zeroed or o.name in ("potential", "energy")
                assert (OK, got) == witness(i), f"oracle 3: the result depends on the diagnostics before it: {where(i)}"
            elif kind == "free":
                (x, v), m = subject.download(), subject.masses()
                with _engine(precision, n_threads, flags) as fresh:
                    fresh.upload(x, v, m)
                    if twin.softening != 0.0:
                        fresh.set_softening(twin.softening)
                    assert (OK, got) == execute(fresh, o), f"oracle 4: not the answer of a fresh context on this state: {where(i)}"
                if o.name == "direct_forces":
                    mine = np.frombuffer(got[0][2]).reshape(got[0][1])
                    assert same_bits(mine, _direct_reference(x, m, twin.softening)), f"oracle 4: not the direct sum: {where(i)}"
            elif o.name in ("download", "masses", "forces", "accelerations"):
                assert got == cache[o.name], f"reader: {o.name} is not the control's: {where(i)}"
            elif o.name == "stats":
                bad = _stats_differ(got, cache["stats"], twin.tree_valid and ctwin.tree_valid, zeroed)
                assert bad is None, f"reader: stats().{bad} is not the control's: {where(i)}"
            elif o.name == "sync":
                assert got == ()
            else:
                # timestep reads the force buffer, export_tree and sort_snapshot the tree in the buffers: that of the last real build,
                # or of the one diagnostic whose quiet build came after it
                assert o.name in ("timestep", "export_tree", "sort_snapshot")
                assert (OK, got) == witness(i, quiet_tree), f"reader: {o.name} depends on the diagnostics before it: {where(i)}"
            compared += 1
    log(f"{precision.name}: {len(sequence)} operations, {compared} compared, {refused} refused as predicted")
    assert compared + refused == len(sequence), "oracle 5: an operation was neither compared nor refused"
    return compared, refused
