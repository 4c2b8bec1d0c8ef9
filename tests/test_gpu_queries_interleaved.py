"""The six analysis families on ONE context, one after another: moment map, radial profile, Lagrangian radii, field at points,
neighbours, count_within, pair counts (auto and cross) and groups with a catalogue, then the same calls in reverse order.  They
share helpers, events and -- neighbours, pair counts, groups -- one search structure on the host side, so every result is held,
integer for integer and bit for bit, to the same call made alone on a fresh context with the same upload; the device buffers of
the first round serve the second; and the timing getters that share events keep their own call's times.

n = 257: one full workgroup and one body; the neighbour structure has more than one level and a leaf that is not full."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_nbody_simulation_amd as G  # noqa: E402

P = G.Precision
N, Q = 257, 65
BOX = (0.0, 1.0, -0.1, 0.9)
CENTRE, CENTRE_VEL = (0.47, 0.52), (0.01, -0.02)
EDGES = G.radial_edges(0.01, 0.8, 12)
FRACTIONS = (0.01, 0.1, 0.5, 0.5, 0.9, 1.0)
LINKING = 0.05


def bodies():
    rng = np.random.default_rng(257)
    return rng.random((N, 2)), rng.normal(0.0, 0.1, (N, 2)), rng.uniform(0.5, 1.5, N) * 1e-3


def points():
    return np.random.default_rng(65).uniform(-0.1, 1.1, (Q, 2))


def engine(precision):
    kw = {"max_depth": 21, "reference_compat": False} if precision == P.F32 else {}
    e = G.BarnesHutEngine(G.BhConfig(capacity=N, precision=precision, **kw))
    e.upload(*bodies())
    return e


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


CALLS = [
    ("moment_map", _moment_map),
    ("radial_profile", _radial_profile),
    ("lagrangian_radii", _lagrangian),
    ("field", lambda e: e.field(points(), with_counts=True)),
    ("neighbours", lambda e: e.neighbours(8, with_evals=True)),
    ("count_within", lambda e: (e.count_within(0.07),)),
    ("pair_counts", lambda e: e.pair_counts_raw(EDGES)),
    ("pair_counts_points", lambda e: e.pair_counts_raw(EDGES, points())),
    ("groups", _groups),
]


def frozen(result):
    """a call's result as (dtype, shape, bytes) per item: equal means bit for bit, NaN and the sign of zero included"""
    return tuple((a.dtype.str, a.shape, a.tobytes()) for a in (np.asarray(x) for x in result))


@functools.lru_cache(maxsize=None)
def alone(precision):
    """name -> the call's result on a context that makes no other call"""
    out = {}
    for name, call in CALLS:
        with engine(precision) as e:
            out[name] = frozen(call(e))
    return out


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_interleaved_calls_equal_the_calls_alone(precision):
    want = alone(precision)
    assert len(want["groups"][2][2]) > 0 and len(want["neighbours"][0][2]) == N * 8 * 8           # a catalogue; (n, 8) int64
    with engine(precision) as e:
        for name, call in CALLS:
            assert frozen(call(e)) == want[name], f"first round: {name}"
        after_first = e.stats().device_bytes
        for name, call in reversed(CALLS):
            assert frozen(call(e)) == want[name], f"second round, in reverse: {name}"
        assert e.stats().device_bytes == after_first                     # (nothing was allocated again)


@pytest.mark.parametrize("precision", [P.F64, P.F32], ids=lambda p: p.name)
def test_the_timing_getters_keep_their_own_call(precision):
    """neighbours and pair counts mark the same events around the structure's build and the searches; each call copies its times
    out at its end, so a pair count leaves the times of the last neighbours call alone"""
    with engine(precision) as e:
        assert e.neighbours_times() == (0.0, 0.0) and e.pair_counts_times() == (0.0, 0.0)
        e.neighbours(8)
        nb = e.neighbours_times()
        assert nb[0] > 0.0 and nb[1] > 0.0 and e.pair_counts_times() == (0.0, 0.0)
        e.pair_counts_raw(EDGES)
        assert e.neighbours_times() == nb
        auto = e.pair_counts_times()
        assert auto[0] > 0.0 and auto[1] > 0.0
        e.pair_counts_raw(EDGES, points())
        assert e.neighbours_times() == nb
        cross = e.pair_counts_times()
        assert cross[0] > 0.0 and cross[1] > 0.0
        e.groups(LINKING, 2)
        assert e.neighbours_times() == nb and e.pair_counts_times() == cross and all(t > 0.0 for t in e.groups_times())
