"""BarnesHutEngine: the Python face of one bh_ctx (include/bhgpu.h).

Mirrors what runSimulationGpu (project.cu:918-1024) does with its device buffers, with the
reference's compile-time constants (project.cu:1-11, 27-35, 60-62) as a runtime BhConfig.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import os
from dataclasses import dataclass, field, replace
from typing import NamedTuple

import numpy as np

from . import _lib

TREE_NODE_DTYPE = np.dtype(
    [("child", "<f8", (4,)), ("comx", "<f8"), ("comy", "<f8"), ("mass", "<f8"), ("xmin", "<f8"),
     ("xmax", "<f8"), ("ymin", "<f8"), ("ymax", "<f8"), ("particle", "<f8")])

FLAG_WALK_STATS = 1 << 0
FLAG_LDS_STACK = 1 << 1
FLAG_WALK_NO_SPLIT = 1 << 2
FLAG_WALK_PORTABLE = 1 << 3


class Precision(enum.IntEnum):
    F64_EXACT = 0   # bit-identical to the reference CPU path
    F32 = 1         # throughput mode (BASELINE configs "fp32")
    MIXED = 2       # fp64 state, fp32 forces (BASELINE config "fp64 positions / fp32 forces")
    F64 = 3         # fp64 throughout at throughput: the exact mode's tree, a free-order rsqrt walk (<= 1e-12 of the oracle)


class BhError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bhgpu error {code}: {msg}")
        self.code = code


@dataclass
class BhConfig:
    capacity: int
    theta: float = 0.5              # THETA, project.cu:60
    G: float = 6.67e-11             # project.cu:27
    dt: float = 1.0                 # DELTA_T, project.cu:29
    max_depth: int = 10             # QUADTREE_MAX_DEPTH, project.cu:61
    precision: Precision = Precision.F64_EXACT
    reference_compat: bool = True
    device: int = 0
    n_threads: int = 0              # N_THREADS, project.cu:5-7: bodies walked at a time (passes of whole workgroups); 0 = all
    flags: int = 0
    node_capacity: int = 0
    softening: float = 0.0          # Plummer softening length (bh_set_softening); 0: the reference's unsoftened law.  Not a
                                    # field of the C struct: applied through the setter once the context exists


@dataclass
class BhStats:
    n_bodies: int
    n_nodes: int
    n_internal: int
    steps_done: int
    visits: int
    interactions: int
    wave_nodes: int
    last_step_ms: float
    build_ms: float
    walk_ms: float
    device_bytes: int
    keys_ms: float = 0.0        # per kernel group of the last timed step
    sort_ms: float = 0.0
    scan_ms: float = 0.0
    nodes_ms: float = 0.0
    build_bytes: int = 0        # algorithmic bytes of that step
    walk_bytes: int = 0
    wave_quads: int = 0         # FLAG_WALK_STATS: quads loaded, once per wavefront
    sort_spill_buckets: int = 0  # bucket-sort buckets sorted through memory since creation (0 in steady motion)
    let_tree_ms: float = 0.0    # last let_build: global box + local tree
    let_pack_ms: float = 0.0    # last let_build: LET marking / numbering / packing
    sort_rerun_buckets: int = 0  # bucket-sort buckets whose short sort met a long run and was repeated in full (bh_sort.hpp)
    wave_accepts: int = 0       # FLAG_WALK_STATS, fp64 precisions: nodes some lane took a term from, once per wavefront
    walk_launches: int = 0      # walk kernel launches of the last step (1, or the passes of n_threads)


@dataclass
class BhEnergy:
    """bh_energy_t: energy, momentum and angular momentum of the current state (fp64 device reductions)."""
    kinetic: float               # 1/2 sum m |v|^2
    potential: float             # 1/2 sum m_i phi_i, over the force walk's terms
    total: float
    momentum: tuple              # (px, py) = sum m v
    angular_momentum: float      # sum m (x vy - y vx), about the origin
    com: tuple                   # centre of mass
    mass: float
    n_bodies: int


@dataclass
class BhTimestep:
    """bh_timestep_t: the criterion dt = eta * sqrt(length / a_max) over the accelerations of the last compute_forces()."""
    dt: float
    a_max: float                 # the largest |a| (inf when some acceleration is not finite; dt is 0 then)
    worst: int                   # caller index of the body that has it (-1: no bodies)
    n_bodies: int


@dataclass
class BhForceError:
    """Relative Barnes-Hut force error rel_i = |F_tree - F_dir| / |F_dir| over a set of bodies (force_error_stats)."""
    n: int                       # bodies in the statistics
    n_zero: int                  # excluded: |F_dir| == 0 (finite forces)
    n_nonfinite: int             # excluded: a non-finite component in F_tree or F_dir
    median: float                # order statistics: the sorted value at index ceil(q n) - 1
    p90: float
    p99: float
    p999: float
    max: float
    worst: int                   # caller index of the body with the largest error (-1: none)
    rms: float                   # RMS |F_tree - F_dir| / RMS |F_dir|


MAP_SCHEMES = {"ngp": 0, "cic": 1}      # BH_MAP_NGP, BH_MAP_CIC
MAP_MAX_CELLS = 1 << 24                 # BH_MAP_MAX_CELLS


@dataclass
class BhMomentMap:
    """Moment maps of the current state on nx x ny cells over box (moment_map): fp64 arrays (ny, nx), y the outer axis.
    mass, px, py, k2 are the fixed-point sums times 2^-exponent (sums beyond 2^53 units round to fp64 there; the scaling
    itself is exact); the others are derived from them, NaN in a cell without mass except sigma, which is 0 there."""
    mass: np.ndarray             # sum m
    px: np.ndarray               # sum m vx
    py: np.ndarray               # sum m vy
    k2: np.ndarray               # sum m (vx^2 + vy^2)
    sigma: np.ndarray            # surface density: mass / cell area
    vx: np.ndarray               # mass-weighted mean velocity: px / mass
    vy: np.ndarray
    dispersion: np.ndarray       # sqrt(max(k2 / mass - vx^2 - vy^2, 0))
    box: tuple                   # (xmin, xmax, ymin, ymax)
    scheme: str                  # "ngp" or "cic"
    n_deposited: int             # bodies with at least one corner inside the grid
    planes: np.ndarray | None = None      # raw=True: the int64 sums (4, ny, nx) ...
    exponents: np.ndarray | None = None   # ... and their exponents: value = planes * 2^-exponent


def fixed_point_exponents(maxabs, n_total: int) -> np.ndarray:
    """The rule of every binned sum: the exponents 62 - E_p - L of int64 planes from their maxima max |q_p| (combined over the
    ranks with MAX) and the body count of the whole system: max < 2^E_p, L = ceil(log2(max(n, 1))); 0 where the maximum is 0."""
    m = np.asarray(maxabs, dtype=np.float64).reshape(-1)
    L = 0 if n_total <= 1 else (int(n_total) - 1).bit_length()
    _, E = np.frexp(m)
    return np.where(m == 0.0, 0, 62 - E - L).astype(np.int32)


def _scaled(planes, exponents, count: int) -> list:
    """The first `count` int64 planes times 2^-exponent, in fp64."""
    return [np.ldexp(planes[p].astype(np.float64), -int(exponents[p])) for p in range(count)]


def _raw(planes, exponents, raw: bool):
    """What a result keeps of its sums: (planes, a copy of the exponents as int32) when raw, else (None, None)."""
    return (planes, np.asarray(exponents, dtype=np.int32).copy()) if raw else (None, None)


def moment_exponents(maxabs, n_total: int) -> np.ndarray:
    """The four exponents of a moment map (fixed_point_exponents) from the maxima of bh_moment_map_max."""
    return fixed_point_exponents(np.asarray(maxabs, dtype=np.float64).reshape(4), n_total)


def moment_map_from_planes(planes, exponents, box, scheme: str, n_deposited: int, raw: bool = False) -> BhMomentMap:
    """BhMomentMap of the int64 sums (4, ny, nx) and their exponents."""
    planes = np.asarray(planes, dtype=np.int64)
    _, ny, nx = planes.shape
    box = tuple(float(b) for b in box)
    mass, px, py, k2 = _scaled(planes, exponents, 4)
    area = ((box[1] - box[0]) / nx) * ((box[3] - box[2]) / ny)
    with np.errstate(divide="ignore", invalid="ignore"):
        vx, vy = px / mass, py / mass
        disp = np.sqrt(np.maximum(k2 / mass - vx * vx - vy * vy, 0.0))
    empty = mass == 0.0
    for a in (vx, vy, disp):
        a[empty] = np.nan
    return BhMomentMap(mass, px, py, k2, mass / area, vx, vy, disp, box, scheme, int(n_deposited), *_raw(planes, exponents, raw))


RADIAL_MAX_BINS = 4096                  # BH_RADIAL_MAX_BINS
RADIAL_MAX_FRACTIONS = 32               # BH_RADIAL_MAX_FRACTIONS
RADIAL_DIGIT_BITS = 8                   # BH_RADIAL_DIGIT_BITS


@dataclass
class BhRadialProfile:
    """Radial profile of the current state about a centre on the nb bins between edges (radial_profile): fp64 arrays (nb,)
    unless said otherwise.  mass and the enclosed masses are the fixed-point sums times 2^-exponent; the others are derived
    from them, NaN in a bin without mass except sigma, which is 0 there."""
    edges: np.ndarray            # (nb + 1,)
    r_mid: np.ndarray            # (edges[k] + edges[k + 1]) / 2
    count: np.ndarray            # bodies per bin, int64
    mass: np.ndarray             # sum m
    sigma: np.ndarray            # surface density: mass / (pi (e2[k + 1] - e2[k])), e2 the squared edges
    vr: np.ndarray               # mass-weighted mean radial velocity
    vt: np.ndarray               # mass-weighted mean tangential velocity: the rotation curve
    sigma_r: np.ndarray          # sqrt(max(sum m vr^2 / mass - vr^2, 0))
    sigma_t: np.ndarray          # sqrt(max(sum m vt^2 / mass - vt^2, 0))
    anisotropy: np.ndarray       # 1 - (tangential variance) / (radial variance), both clipped at 0
    mass_inside: float           # inside edges[0] ...
    mass_outside: float          # ... and at or beyond edges[nb]
    count_inside: int
    count_outside: int
    enclosed: np.ndarray         # (nb + 1,): the mass inside every edge, summed in integers
    centre: tuple
    centre_velocity: tuple
    planes: np.ndarray | None = None      # raw=True: the int64 sums (6, nb + 2), plane 5 the counts ...
    exponents: np.ndarray | None = None   # ... and the five exponents: value = planes * 2^-exponent


@dataclass
class BhLagrangian:
    """Lagrangian radii of the current state about a centre (lagrangian_radii): per fraction, in the caller's order."""
    fractions: np.ndarray
    r: np.ndarray                # sqrt(r2), taken on the host
    r2: np.ndarray               # the squared radius of a body: the smallest that encloses the fraction (NaN without mass)
    count: np.ndarray            # bodies with r2_i <= r2, int64
    mass: np.ndarray             # their mass: mass_units * 2^-exponent
    mass_units: np.ndarray       # int64: sum of rint(ldexp(m_i, exponent))
    exponent: int
    centre: tuple


def radial_edges(r_min: float, r_max: float, nb: int, spacing: str = "log") -> np.ndarray:
    """nb + 1 edges from r_min to r_max: "linear" (r_min >= 0) or "log" (r_min > 0) spacing; the end points are exact."""
    nb = int(nb)
    r_min, r_max = float(r_min), float(r_max)
    if nb < 1 or not (np.isfinite(r_min) and np.isfinite(r_max) and 0.0 <= r_min < r_max):
        raise ValueError("edges need nb >= 1 and finite 0 <= r_min < r_max")
    if spacing == "linear":
        e = r_min + (r_max - r_min) * (np.arange(nb + 1) / nb)
    elif spacing == "log":
        if r_min <= 0.0:
            raise ValueError("log spacing needs r_min > 0")
        e = r_min * (r_max / r_min) ** (np.arange(nb + 1) / nb)
    else:
        raise ValueError("spacing must be 'log' or 'linear'")
    e[0], e[-1] = r_min, r_max
    return e


def radial_exponents(maxabs, n_total: int) -> np.ndarray:
    """The exponents of the radial planes (fixed_point_exponents) from the maxima of bh_radial_max."""
    return fixed_point_exponents(maxabs, n_total)


def radial_profile_from_planes(planes, exponents, edges, centre, centre_velocity=(0.0, 0.0), raw: bool = False) -> BhRadialProfile:
    """BhRadialProfile of the int64 sums (6, nb + 2) and their five exponents."""
    planes = np.asarray(planes, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1).copy()
    nb = len(edges) - 1
    if planes.shape != (6, nb + 2):
        raise ValueError("planes must be (6, nb + 2)")
    val = _scaled(planes, exponents, 5)
    mass, pr, pt, kr, kt = (v[1:-1] for v in val)
    e2 = edges * edges
    with np.errstate(divide="ignore", invalid="ignore"):
        vr, vt = pr / mass, pt / mass
        var_r, var_t = np.maximum(kr / mass - vr * vr, 0.0), np.maximum(kt / mass - vt * vt, 0.0)
        beta = 1.0 - var_t / var_r
    sig_r, sig_t = np.sqrt(var_r), np.sqrt(var_t)
    empty = mass == 0.0
    for a in (vr, vt, sig_r, sig_t, beta):
        a[empty] = np.nan
    enclosed = np.ldexp(np.cumsum(planes[0, :-1]).astype(np.float64), -int(exponents[0]))       # (integer sums: |total| <= 2^62)
    return BhRadialProfile(edges, 0.5 * (edges[:-1] + edges[1:]), planes[5, 1:-1].copy(), mass, mass / (np.pi * (e2[1:] - e2[:-1])),
                           vr, vt, sig_r, sig_t, beta, float(val[0][0]), float(val[0][-1]), int(planes[5, 0]), int(planes[5, -1]),
                           enclosed, tuple(float(x) for x in centre), tuple(float(x) for x in centre_velocity),
                           *_raw(planes, exponents, raw))


class LagrangianSelect:
    """The decisions of the radix select of the Lagrangian radii, in Python integers: which prefixes the next round needs
    (prefixes()), and which digit every fraction takes from that round's histograms (advance()).  The histograms may come
    from one context (bh_radial_select) or be the sum of many: the decisions are the same wherever they are made."""
    ROUNDS = 64 // RADIAL_DIGIT_BITS

    def __init__(self, fractions):
        self.fractions = [float(f) for f in np.asarray(fractions, dtype=np.float64).reshape(-1)]
        if not 1 <= len(self.fractions) <= RADIAL_MAX_FRACTIONS:
            raise ValueError(f"1 .. {RADIAL_MAX_FRACTIONS} fractions")
        if not all(math.isfinite(f) and 0.0 < f <= 1.0 for f in self.fractions):
            raise ValueError("a fraction must be finite, > 0 and <= 1")
        nf = len(self.fractions)
        self.round, self.total = 0, None
        self.prefix, self.below_w, self.below_n, self.target = [0] * nf, [0] * nf, [0] * nf, [0] * nf
        self.last_w, self.last_n = [0] * nf, [0] * nf

    @property
    def done(self) -> bool:
        return self.round >= self.ROUNDS or self.total == 0

    def prefixes(self) -> list:
        """The distinct prefixes of the fractions, in the order of their first appearance."""
        out = []
        for p in self.prefix:
            if p not in out:
                out.append(p)
        return out

    def advance(self, hist) -> None:
        """hist (np, 256, 2) int64: {sum w, count} per digit, for prefixes() in that order."""
        pre = self.prefixes()
        h = np.asarray(hist, dtype=np.int64).reshape(len(pre), 1 << RADIAL_DIGIT_BITS, 2).tolist()
        if self.round == 0:
            self.total = W = sum(d[0] for d in h[0])
            if W == 0:
                return
            self.target = [min(W, max(1, int(math.ceil(f * float(W))))) for f in self.fractions]
        for f in range(len(self.fractions)):
            row = h[pre.index(self.prefix[f])]
            d = 0
            while d < (1 << RADIAL_DIGIT_BITS) - 1 and self.below_w[f] + row[d][0] < self.target[f]:
                self.below_w[f] += row[d][0]
                self.below_n[f] += row[d][1]
                d += 1
            self.prefix[f] = (self.prefix[f] << RADIAL_DIGIT_BITS) | d
            self.last_w[f], self.last_n[f] = row[d][0], row[d][1]
        self.round += 1

    def result(self):
        """(r2 float64, count int64, mass_units int64) per fraction; NaN, 0, 0 for a system without mass."""
        nf = len(self.fractions)
        if self.total == 0:
            return np.full(nf, np.nan), np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
        if self.round != self.ROUNDS:
            raise ValueError("the selection has not run its eight rounds")
        r2 = np.array(self.prefix, dtype=np.uint64).view(np.float64)
        return (r2, np.array([a + b for a, b in zip(self.below_n, self.last_n)], dtype=np.int64),
                np.array([a + b for a, b in zip(self.below_w, self.last_w)], dtype=np.int64))


def lagrangian_from(fractions, r2, count, mass_units, exponent: int, centre) -> BhLagrangian:
    """BhLagrangian of the selection's results."""
    r2 = np.asarray(r2, dtype=np.float64).copy()
    units = np.asarray(mass_units, dtype=np.int64).copy()
    return BhLagrangian(np.asarray(fractions, dtype=np.float64).copy(), np.sqrt(r2), r2, np.asarray(count, dtype=np.int64).copy(),
                        np.ldexp(units.astype(np.float64), -int(exponent)), units, int(exponent), tuple(float(x) for x in centre))


MODES_MAX_M = 16                        # BH_MODES_MAX_M
MODES_MAX_BINS = 4096                   # BH_MODES_MAX_BINS


class BhModeTotal(NamedTuple):
    """One harmonic of the coherent sum over a range of bins (BhAzimuthalModes.total)."""
    amplitude: float             # |A_k| / A_0 (NaN without mass)
    phase: float                 # atan2(Im A_k, Re A_k) / k (0 for k = 0)
    pattern_speed: float         # Re(D_k / A_k); NaN for k = 0, A_k = 0 or without rates


def modes_planes(m_max: int, rates: bool) -> int:
    """The number of int64 planes of azimuthal modes up to m_max: A, with rates D, and the count."""
    return (2 if rates else 1) * (1 + 2 * int(m_max)) + 1


def modes_exponents(maxabs, n_total: int) -> np.ndarray:
    """The two exponents of the A- and the D-planes (fixed_point_exponents) from the maxima {maxA, maxD} of bh_modes_max."""
    m = np.asarray(maxabs, dtype=np.float64).reshape(-1)
    if len(m) != 2:
        raise ValueError("two maxima")
    return fixed_point_exponents(m, n_total)


def _mode_numbers(re_a, im_a, a0, re_d, im_d, k):
    """(amplitude, phase, pattern speed) of one harmonic from the values of its sums (arrays or scalars; re_d None: no rates)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.hypot(re_a, im_a) / a0
        amp = np.where(a0 == 0.0, np.nan, amp)
        phase = np.arctan2(im_a, re_a) / k if k else np.zeros_like(amp)
        if re_d is None or k == 0:
            speed = np.full_like(amp, np.nan)
        else:
            speed = (re_d * re_a + im_d * im_a) / (re_a * re_a + im_a * im_a)
            speed = np.where((re_a == 0.0) & (im_a == 0.0), np.nan, speed)
    return amp, phase, speed


@dataclass
class BhAzimuthalModes:
    """Azimuthal Fourier modes of the current state about a centre on the nb bins between edges (azimuthal_modes):
    A_k(bin) = sum m exp(i k phi) for k = 0 .. m_max, and with rates D_k(bin) = sum m w exp(i k phi), w the angular velocity of
    a body about the centre.  The sums are fixed-point integers times 2^-exponent; everything else is derived from them.

    pattern_speed = Re(D_k / A_k) is the INSTANTANEOUS rate of the phase of A_k with the membership of the bin held fixed.  It
    is exact for the sum over all slots and for a rigidly turning pattern; for a single narrow bin it ignores the flux of
    bodies across the bin's edges.  For a measured speed take pattern_speed_between two results a time dt apart."""
    edges: np.ndarray            # (nb + 1,)
    centre: tuple
    centre_velocity: tuple
    m_max: int
    count: np.ndarray            # (nb,) bodies per bin, int64
    mass: np.ndarray             # (nb,) A_0 per bin
    inside: float                # the mass inside edges[0] ...
    beyond: float                # ... and at or beyond edges[nb]
    coeff: np.ndarray            # (m_max + 1, nb) complex: A_k
    amplitude: np.ndarray        # (m_max + 1, nb): |A_k| / A_0, NaN in a bin without mass; row 0 is 1
    phase: np.ndarray            # (m_max + 1, nb): atan2(Im A_k, Re A_k) / k; row 0 is 0
    rate_coeff: np.ndarray | None = None       # rates: (m_max + 1, nb) complex D_k; row 0 / mass is the mean angular velocity
    pattern_speed: np.ndarray | None = None    # rates: (m_max + 1, nb) Re(D_k / A_k); NaN for k = 0 or A_k = 0
    planes: np.ndarray | None = None           # raw=True: the int64 sums (P, nb + 2) ...
    exponents: np.ndarray | None = None        # ... and the two exponents {A, D}: value = planes * 2^-exponent
    _units: np.ndarray | None = field(default=None, repr=False)       # the planes, kept for total()
    _exp: tuple = field(default=(0, 0), repr=False)

    @property
    def rates(self) -> bool:
        return self.rate_coeff is not None

    def total(self, k: int = 2, r_min=None, r_max=None) -> BhModeTotal:
        """Amplitude, phase and pattern speed of harmonic k of the COHERENT sum -- the integer planes added, then converted --
        over the bins whose two edges lie in [r_min, r_max] (None: from the first edge, to the last): the global bar strength
        for k = 2.  The bodies inside edges[0] and beyond edges[nb] are not part of it."""
        k = int(k)
        if not 0 <= k <= self.m_max:
            raise ValueError(f"k must be 0 .. m_max = {self.m_max}")
        lo = -np.inf if r_min is None else float(r_min)
        hi = np.inf if r_max is None else float(r_max)
        sel = np.concatenate([[False], (self.edges[:-1] >= lo) & (self.edges[1:] <= hi), [False]])
        n_a = 1 + 2 * self.m_max

        def summed(p, e):
            return float(np.ldexp(float(sum(int(v) for v in self._units[p][sel])), -e))

        e_a, e_d = self._exp
        a0 = summed(0, e_a)
        re_a, im_a = (a0, 0.0) if k == 0 else (summed(2 * k - 1, e_a), summed(2 * k, e_a))
        re_d = im_d = None
        if self.rates and k > 0:
            re_d, im_d = summed(n_a + 2 * k - 1, e_d), summed(n_a + 2 * k, e_d)
        amp, phase, speed = _mode_numbers(np.float64(re_a), np.float64(im_a), np.float64(a0), re_d, im_d, k)
        return BhModeTotal(float(amp), float(phase), float(speed))

    @staticmethod
    def pattern_speed_between(a: "BhAzimuthalModes", b: "BhAzimuthalModes", dt: float, k: int = 2, r_min=None, r_max=None) -> float:
        """The mean pattern speed of harmonic k between two results a time dt apart: the difference of the phases of their
        total(k, r_min, r_max), b's minus a's, unwrapped into (-pi / k, pi / k], over dt.  A pattern that turns
        by pi / k or more in dt cannot be followed."""
        k = int(k)
        if k < 1:
            raise ValueError("k must be at least 1")
        period = 2.0 * math.pi / k
        d = math.remainder(b.total(k, r_min, r_max).phase - a.total(k, r_min, r_max).phase, period)
        if d <= -0.5 * period:
            d += period
        return d / float(dt)


def azimuthal_modes_from_planes(planes, exponents, edges, m_max: int, rates: bool, centre, centre_velocity=(0.0, 0.0),
                                raw: bool = False) -> BhAzimuthalModes:
    """BhAzimuthalModes of the int64 sums (P, nb + 2), P = modes_planes(m_max, rates), and their two exponents."""
    planes = np.asarray(planes, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1).copy()
    nb, M, rates = len(edges) - 1, int(m_max), bool(rates)
    if planes.shape != (modes_planes(M, rates), nb + 2):
        raise ValueError("planes must be (modes_planes(m_max, rates), nb + 2)")
    e_a, e_d = (int(x) for x in exponents)
    n_a = 1 + 2 * M

    def complex_rows(first, e):
        val = np.ldexp(planes[first:first + n_a].astype(np.float64), -e)
        out = np.zeros((M + 1, nb + 2), dtype=np.complex128)
        out[0] = val[0]
        out[1:] = val[1::2] + 1j * val[2::2]
        return out

    a_all = complex_rows(0, e_a)
    a = a_all[:, 1:-1]
    mass = a[0].real.copy()
    d = complex_rows(n_a, e_d)[:, 1:-1] if rates else None
    amp, phase, speed = np.zeros((M + 1, nb)), np.zeros((M + 1, nb)), np.full((M + 1, nb), np.nan)
    for k in range(M + 1):
        amp[k], phase[k], speed[k] = _mode_numbers(a[k].real, a[k].imag, mass, d[k].real if rates else None,
                                                   d[k].imag if rates else None, k)
    return BhAzimuthalModes(edges, tuple(float(x) for x in centre), tuple(float(x) for x in centre_velocity), M,
                            planes[-1, 1:-1].copy(), mass, float(a_all[0, 0].real), float(a_all[0, -1].real), a.copy(), amp, phase,
                            d.copy() if rates else None, speed if rates else None, *_raw(planes, (e_a, e_d), raw), planes, (e_a, e_d))


DISC_MAX_BINS = 1022                    # BH_DISC_MAX_BINS
DISC_MAX_TABLE = 1024                   # BH_DISC_MAX_TABLE
TOOMRE_STELLAR = 3.36                   # Toomre (1964): Q = sigma_R kappa / (3.36 G Sigma) for a stellar disc


@dataclass
class BhRotationCurve:
    """The rotation curve of the engine's own forces about a centre on the nb bins between edges (rotation_curve): fp64 arrays
    (nb,) unless said otherwise.  mass and torque are the fixed-point sums times 2^-exponent, the others are derived from them,
    NaN in a bin where they are not defined."""
    edges: np.ndarray            # (nb + 1,)
    count: np.ndarray            # bodies per bin, int64
    mass: np.ndarray             # sum m
    radius: np.ndarray           # sum m r / sum m: the radius the bin's numbers belong to
    vc2: np.ndarray              # - sum m (x . a) / sum m: the squared circular speed (negative where the force points outwards)
    vc: np.ndarray               # sqrt(max(vc2, 0))
    omega: np.ndarray            # vc / radius
    kappa: np.ndarray            # epicyclic frequency: omega sqrt(clip(4 + d ln omega^2 / d ln radius, 1, 4)), see epicyclic_from
    torque: np.ndarray           # sum m (x cross a): the gravitational torque on the bin
    torque_cumulative: np.ndarray    # (nb + 1,): the torque on everything inside every edge, summed in integers
    mass_inside: float           # inside edges[0] ...
    mass_outside: float          # ... and at or beyond edges[nb]
    count_inside: int
    count_outside: int
    centre: tuple
    planes: np.ndarray | None = None      # raw=True: the int64 sums (5, nb + 2), plane 4 the counts ...
    exponents: np.ndarray | None = None   # ... and the four exponents: value = planes * 2^-exponent


class BhResonances(NamedTuple):
    """The radii where a pattern speed meets the disc's frequencies (resonances_from)."""
    corotation: np.ndarray       # omega = pattern speed
    inner: np.ndarray            # omega - kappa / m = pattern speed: inner Lindblad resonances
    outer: np.ndarray            # omega + kappa / m = pattern speed: outer Lindblad resonance


def _dlog(y, x) -> np.ndarray:
    """d ln y / d ln x by np.gradient over the (unevenly spaced) points; needs two points at least."""
    return np.gradient(np.log(y), np.log(x))


def epicyclic_from(radius, omega) -> np.ndarray:
    """kappa from kappa^2 = omega^2 clip(4 + d ln omega^2 / d ln radius, 1, 4) (between a Keplerian and a rigid curve), the
    derivative by np.gradient over the points given: all of them need radius > 0 and omega > 0, and there are two at least."""
    radius, omega = np.asarray(radius, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    return omega * np.sqrt(np.clip(4.0 + _dlog(omega * omega, radius), 1.0, 4.0))


def rotation_curve_from_planes(planes, exponents, edges, centre, raw: bool = False) -> BhRotationCurve:
    """BhRotationCurve of the int64 sums (5, nb + 2) and their four exponents.  kappa takes its derivative over the bins that
    have mass and vc2 > 0 (NaN in the others, and everywhere when fewer than two have)."""
    planes = np.asarray(planes, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1).copy()
    nb = len(edges) - 1
    if planes.shape != (5, nb + 2):
        raise ValueError("planes must be (5, nb + 2)")
    val = _scaled(planes, exponents, 4)
    mass, mr, mxa, torque = (v[1:-1] for v in val)
    with np.errstate(divide="ignore", invalid="ignore"):
        radius, vc2 = mr / mass, -mxa / mass
        vc = np.sqrt(np.maximum(vc2, 0.0))
        omega = vc / radius
    empty = mass == 0.0
    for a in (radius, vc2, vc, omega):
        a[empty] = np.nan
    good = ~empty & (vc2 > 0.0) & (radius > 0.0) & np.isfinite(omega)
    kappa = np.full(nb, np.nan)
    if good.sum() >= 2:
        kappa[good] = epicyclic_from(radius[good], omega[good])
    cumulative = np.ldexp(np.cumsum(planes[3, :-1]).astype(np.float64), -int(exponents[3]))        # (integer sums: |total| <= 2^62)
    return BhRotationCurve(edges, planes[4, 1:-1].copy(), mass, radius, vc2, vc, omega, kappa, torque, cumulative, float(val[0][0]),
                           float(val[0][-1]), int(planes[4, 0]), int(planes[4, -1]), tuple(float(x) for x in centre),
                           *_raw(planes, exponents, raw))


def toomre_q_from(curve: BhRotationCurve, profile: BhRadialProfile, G: float) -> np.ndarray:
    """Toomre's Q = sigma_R kappa / (3.36 G Sigma) per bin from the curve and the radial profile of the same edges and centre;
    NaN where kappa, the dispersion or a positive surface density is missing."""
    if len(curve.edges) != len(profile.edges) or not np.array_equal(curve.edges, profile.edges):
        raise ValueError("the curve and the profile must share their edges")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = profile.sigma_r * curve.kappa / (TOOMRE_STELLAR * float(G) * profile.sigma)
    q[~(profile.sigma > 0.0) | ~np.isfinite(q)] = np.nan
    return q


def _crossings(x, f, level: float) -> np.ndarray:
    """Where the broken line through (x, f) meets `level`: a point on it counts once."""
    out = []
    d = f - level
    for i in range(len(x)):
        if d[i] == 0.0:
            out.append(x[i])
        elif i + 1 < len(x) and d[i] * d[i + 1] < 0.0:
            out.append(x[i] + (x[i + 1] - x[i]) * (d[i] / (d[i] - d[i + 1])))
    return np.array(out, dtype=np.float64)


def resonances_from(curve: BhRotationCurve, pattern_speed: float, m: int = 2) -> BhResonances:
    """The radii where omega (corotation), omega - kappa / m (inner) and omega + kappa / m (outer Lindblad resonance) cross
    pattern_speed, by linear interpolation between the radii of neighbouring bins that have a kappa."""
    ok = np.isfinite(curve.kappa) & np.isfinite(curve.omega) & np.isfinite(curve.radius)
    r, w, k = curve.radius[ok], curve.omega[ok], curve.kappa[ok] / float(m)
    p = float(pattern_speed)
    return BhResonances(_crossings(r, w, p), _crossings(r, w - k, p), _crossings(r, w + k, p))


def disc_velocity_table_from(curve: BhRotationCurve, profile: BhRadialProfile, G: float, Q: float, min_count: int = 8):
    """(radii, vt, sigma_r, sigma_t) for set_disc_velocities: the table that gives the disc Toomre's Q everywhere.  Over the bins
    with count >= min_count and vc2 > 0 (ValueError when fewer than two): Sigma of the profile, omega and kappa of the curve's
    radius and vc2 (epicyclic_from over these bins), sigma_r = Q 3.36 G Sigma / kappa, sigma_t = sigma_r kappa / (2 omega)
    (the epicyclic ratio), and the asymmetric drift
    vt^2 = vc2 + sigma_r^2 (1 - kappa^2 / (4 omega^2) + d ln(Sigma sigma_r^2) / d ln radius), floored at 0."""
    if len(curve.edges) != len(profile.edges) or not np.array_equal(curve.edges, profile.edges):
        raise ValueError("the curve and the profile must share their edges")
    with np.errstate(invalid="ignore"):
        keep = (curve.count >= int(min_count)) & (curve.vc2 > 0.0) & (curve.radius > 0.0) & (profile.sigma > 0.0)
    if keep.sum() < 2:
        raise ValueError("fewer than two bins with count >= min_count and vc2 > 0")
    radius, vc2, sigma = curve.radius[keep], curve.vc2[keep], profile.sigma[keep]
    omega = np.sqrt(vc2) / radius
    kappa = epicyclic_from(radius, omega)
    sigma_r = float(Q) * TOOMRE_STELLAR * float(G) * sigma / kappa
    sigma_t = sigma_r * kappa / (2.0 * omega)
    vt2 = vc2 + sigma_r * sigma_r * (1.0 - kappa * kappa / (4.0 * omega * omega) + _dlog(sigma * sigma_r * sigma_r, radius))
    return radius, np.sqrt(np.maximum(vt2, 0.0)), sigma_r, sigma_t


@dataclass
class BhGroups:
    """Friends-of-friends groups of the current state (groups): the label of every body, and a catalogue of the groups with at
    least min_members bodies in the order (count descending, id ascending).  mass, com and velocity are the fixed-point sums
    times 2^-exponent and their quotients (sums beyond 2^53 units round to fp64 there); NaN where a group has no mass."""
    label: np.ndarray            # (n,) int64: the smallest caller index in the body's group
    n_groups: int                # all components, whatever min_members
    linking_length: float
    min_members: int
    id: np.ndarray               # (g,) int64: the label of the group
    count: np.ndarray            # (g,) int64
    mass: np.ndarray             # (g,): sum m
    com: np.ndarray              # (g, 2): sum m x / sum m
    velocity: np.ndarray         # (g, 2): sum m v / sum m
    sums: np.ndarray | None = None        # raw=True: the int64 sums (g, 5) of m, m x, m y, m vx, m vy ...
    exponents: np.ndarray | None = None   # ... and their exponents: value = sums * 2^-exponent
    stats: tuple | None = None            # with_stats=True: (distances computed, friend pairs found, unions that joined)

    def members(self, g: int) -> np.ndarray:
        """the caller indices of the bodies of catalogue entry g, ascending"""
        return np.nonzero(self.label == self.id[g])[0]


def groups_from_sums(label, n_groups: int, linking_length: float, min_members: int, ids, counts, sums, exponents,
                     raw: bool = False, stats=None) -> BhGroups:
    """BhGroups of the labels and the catalogue's int64 sums (g, 5) and their exponents."""
    sums = np.asarray(sums, dtype=np.int64).reshape(-1, 5)
    exponents = np.asarray(exponents, dtype=np.int32).reshape(5)
    val = [np.ldexp(sums[:, p].astype(np.float64), -int(exponents[p])) for p in range(5)]
    with np.errstate(divide="ignore", invalid="ignore"):
        com = np.stack([val[1] / val[0], val[2] / val[0]], axis=1)
        vel = np.stack([val[3] / val[0], val[4] / val[0]], axis=1)
    com[val[0] == 0.0] = np.nan
    vel[val[0] == 0.0] = np.nan
    return BhGroups(np.asarray(label, dtype=np.int64), int(n_groups), float(linking_length), int(min_members),
                    np.asarray(ids, dtype=np.int64), np.asarray(counts, dtype=np.int64), val[0], com, vel,
                    sums if raw else None, exponents.copy() if raw else None, stats)


@dataclass
class BhBinaries:
    """Bound pairs of the current state (binaries): every body's partner -- among the bodies j within max_separation with
    two-body energy eps_ij = 0.5 * |v_j - v_i|^2 - G (m_i + m_j) / |x_j - x_i| < 0, the one first in the order (eps_ij, j) --
    and the catalogue of the mutual pairs lo < hi, ascending in lo, with their Keplerian elements as the device computed them
    (include/bhgpu.h).  The engine's softening does not enter.  The state is read as it is: after step() the velocities lie half
    a step from the positions; synchronised elements want a step_kdk state."""
    n: int
    max_separation: float
    partner: np.ndarray          # (n,) int64: caller index of the partner, -1: none
    eps: np.ndarray              # (n,): eps of (body, partner), +inf: none
    lo: np.ndarray               # (p,) int64
    hi: np.ndarray               # (p,) int64
    separation: np.ndarray       # (p,): r = sqrt(d2)
    energy: np.ndarray           # (p,): eps, per unit reduced mass
    semi_major_axis: np.ndarray  # (p,)
    eccentricity: np.ndarray     # (p,)
    period: np.ndarray           # (p,)
    binding_energy: np.ndarray   # (p,): -(m_lo m_hi / M) eps > 0
    mass: np.ndarray             # (p,): M = m_lo + m_hi
    com: np.ndarray              # (p, 2)
    velocity: np.ndarray         # (p, 2)
    stats: tuple | None = None   # with_stats=True: (energies computed, the most by one body, nodes opened, pairs)
    mean_kinetic: object = None  # what hardness() divides by without an argument: a float, or a callable that gives it

    @property
    def total_binding_energy(self) -> float:
        return math.fsum(self.binding_energy.tolist())

    @property
    def fraction(self) -> float:
        """the fraction of bodies in a catalogued pair: 2 pairs / n"""
        return 2.0 * len(self.lo) / self.n if self.n else 0.0

    def hardness(self, mean_kinetic=None) -> np.ndarray:
        """binding_energy / mean_kinetic; by default the mean kinetic energy of a body, the engine's energy().kinetic / n, taken
        at the first such call (so call it before the run goes on) and kept"""
        if mean_kinetic is None:
            if callable(self.mean_kinetic):
                self.mean_kinetic = float(self.mean_kinetic())
            mean_kinetic = self.mean_kinetic
        if mean_kinetic is None:
            raise ValueError("hardness needs a mean kinetic energy")
        return self.binding_energy / float(mean_kinetic)

    def within(self, a_max: float) -> "BhBinaries":
        """the catalogue's pairs with semi_major_axis <= a_max (partner and eps stay whole)"""
        keep = self.semi_major_axis <= float(a_max)
        return replace(self, **{f: getattr(self, f)[keep] for f in BINARIES_COLUMNS})


BINARIES_COLUMNS = ("lo", "hi", "separation", "energy", "semi_major_axis", "eccentricity", "period", "binding_energy", "mass", "com",
                    "velocity")


def binaries_from_records(partner, eps, lo, hi, records, max_separation: float, stats=None, mean_kinetic=None) -> BhBinaries:
    """BhBinaries of the partners and the catalogue's records (p, 11) of bh_binaries_catalogue."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 11)
    partner = np.asarray(partner, dtype=np.int64).reshape(-1)
    return BhBinaries(len(partner), float(max_separation), partner, np.asarray(eps, dtype=np.float64).reshape(-1),
                      np.asarray(lo, dtype=np.int64).reshape(-1), np.asarray(hi, dtype=np.int64).reshape(-1),
                      rec[:, 0].copy(), rec[:, 1].copy(), rec[:, 2].copy(), rec[:, 3].copy(), rec[:, 4].copy(), rec[:, 5].copy(),
                      rec[:, 6].copy(), rec[:, 7:9].copy(), rec[:, 9:11].copy(), stats, mean_kinetic)


@dataclass
class BhNeighbourLists:
    """Fixed-radius neighbour lists (neighbours_within): row r holds the bodies with d2 <= radius_r * radius_r of query r --
    a body (itself left out by index) or a point (nobody left out) --, ascending in (d2, caller index), with
    d2 = dx * dx + dy * dy in fp64.  Row r is idx[offsets[r]:offsets[r + 1]] with the matching d2."""
    offsets: np.ndarray          # (q + 1,) int64: the exclusive prefix of the row lengths
    idx: np.ndarray              # (entries,) int64: caller indices
    d2: np.ndarray               # (entries,) float64
    radius: np.ndarray           # () or (q,) float64: as it was asked
    body_queries: bool           # the queries are the bodies themselves
    stats: tuple | None = None   # with_stats=True: (distances the fill pass computed, nodes it opened, entries, longest row)
    evals: np.ndarray | None = None   # with_stats=True: (q,) uint32, the distances the fill pass computed per query

    @property
    def counts(self) -> np.ndarray:
        """(q,) int64: the row lengths"""
        return np.diff(self.offsets)

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def row(self, r: int):
        """(idx, d2) of row r, as views"""
        a, b = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.idx[a:b], self.d2[a:b]

    def nearest(self):
        """(idx (q,) int64, d2 (q,)): the first entry of every row; -1 / inf for an empty row"""
        q = len(self)
        idx, d2 = np.full(q, -1, dtype=np.int64), np.full(q, np.inf)
        have = self.counts > 0
        idx[have], d2[have] = self.idx[self.offsets[:-1][have]], self.d2[self.offsets[:-1][have]]
        return idx, d2

    def pairs(self):
        """(lo, hi, d2): every unordered pair of bodies within the radius once, lo < hi, ascending in (lo, hi).  For body
        queries with one radius only: with per-query radii the relation is one-sided, and a point is nobody's partner."""
        if not self.body_queries or np.ndim(self.radius) != 0:
            raise ValueError("pairs() needs body queries and one radius: otherwise the relation is one-sided")
        lo = np.repeat(np.arange(len(self), dtype=np.int64), self.counts)
        keep = lo < self.idx
        lo, hi, d2 = lo[keep], self.idx[keep], self.d2[keep]
        order = np.lexsort((hi, lo))
        return lo[order], hi[order], d2[order]


def neighbour_lists_from(offsets, idx, d2, radius, body_queries: bool, stats=None, evals=None) -> BhNeighbourLists:
    """BhNeighbourLists of the arrays of bh_neighbour_lists (or of a twin's)."""
    radius = np.asarray(radius, dtype=np.float64)
    if radius.ndim > 1:
        raise ValueError("radius is a scalar or an array of shape (q,)")
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    idx, d2 = np.asarray(idx, dtype=np.int64).reshape(-1), np.asarray(d2, dtype=np.float64).reshape(-1)
    if len(offsets) < 1 or len(idx) != offsets[-1] or len(d2) != offsets[-1] or (radius.ndim == 1 and len(radius) != len(offsets) - 1):
        raise ValueError("offsets, idx, d2 and radius do not belong together")
    return BhNeighbourLists(offsets, idx, d2, radius, bool(body_queries), stats, evals)


MST_SUBSET_MAX = 512                    # BH_MST_SUBSET_MAX


@dataclass
class BhSpanningTree:
    """The Euclidean minimum spanning tree of the current state (spanning_tree) under the edge order (d2, lo, hi), lo < hi the
    caller indices of an edge's ends and d2 = dx * dx + dy * dy in fp64: unique, and ascending in that order.  It is the
    friends-of-friends clustering at every linking length at once: the groups at b are the components of the edges with
    d2 <= b * b."""
    lo: np.ndarray               # (n - 1,) int64
    hi: np.ndarray               # (n - 1,) int64
    d2: np.ndarray               # (n - 1,) float64, ascending
    length: np.ndarray           # sqrt(d2)
    total_length: float          # math.fsum(length)
    n: int
    stats: tuple | None = None   # with_stats=True: (rounds, distances computed, nodes skipped as own-component, edges)

    def _edges_within(self, lengths) -> np.ndarray:
        b = np.asarray(lengths, dtype=np.float64)
        if not (b >= 0.0).all():
            raise ValueError("a linking length must be >= 0")
        return np.searchsorted(self.d2, b * b, side="right")

    def n_groups_at(self, lengths):
        """the number of groups(b) at every linking length of `lengths` (any shape): n - the edges with d2 <= b * b"""
        return self.n - self._edges_within(lengths)

    def groups_at(self, b: float) -> np.ndarray:
        """(n,) int64: the label groups(b) gives every body -- the smallest caller index of its component of the edges with
        d2 <= b * b."""
        m = int(self._edges_within(float(b)))
        parent = list(range(self.n))
        for a, c in zip(self.lo[:m].tolist(), self.hi[:m].tolist()):
            while parent[a] != a:
                parent[a] = a = parent[parent[a]]
            while parent[c] != c:
                parent[c] = c = parent[parent[c]]
            if a < c:
                parent[c] = a
            else:
                parent[a] = c
        # (the larger root hangs under the smaller: parent[i] <= i, so one ascending pass resolves every body)
        label = np.arange(self.n, dtype=np.int64)
        for i in range(self.n):
            label[i] = label[parent[i]]
        return label


def spanning_tree_from(lo, hi, d2, n: int, stats=None) -> BhSpanningTree:
    """BhSpanningTree of the sorted edges of bh_spanning_tree."""
    d2 = np.asarray(d2, dtype=np.float64).reshape(-1)
    length = np.sqrt(d2)
    return BhSpanningTree(np.asarray(lo, dtype=np.int64).reshape(-1), np.asarray(hi, dtype=np.int64).reshape(-1), d2, length,
                          math.fsum(length.tolist()), int(n), stats)


@dataclass
class BhMassSegregation:
    """The mass segregation ratio Lambda_MSR of Allison et al. (2009) (mass_segregation): the mean spanning-tree length of
    random sets of n_massive bodies over the spanning-tree length of the n_massive most massive ones; above 1 when the massive
    bodies lie closer together than bodies at random."""
    ratio: float                 # mean(l_random) / l_massive
    sigma: float                 # std(l_random) / l_massive
    l_massive: float
    l_random: np.ndarray         # (n_random,)
    members: np.ndarray          # (1 + n_random, n_massive) int64: row 0 the massive set, then the random sets
    n_massive: int


def mass_segregation_from(d2, members) -> BhMassSegregation:
    """BhMassSegregation from the squared edge lengths d2 (1 + n_random, k - 1) of the sets `members` (1 + n_random, k), row 0
    the massive set: l = math.fsum(sqrt(d2)) per row, mean = fsum(l_random) / n_random, std^2 = fsum((l_random - mean)^2) /
    n_random, both over l_massive (inf or NaN where that is 0)."""
    d2 = np.asarray(d2, dtype=np.float64)
    members = np.asarray(members, dtype=np.int64)
    if d2.ndim != 2 or members.ndim != 2 or len(d2) != len(members) or len(d2) < 2 or d2.shape[1] != members.shape[1] - 1:
        raise ValueError("d2 (1 + n_random, k - 1) and members (1 + n_random, k), n_random >= 1")
    l = np.array([math.fsum(np.sqrt(row).tolist()) for row in d2])
    l_massive, l_random = float(l[0]), l[1:].copy()
    mean = math.fsum(l_random.tolist()) / len(l_random)
    std = math.sqrt(math.fsum(((l_random - mean) * (l_random - mean)).tolist()) / len(l_random))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio, sigma = float(np.float64(mean) / np.float64(l_massive)), float(np.float64(std) / np.float64(l_massive))
    return BhMassSegregation(ratio, sigma, l_massive, l_random, members, members.shape[1])


PAIR_MAX_BINS = 1024                    # BH_PAIR_MAX_BINS


@dataclass
class BhPairCounts:
    """Pair-separation counts of the current state on the nb bins between edges (pair_counts): auto mode counts every
    unordered pair of bodies once, cross mode every (point, body) combination.  A pair belongs to bin k when
    edges[k]^2 < d2 <= edges[k + 1]^2 (the upper edge inclusive), d2 = dx * dx + dy * dy in fp64."""
    edges: np.ndarray            # (nb + 1,)
    counts: np.ndarray           # (nb,) int64
    below: int                   # d2 <= edges[0]^2
    beyond: int                  # d2 > edges[nb]^2
    total: int                   # below + counts.sum() + beyond: n (n - 1) / 2, or n_points * n
    n_bodies: int
    n_points: int | None         # None in auto mode
    evals: int | None            # the distances the call computed (with_evals), a measure of the work
    cumulative: np.ndarray       # (nb + 1,) int64: the pairs with d2 <= edges[k]^2 at every edge


def pair_counts_from(raw, edges, n_bodies: int, n_points=None, evals=None) -> BhPairCounts:
    """BhPairCounts from the int64[nb + 2] of bh_pair_counts (of one context, or the sum of many)."""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1)
    ed = np.asarray(edges, dtype=np.float64).reshape(-1).copy()
    if len(raw) != len(ed) + 1:
        raise ValueError("nb + 2 counts for nb + 1 edges")
    return BhPairCounts(ed, raw[1:-1].copy(), int(raw[0]), int(raw[-1]), int(raw.sum()), int(n_bodies),
                        None if n_points is None else int(n_points), None if evals is None else int(evals), np.cumsum(raw[:-1]))


@dataclass
class BhSortSnapshot:
    """What the sort of the most recent build was given, decided and wrote (sort_snapshot).  The last six
    arrays are None unless direct input was offered to that build."""
    offered: bool                # direct input was offered (the device then decided: `counting`)
    n: int
    nb: int                      # buckets; bucket b is the range [b L, (b + 1) L) of keys_in
    L: int
    cap: int                     # T: most crossers in all
    subcap: int                  # room of one list
    nsub: int                    # lists
    keys_sorted: np.ndarray      # (n,) uint64: the sort's output (offered: the 40 key bits)
    perm: np.ndarray             # (n,) uint32: the slot each sorted key came from
    decision: np.ndarray | None = None     # (65,) uint32: word 0, then the 64 list counters of that build
    range_keys: np.ndarray | None = None   # (nb,) uint64
    lists: np.ndarray | None = None        # (nsub, subcap) uint64: the listed packed keys (counter s of them valid in list s)
    keys_in: np.ndarray | None = None      # (n,) uint64: key | slot << 40 in state order, as keys_kernel left them
    counting: bool | None = None           # the decision of direct_total on `decision`: the counting pass ran


def correlation_from(dd, dr, n: int, n_r: int) -> np.ndarray:
    """The Davis-Peebles estimate xi_k = (n_r / (n - 1)) * (2 * dd_k / dr_k) - 1 of the two-point correlation from the
    unordered auto counts dd of n bodies and the cross counts dr of n_r random points against them; NaN where dr_k = 0."""
    dd = np.asarray(dd, dtype=np.float64)
    dr = np.asarray(dr, dtype=np.float64)
    if dd.shape != dr.shape:
        raise ValueError("dd and dr must have the same shape")
    if n < 2 or n_r < 1:
        raise ValueError("the estimator needs n >= 2 bodies and n_r >= 1 random points")
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = (n_r / (n - 1)) * (2.0 * dd / dr) - 1.0
    xi[dr == 0.0] = np.nan
    return xi


NEIGHBOURS_MAX_K = 32                   # BH_NEIGHBOURS_MAX_K


def _density_k(k) -> int:
    k = int(k)
    if not 2 <= k <= NEIGHBOURS_MAX_K:
        raise ValueError(f"local density needs 2 <= k <= {NEIGHBOURS_MAX_K}")
    return k


def local_density_from(idx, d2, masses):
    """(sigma, r_k) from the k nearest neighbours idx, d2 (n, k) of every body and the masses: Casertano and Hut's estimator
    in two dimensions, sigma_i = (m of the 1st + ... + m of the (k-1)-th neighbour, added in that order) / (pi * d2 of the
    k-th), r_k = sqrt(d2 of the k-th).  sigma is NaN (and r_k inf) where a body has fewer than k neighbours, inf where
    d2 of the k-th is 0."""
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=np.float64)
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    k = _density_k(idx.shape[1])
    msum = np.zeros(len(idx))
    for j in range(k - 1):
        msum = msum + m[np.maximum(idx[:, j], 0)]
    d2k = d2[:, k - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = msum / (np.pi * d2k)
    sigma[d2k == 0.0] = np.inf
    sigma[idx[:, k - 1] < 0] = np.nan
    return sigma, np.sqrt(d2k)


def density_centre_from(sigma, positions) -> np.ndarray:
    """sum sigma_i x_i / sum sigma_i over the bodies with finite sigma, each sum with math.fsum (NaN without such a body)."""
    import math
    sigma = np.asarray(sigma, dtype=np.float64)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    ok = np.isfinite(sigma)
    w = math.fsum(sigma[ok].tolist())
    if w == 0.0:
        return np.array([np.nan, np.nan])
    return np.array([math.fsum((sigma[ok] * pos[ok, 0]).tolist()) / w, math.fsum((sigma[ok] * pos[ok, 1]).tolist()) / w])


# (q as exact fractions: ceil(q n) in integers, so that no rounding of q * n moves an index)
_QUANTILES = {"median": (1, 2), "p90": (9, 10), "p99": (99, 100), "p999": (999, 1000)}


def force_error_stats(tree, direct, targets=None) -> BhForceError:
    """Reduce tree and direct forces ((k, 2) each, row t for body targets[t], or body t without targets) to BhForceError.
    Bodies with a non-finite component are counted in n_nonfinite, then bodies with |F_dir| == 0 in n_zero; both are
    left out of every statistic.  With no body left, the statistics are NaN and worst is -1."""
    tree = np.asarray(tree, dtype=np.float64).reshape(-1, 2)
    direct = np.asarray(direct, dtype=np.float64).reshape(-1, 2)
    if tree.shape != direct.shape:
        raise ValueError("tree and direct must have the same shape")
    idx = np.arange(len(direct)) if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1)
    if len(idx) != len(direct):
        raise ValueError("one target per row")
    finite = np.isfinite(tree).all(axis=1) & np.isfinite(direct).all(axis=1)
    fd = np.hypot(direct[:, 0], direct[:, 1])
    zero = finite & (fd == 0.0)
    ok = finite & ~zero
    fd = fd[ok]
    df = np.hypot(tree[ok, 0] - direct[ok, 0], tree[ok, 1] - direct[ok, 1])
    m = int(ok.sum())
    n_nonfinite, n_zero = int((~finite).sum()), int(zero.sum())
    if m == 0:
        nan = float("nan")
        return BhForceError(0, n_zero, n_nonfinite, nan, nan, nan, nan, nan, -1, nan)
    rel = df / fd
    srt = np.sort(rel)
    q = {k: float(srt[-(-num * m // den) - 1]) for k, (num, den) in _QUANTILES.items()}
    w = int(np.argmax(rel))
    rms = float(np.sqrt(np.mean(df * df)) / np.sqrt(np.mean(fd * fd)))
    return BhForceError(m, n_zero, n_nonfinite, q["median"], q["p90"], q["p99"], q["p999"], float(srt[-1]),
                        int(idx[ok][w]), rms)


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i64ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _edges_arg(edges):
    """(the edges as a contiguous fp64 array, its pointer -- None without any --, nb) as the radial calls take them."""
    ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    return ed, (_dptr(ed) if len(ed) else None), len(ed) - 1


def _exponents_arg(exponents, count: int, words: str) -> np.ndarray:
    """A caller's `count` exponents as a contiguous int32 array."""
    e = np.ascontiguousarray(exponents, dtype=np.int32).reshape(-1)
    if len(e) != count:
        raise ValueError(words)
    return e


def sample_targets(n: int, sample: int = 65536, seed: int = 0) -> np.ndarray:
    """min(n, sample) distinct caller indices, drawn with numpy.random.default_rng(seed), in drawing order."""
    return np.random.default_rng(seed).choice(n, size=min(n, max(int(sample), 0)), replace=False).astype(np.int64)


class BarnesHutEngine:
    def __init__(self, cfg: BhConfig):
        self._lib = _lib.load()
        self.cfg = cfg
        c = _lib.bh_config(cfg.capacity, cfg.theta, cfg.G, cfg.dt, cfg.max_depth, int(cfg.precision),
                           1 if cfg.reference_compat else 0, cfg.device, cfg.n_threads, cfg.flags,
                           cfg.node_capacity)
        h = C.c_void_p()
        rc = self._lib.bh_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise BhError(rc, (self._lib.bh_last_error(None) or b"").decode())
        self._h = h
        self.n = 0
        if cfg.softening != 0.0:
            try:
                self.set_softening(cfg.softening)
            except BhError:
                self.close()
                raise

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != 0:
            raise BhError(rc, (self._lib.bh_last_error(self._h) or b"").decode())

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.bh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ------------------------------------------------------------------------------
    def upload(self, positions, velocities, masses) -> None:
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 2)
        vel = np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1, 2)
        m = np.ascontiguousarray(masses, dtype=np.float64).reshape(-1)
        if not (len(pos) == len(vel) == len(m)):
            raise ValueError("positions, velocities and masses must have the same length")
        self._check(self._lib.bh_upload(self._h, _dptr(pos), _dptr(vel), _dptr(m), len(m)))
        self.n = len(m)

    def download(self):
        pos = np.empty((self.n, 2))
        vel = np.empty((self.n, 2))
        self._check(self._lib.bh_download(self._h, _dptr(pos), _dptr(vel)))
        return pos, vel

    def initialize(self, n: int, seed: int = 0, kind: str = "box", lower_m=1e-1, higher_m=5e-1,
                   lower_p=-1e-1, higher_p=1e-1, lower_v=-1e-4, higher_v=1e-4) -> None:
        """On-device initial conditions (initializeGpu, project.cu:304-341; defaults = its
        constants, project.cu:30-35).  kind "plummer": scale lower_p, truncation higher_p, equal
        masses higher_m, zero velocities.  Body i is a function of (seed, i) alone.

        The Plummer radius is drawn again while it lies beyond higher_p, up to 64 draws; after that the last
        one stands, with probability (1 - M(higher_p))^64 per body, M(r) = r^3 / (r^2 + a^2)^(3/2): below 1e-12
        for higher_p >= a, about 0.2 at higher_p = 0.3 a.  BhError -1 unless lower_p is finite and > 0, higher_p
        is > 0 (inf: untruncated) and higher_m is finite."""
        k = {"box": 0, "plummer": 1}[kind]
        self._check(self._lib.bh_initialize(self._h, n, seed, k, lower_m, higher_m, lower_p, higher_p,
                                            lower_v, higher_v))
        self.n = n

    def masses(self) -> np.ndarray:
        m = np.empty(self.n)
        self._check(self._lib.bh_download_masses(self._h, _dptr(m)))
        return m

    # -- hot path ---------------------------------------------------------------------------
    def step(self, nsteps: int = 1) -> None:
        self._check(self._lib.bh_step(self._h, nsteps))

    def sync(self) -> None:
        self._check(self._lib.bh_sync(self._h))

    # -- kick, drift, time-step criterion, leapfrog ---------------------------------------------
    def kick(self, h: float) -> None:
        """v += a h from the accelerations of the last compute_forces() (BhError -5 when they are not those of the
        current positions).  The arithmetic per precision: include/bhgpu.h."""
        self._check(self._lib.bh_kick(self._h, float(h)))

    def forces_current(self) -> bool:
        """Whether the force buffer holds the accelerations of the current positions: whether kick(), timestep() and
        rotation_curve() would accept it.  The host's record; nothing is launched."""
        cur = C.c_int32()
        self._check(self._lib.bh_forces_current(self._h, C.byref(cur)))
        return bool(cur.value)

    def drift(self, h: float) -> None:
        """p += v h.  The forces, the potential and the tree stop being current."""
        self._check(self._lib.bh_drift(self._h, float(h)))

    def timestep(self, eta: float, length: float | None = None) -> BhTimestep:
        """dt = eta * sqrt(length / a_max) over the accelerations of the last compute_forces(), reduced on the device;
        length None: the softening length."""
        t = _lib.bh_timestep_t()
        self._check(self._lib.bh_timestep(self._h, float(eta), 0.0 if length is None else float(length), C.byref(t)))
        return BhTimestep(t.dt, t.a_max, t.worst, t.n_bodies)

    def step_kdk(self, nsteps: int = 1) -> None:
        """nsteps kick-drift-kick leapfrog steps at cfg.dt: velocities and positions are synchronised on return, and the
        closing forces serve the next call.  nsteps + 1 walks (nsteps when the forces were current)."""
        self._check(self._lib.bh_step_kdk(self._h, nsteps))

    def step_adaptive(self, t_end: float, eta: float, length: float | None = None, dt_max: float | None = None,
                      t: float = 0.0):
        """Kick-drift-kick steps with dt = min(timestep(eta, length).dt, dt_max, t_end - t) chosen anew before every step,
        from t until t == t_end exactly.  Returns (t, steps).  Raises BhError when a step comes out 0 or not finite
        (coincident bodies; no acceleration at all and no dt_max)."""
        t, t_end, steps = float(t), float(t_end), 0
        while t < t_end:
            try:
                ts = self.timestep(eta, length)
            except BhError as e:
                if e.code != -5:
                    raise
                self._check(self._lib.bh_compute_forces(self._h))       # the forces were not current
                ts = self.timestep(eta, length)
            dt = ts.dt if dt_max is None else min(ts.dt, float(dt_max))
            last = not (dt < t_end - t)
            if last:
                dt = t_end - t
            if not (dt > 0.0 and dt < float("inf")):
                raise BhError(-1, f"step_adaptive: time step {dt!r} at t = {t!r} (a_max = {ts.a_max!r}, body {ts.worst})")
            self.kick(0.5 * dt)
            self.drift(dt)
            self._check(self._lib.bh_compute_forces(self._h))
            self.kick(0.5 * dt)
            t = t_end if last else t + dt
            steps += 1
        return t, steps

    def build_tree(self) -> None:
        self._check(self._lib.bh_build_tree(self._h))

    def compute_forces(self) -> np.ndarray:
        self._check(self._lib.bh_compute_forces(self._h))
        return self.forces()

    def forces(self) -> np.ndarray:
        f = np.empty((self.n, 2))
        self._check(self._lib.bh_get_forces(self._h, _dptr(f)))
        return f

    def accelerations(self) -> np.ndarray:
        a = np.empty((self.n, 2))
        self._check(self._lib.bh_get_accel(self._h, _dptr(a)))
        return a

    def interaction_counts(self) -> np.ndarray:
        """Accepted force evaluations per body of the last walk (FLAG_WALK_STATS; fp32 / mixed / Precision.F64), caller order."""
        c = np.zeros(max(self.n, 1), dtype=np.uint32)
        self._check(self._lib.bh_get_interaction_counts(self._h, c.ctypes.data_as(C.POINTER(C.c_uint32))))
        return c[:self.n]

    # -- Plummer softening ------------------------------------------------------------------
    def set_softening(self, eps: float) -> None:
        """Softening length eps >= 0 of every term evaluated from now on: force G m M (dx, dy) / (d2 + eps^2)^(3/2),
        potential -G M / sqrt(d2 + eps^2), in the force walks, the potential, the field, the direct sum and the force
        check.  Acceptance and the self / coincident-body tests stay on the geometric distance, so the set of terms does
        not depend on eps.  0 (the default) is the unsoftened law; Precision.F64_EXACT refuses any other value.  The
        potential has to be recomputed after a change."""
        self._check(self._lib.bh_set_softening(self._h, float(eps)))

    @property
    def softening(self) -> float:
        eps = C.c_double()
        self._check(self._lib.bh_get_softening(self._h, C.byref(eps)))
        return eps.value

    # -- diagnostics ------------------------------------------------------------------------
    def potential(self, with_counts: bool = False):
        """Potential per unit mass of every body (caller order) over the force walk's terms of the current state;
        with_counts: also the terms summed per body.  Builds a tree; the run is not perturbed."""
        self._check(self._lib.bh_compute_potential(self._h))
        phi = np.zeros(max(self.n, 1))
        cnt = np.zeros(max(self.n, 1), dtype=np.uint32) if with_counts else None
        self._check(self._lib.bh_get_potential(self._h, _dptr(phi),
                                               cnt.ctypes.data_as(C.POINTER(C.c_uint32)) if with_counts else None))
        return (phi[:self.n], cnt[:self.n]) if with_counts else phi[:self.n]

    def energy(self) -> BhEnergy:
        """Kinetic, potential and total energy, momentum, angular momentum, centre of mass of the current state."""
        e = _lib.bh_energy_t()
        self._check(self._lib.bh_energy(self._h, C.byref(e)))
        return BhEnergy(e.kinetic, e.potential, e.total, (e.momentum[0], e.momentum[1]), e.angular_momentum,
                        (e.com[0], e.com[1]), e.mass, e.n_bodies)

    # -- exact forces and the Barnes-Hut force error --------------------------------------------
    def _targets(self, targets):
        """(int64 array or None, count, pointer for the C-ABI) of a target list (None: every body)."""
        if targets is None:
            return None, self.n, None
        t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
        return t, len(t), t.ctypes.data_as(C.POINTER(C.c_int64)) if len(t) else (C.c_int64 * 1)()

    def direct_forces(self, targets=None) -> np.ndarray:
        """fp64 direct-sum forces of the current state (main_approach_1.cpp:53-75 bit for bit) on the caller indices
        `targets` (None: every body), shape (k, 2).  Reads the state only."""
        _, k, tp = self._targets(targets)
        f = np.zeros((max(k, 1), 2))
        self._check(self._lib.bh_direct_forces(self._h, tp, k, _dptr(f)))
        return f[:k]

    def force_check(self, targets=None):
        """(tree, direct), (k, 2) each: the precision's Barnes-Hut forces of the current state (a quiet tree build and
        the force walk; n_threads applies) and the direct-sum forces, on `targets` (None: every body).  The run is not
        perturbed: forces(), interaction_counts(), stats() and the following steps are as they were."""
        _, k, tp = self._targets(targets)
        tree, direct = np.zeros((max(k, 1), 2)), np.zeros((max(k, 1), 2))
        self._check(self._lib.bh_force_check(self._h, tp, k, _dptr(tree), _dptr(direct)))
        return tree[:k], direct[:k]

    def force_error(self, sample: int = 65536, seed: int = 0, targets=None) -> BhForceError:
        """Barnes-Hut force error of the current state against the direct sum on min(n, sample) distinct caller indices
        drawn with numpy.random.default_rng(seed) (or on `targets`): force_error_stats of force_check."""
        if targets is None:
            targets = sample_targets(self.n, sample, seed)
        t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
        tree, direct = self.force_check(t)
        return force_error_stats(tree, direct, t)

    # -- the field at arbitrary points ----------------------------------------------------------
    def field(self, points, with_counts: bool = False):
        """(accel (k, 2), phi (k,)[, counts (k,)]) at the coordinates `points` (k, 2): what the precision's Barnes-Hut walk
        of the current state gives a body standing there that is nobody -- no self skip, so a point ON a body is
        non-finite in the fp64 precisions and feels nothing of that body in F32 / MIXED.  Row t belongs to points[t],
        whatever else is in the list.  Builds a tree; the run is not perturbed."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        k = len(p)
        acc, phi = np.zeros((max(k, 1), 2)), np.zeros(max(k, 1))
        cnt = np.zeros(max(k, 1), dtype=np.uint32) if with_counts else None
        self._check(self._lib.bh_field_at(self._h, _dptr(p) if k else None, k, _dptr(acc), _dptr(phi),
                                          cnt.ctypes.data_as(C.POINTER(C.c_uint32)) if with_counts else None))
        return (acc[:k], phi[:k], cnt[:k]) if with_counts else (acc[:k], phi[:k])

    # -- moment maps ----------------------------------------------------------------------------
    @staticmethod
    def _map_args(box, scheme):
        b = np.ascontiguousarray(box, dtype=np.float64).reshape(-1)
        if len(b) != 4:
            raise ValueError("box = (xmin, xmax, ymin, ymax)")
        if scheme not in MAP_SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(MAP_SCHEMES)}")
        return b, MAP_SCHEMES[scheme]

    def moment_map(self, box, nx: int, ny: int, scheme: str = "cic", raw: bool = False) -> BhMomentMap:
        """Surface density, mean velocity and velocity dispersion of the current state on nx x ny cells over
        box = (xmin, xmax, ymin, ymax), deposited on the device ("ngp": nearest grid point, "cic": cloud in cell) in
        fixed point: the same bodies give the same bits in any order.  Reads the state only; the run is not perturbed.
        raw: also the int64 planes and their exponents."""
        b, sch = self._map_args(box, scheme)
        nx, ny = int(nx), int(ny)
        ok = nx >= 1 and ny >= 1 and nx * ny <= MAP_MAX_CELLS          # (else the call refuses before it writes)
        planes = np.zeros((4, ny, nx) if ok else (4, 1, 1), dtype=np.int64)
        e = np.zeros(4, dtype=np.int32)
        nd = C.c_int64()
        self._check(self._lib.bh_moment_map(self._h, _dptr(b), nx, ny, sch, _i64ptr(planes), _i32ptr(e), C.byref(nd)))
        return moment_map_from_planes(planes, e, b, scheme, nd.value, raw)

    def moment_map_max(self) -> np.ndarray:
        """max |m|, |m vx|, |m vy|, |m (vx^2 + vy^2)| over this context's bodies (zeros without bodies)."""
        m = np.zeros(4)
        self._check(self._lib.bh_moment_map_max(self._h, _dptr(m)))
        return m

    def moment_map_deposit(self, box, nx: int, ny: int, scheme: str, exponents):
        """(device pointer of the int64 grid 4 x ny x nx, n_deposited): this context's bodies deposited with the caller's
        exponents (moment_exponents); the grid stays valid until the next moment-map call."""
        b, sch = self._map_args(box, scheme)
        e = _exponents_arg(exponents, 4, "four exponents")
        p, nd = C.c_void_p(), C.c_int64()
        self._check(self._lib.bh_moment_map_deposit(self._h, _dptr(b), int(nx), int(ny), sch, _i32ptr(e), C.byref(p), C.byref(nd)))
        return p.value, nd.value

    # -- radial profiles and Lagrangian radii -----------------------------------------------------
    def centre_of(self, centre) -> np.ndarray:
        """(cx, cy) of "density" (density_centre(6)), "com" (energy().com) or a pair."""
        if isinstance(centre, str):
            if centre == "density":
                return np.ascontiguousarray(self.density_centre(6), dtype=np.float64)
            if centre == "com":
                return np.array(self.energy().com, dtype=np.float64)
            raise ValueError("centre must be 'density', 'com' or a pair (x, y)")
        c = np.ascontiguousarray(centre, dtype=np.float64).reshape(-1)
        if len(c) != 2:
            raise ValueError("centre must be 'density', 'com' or a pair (x, y)")
        return c

    @staticmethod
    def _pair_or_zero(v) -> np.ndarray:
        u = np.zeros(2) if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if len(u) != 2:
            raise ValueError("centre_velocity must be a pair (ux, uy)")
        return u

    def radial_profile(self, edges, centre="density", centre_velocity=None, raw: bool = False) -> BhRadialProfile:
        """Surface density, rotation curve, radial and tangential dispersion and anisotropy of the current state in the bins
        between `edges` (nb + 1 ascending radii, see radial_edges) about `centre` ("density", "com" or a pair), velocities
        relative to centre_velocity (default 0); binned on the device in fixed point: the same bodies give the same bits in any
        order.  Reads the state only; the run is not perturbed.  raw: also the int64 planes and their exponents."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        ed, edp, nb = _edges_arg(edges)
        ok = 1 <= nb <= RADIAL_MAX_BINS                            # (else the call refuses before it writes)
        planes = np.zeros((6, nb + 2) if ok else (6, 3), dtype=np.int64)
        e = np.zeros(5, dtype=np.int32)
        self._check(self._lib.bh_radial_profile(self._h, _dptr(c), _dptr(u), edp, nb, _i64ptr(planes), _i32ptr(e)))
        return radial_profile_from_planes(planes, e, ed, c, u, raw)

    def radial_max(self, centre, centre_velocity=None) -> np.ndarray:
        """max |m|, |m vr|, |m vt|, |m vr^2|, |m vt^2| over this context's bodies about the pair `centre` (zeros without bodies)."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        m = np.zeros(5)
        self._check(self._lib.bh_radial_max(self._h, _dptr(c), _dptr(u), _dptr(m)))
        return m

    def radial_deposit(self, edges, centre, centre_velocity, exponents) -> int:
        """Device pointer of the int64 planes 6 x (nb + 2): this context's bodies binned with the caller's exponents
        (radial_exponents); valid until the next radial call."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        _, edp, nb = _edges_arg(edges)
        e = _exponents_arg(exponents, 5, "five exponents")
        p = C.c_void_p()
        self._check(self._lib.bh_radial_deposit(self._h, _dptr(c), _dptr(u), edp, nb, _i32ptr(e), C.byref(p)))
        return p.value

    def lagrangian_radii(self, fractions=(0.01, 0.1, 0.5, 0.9), centre="density") -> BhLagrangian:
        """The radii about `centre` ("density", "com" or a pair) that enclose the mass fractions: for each the smallest body
        radius inside which (ties included) at least that fraction of the fixed-point mass lies, selected on the device in
        eight histogram passes -- no sort, no download of the state.  Reads the state only; the run is not perturbed."""
        c = self.centre_of(centre)
        f = np.ascontiguousarray(fractions, dtype=np.float64).reshape(-1)
        nf = len(f)
        k = max(nf, 1)
        r2, cnt, mass, e = np.zeros(k), np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), C.c_int32()
        self._check(self._lib.bh_lagrangian_radii(self._h, _dptr(c), _dptr(f) if nf else None, nf, _dptr(r2), _i64ptr(cnt),
                                                  _i64ptr(mass), C.byref(e)))
        return lagrangian_from(f, r2[:nf], cnt[:nf], mass[:nf], e.value, c)

    def radial_select(self, centre, exponent: int, round: int, prefixes) -> int:
        """Device pointer of one select round's histograms, len(prefixes) x 256 x {sum w, count} int64, over this context's
        bodies (LagrangianSelect makes the decisions); valid until the next radial call."""
        c = self.centre_of(centre)
        pre = np.array([int(p) for p in prefixes], dtype=np.uint64)
        p = C.c_void_p()
        self._check(self._lib.bh_radial_select(self._h, _dptr(c), int(exponent), int(round),
                                               pre.ctypes.data_as(C.POINTER(C.c_uint64)) if len(pre) else None, len(pre), C.byref(p)))
        return p.value

    def radial_times(self):
        """(max_ms, main_ms, rounds_ms (8,)) of the last radial call: HIP events around the first pass, around the deposit or
        the select rounds together, and around every select round."""
        a, b, r = C.c_double(), C.c_double(), np.zeros(8)
        self._check(self._lib.bh_radial_times(self._h, C.byref(a), C.byref(b), _dptr(r)))
        return a.value, b.value, r

    # -- azimuthal modes --------------------------------------------------------------------------
    def azimuthal_modes(self, edges, m_max: int = 4, centre="density", centre_velocity=None, rates: bool = False,
                        raw: bool = False) -> BhAzimuthalModes:
        """The azimuthal Fourier coefficients A_k = sum m exp(i k phi), k = 0 .. m_max, of the current state in the bins between
        `edges` (nb + 1 ascending radii, see radial_edges) about `centre` ("density", "com" or a pair): relative amplitude
        (k = 2: the bar strength) and phase per bin, and with rates=True the sums D_k = sum m w exp(i k phi) and the
        instantaneous pattern speed Re(D_k / A_k), velocities relative to centre_velocity (default 0).  Summed on the device in
        fixed point without a trigonometric function: the same bodies give the same bits in any order.  pattern_speed holds
        the membership of a bin fixed: exact for the sum over all slots and for a rigid pattern, it ignores the flux of bodies
        across the edges of a single narrow bin (see BhAzimuthalModes).  Reads the state only; the run is not perturbed.
        raw: also the int64 planes and their two exponents."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        ed, edp, nb = _edges_arg(edges)
        M, rates = int(m_max), bool(rates)
        ok = 1 <= nb <= MODES_MAX_BINS and 0 <= M <= MODES_MAX_M   # (else the call refuses before it writes)
        planes = np.zeros((modes_planes(M, rates), nb + 2) if ok else (1, 3), dtype=np.int64)
        e = np.zeros(2, dtype=np.int32)
        self._check(self._lib.bh_azimuthal_modes(self._h, _dptr(c), _dptr(u), edp, nb, M, int(rates), _i64ptr(planes), _i32ptr(e)))
        return azimuthal_modes_from_planes(planes, e, ed, M, rates, c, u, raw)

    def modes_max(self, centre, centre_velocity=None, m_max: int = 4, rates: bool = False) -> np.ndarray:
        """{maxA, maxD}: the largest |m c_k|, |m s_k| and (rates) |m w c_k|, |m w s_k| over this context's bodies and k = 0 ..
        m_max about the pair `centre` (zeros without bodies; maxD = 0 without rates)."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        m = np.zeros(2)
        self._check(self._lib.bh_modes_max(self._h, _dptr(c), _dptr(u), int(m_max), int(bool(rates)), _dptr(m)))
        return m

    def modes_deposit(self, edges, centre, centre_velocity, exponents, m_max: int = 4, rates: bool = False) -> int:
        """Device pointer of the int64 planes modes_planes(m_max, rates) x (nb + 2): this context's bodies summed with the
        caller's two exponents (modes_exponents); valid until the next modes call."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        _, edp, nb = _edges_arg(edges)
        e = _exponents_arg(exponents, 2, "two exponents")
        p = C.c_void_p()
        self._check(self._lib.bh_modes_deposit(self._h, _dptr(c), _dptr(u), edp, nb, int(m_max), int(bool(rates)), _i32ptr(e),
                                               C.byref(p)))
        return p.value

    def modes_times(self):
        """(max_ms, deposit_ms) of the last modes call: HIP events around the first pass and around the deposit."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.bh_modes_times(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- a disc: initial conditions, rotation curve, Toomre's Q, velocities -------------------------
    def initialize_disc(self, n: int, seed: int = 0, mass: float = 1.0, scale: float = 0.02, r_max: float = 0.2) -> None:
        """On-device positions of a Kuzmin-Toomre disc: surface density mass scale / (2 pi (R^2 + scale^2)^(3/2)) cut at r_max
        (inf: no cut), equal masses mass / n, zero velocities -- equilibrate_disc gives it velocities.  Body i is a function of
        (seed, i) alone, bit for bit that of tests/disc_ref.py.  BhError -1 unless scale is finite and > 0, r_max > 0 and mass
        finite."""
        self._check(self._lib.bh_initialize_disc(self._h, int(n), int(seed), float(mass), float(scale), float(r_max)))
        self.n = int(n)

    def rotation_curve(self, edges, centre="density", raw: bool = False) -> BhRotationCurve:
        """Circular speed, omega, kappa and gravitational torque of the current state in the bins between `edges` (nb + 1
        ascending radii, nb <= 1,022) about `centre` ("density", "com" or a pair), from the accelerations of the last
        compute_forces() (BhError -5 when they are not those of the current positions); summed on the device in fixed point:
        the same bodies give the same bits in any order.  Reads the state and the forces only; the run is not perturbed.
        raw: also the int64 planes and their exponents."""
        c = self.centre_of(centre)
        ed, edp, nb = _edges_arg(edges)
        ok = 1 <= nb <= DISC_MAX_BINS                              # (else the call refuses before it writes)
        planes = np.zeros((5, nb + 2) if ok else (5, 3), dtype=np.int64)
        e = np.zeros(4, dtype=np.int32)
        self._check(self._lib.bh_rotation_curve(self._h, _dptr(c), edp, nb, _i64ptr(planes), _i32ptr(e)))
        return rotation_curve_from_planes(planes, e, ed, c, raw)

    def toomre_q(self, edges, centre="density") -> np.ndarray:
        """Toomre's Q per bin (toomre_q_from) of the current state: its rotation curve and its radial profile about one centre."""
        c = self.centre_of(centre)
        return toomre_q_from(self.rotation_curve(edges, c), self.radial_profile(edges, c), self.cfg.G)

    def set_disc_velocities(self, radii, vt, sigma_r, sigma_t, seed: int = 0, centre=(0.0, 0.0), centre_velocity=(0.0, 0.0)) -> None:
        """Every body's velocity from a table over ascending radii (1 .. 1,024 of them), interpolated linearly at the body's
        radius about `centre` and held constant beyond the table's ends: the tangential speed vt + sigma_t g2 and the radial
        speed sigma_r g1 with g1, g2 two standard deviates of (seed, caller index) alone, plus centre_velocity; a body at the
        centre gets centre_velocity.  Only the velocities change: the forces stay current, as after kick()."""
        c, u = self.centre_of(centre), self._pair_or_zero(centre_velocity)
        tabs = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in (radii, vt, sigma_r, sigma_t)]
        k = len(tabs[0])
        if any(len(t) != k for t in tabs):
            raise ValueError("radii, vt, sigma_r and sigma_t must have the same length")
        ptrs = [_dptr(t) if k else None for t in tabs]
        self._check(self._lib.bh_set_disc_velocities(self._h, _dptr(c), _dptr(u), *ptrs, k, int(seed)))

    def equilibrate_disc(self, Q: float = 1.5, edges=None, seed: int = 0, centre="com"):
        """Velocities that hold the current bodies -- a disc at rest, as initialize_disc leaves it -- in equilibrium with
        Toomre's Q: the forces (computed when they are not current), their rotation curve and the radial profile in `edges`
        (default: 32 log bins from a tenth of the half-mass radius to the largest body radius), the table of
        disc_velocity_table_from and set_disc_velocities.  Returns (curve, (radii, vt, sigma_r, sigma_t))."""
        c = self.centre_of(centre)
        if edges is None:
            lag = self.lagrangian_radii((0.5, 1.0), c)
            edges = radial_edges(0.1 * float(lag.r[0]), float(np.nextafter(lag.r[1], np.inf)), 32, "log")
        if not self.forces_current():
            self._check(self._lib.bh_compute_forces(self._h))
        curve = self.rotation_curve(edges, c)
        table = disc_velocity_table_from(curve, self.radial_profile(edges, c), self.cfg.G, Q)
        self.set_disc_velocities(*table, seed=seed, centre=c)
        return curve, table

    def disc_times(self):
        """(init_ms, curve_max_ms, curve_deposit_ms, velocities_ms): HIP events around the kernels of the last initialize_disc,
        rotation_curve (its two passes) and set_disc_velocities."""
        t = [C.c_double() for _ in range(4)]
        self._check(self._lib.bh_disc_times(self._h, *(C.byref(x) for x in t)))
        return tuple(x.value for x in t)

    # -- neighbours -----------------------------------------------------------------------------
    def _query_points(self, points):
        """(array or None, number of queries, pointer for the C-ABI) of a query list (None: every body)."""
        if points is None:
            return None, self.n, None
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        return p, len(p), _dptr(p) if len(p) else (C.c_double * 2)()

    def neighbours(self, k: int, points=None, with_evals: bool = False):
        """(idx (q, k) int64, d2 (q, k) float64[, evals (q,) uint32]): the k nearest bodies of every body (points None; the
        body itself left out by index) or of the coordinates `points` (q, 2) (nobody left out), in the order (d2, caller
        index) with d2 = dx * dx + dy * dy in fp64; idx = -1 and d2 = inf where there are fewer than k.  evals: the distances
        the search computed per query.  Reads the state only; the run is not perturbed."""
        p, q, pp = self._query_points(points)
        k = int(k)
        kk = k if 1 <= k <= NEIGHBOURS_MAX_K else 1             # (else the call refuses before it writes)
        idx = np.full((max(q, 1), kk), -1, dtype=np.int64)
        d2 = np.full((max(q, 1), kk), np.inf)
        ev = np.zeros(max(q, 1), dtype=np.uint32) if with_evals else None
        self._check(self._lib.bh_neighbours(self._h, pp, q, k, idx.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(d2),
                                            ev.ctypes.data_as(C.POINTER(C.c_uint32)) if with_evals else None))
        return (idx[:q], d2[:q], ev[:q]) if with_evals else (idx[:q], d2[:q])

    def count_within(self, radius: float, points=None) -> np.ndarray:
        """uint32 (q,): the bodies with d2 <= radius * radius of every body (points None; itself left out) or of `points`."""
        p, q, pp = self._query_points(points)
        cnt = np.zeros(max(q, 1), dtype=np.uint32)
        self._check(self._lib.bh_count_within(self._h, pp, q, float(radius), cnt.ctypes.data_as(C.POINTER(C.c_uint32))))
        return cnt[:q]

    def neighbours_times(self):
        """(build_ms, query_ms) of the last neighbours() / count_within(): HIP events around the structure's build and the
        searches."""
        b, q = C.c_double(), C.c_double()
        self._check(self._lib.bh_neighbours_times(self._h, C.byref(b), C.byref(q)))
        return b.value, q.value

    # -- neighbour lists ------------------------------------------------------------------------
    def neighbours_within(self, radius, points=None, max_entries=None, with_stats: bool = False) -> BhNeighbourLists:
        """Every body within `radius` (a scalar, or one radius per query, shape (q,)) of every body (points None; itself left
        out by index) or of the coordinates `points` (q, 2): see BhNeighbourLists.  Two calls: one that counts (about the cost
        of a count_within), then, with the arrays allocated, one that fills.  More than max_entries entries in all (None: no
        limit) raise BhError with BH_ERR_CAPACITY, and the message carries the number needed.  Reads the state only; the run is
        not perturbed."""
        p, q, pp = self._query_points(points)
        rad = np.asarray(radius, dtype=np.float64)
        if rad.ndim > 1:
            raise ValueError("radius is a scalar or an array of shape (q,)")
        flat = np.ascontiguousarray(rad).reshape(-1)
        i64 = C.POINTER(C.c_int64)
        off = np.zeros(q + 1, dtype=np.int64)
        total = C.c_int64()
        rp = _dptr(flat) if len(flat) else (C.c_double * 1)()
        call = self._lib.bh_neighbour_lists
        self._check(call(self._h, pp, q, rp, len(flat), 0, off.ctypes.data_as(i64), None, None, C.byref(total), None))
        room = total.value if max_entries is None else int(max_entries)
        idx, d2 = np.zeros(max(room, 1), dtype=np.int64), np.zeros(max(room, 1))
        st = (C.c_uint64 * 4)()
        self._check(call(self._h, pp, q, rp, len(flat), room, off.ctypes.data_as(i64), idx.ctypes.data_as(i64), _dptr(d2), C.byref(total), st))
        ev = None
        if with_stats:
            ev = np.zeros(max(q, 1), dtype=np.uint32)
            self._check(self._lib.bh_neighbour_lists_evals(self._h, q, ev.ctypes.data_as(C.POINTER(C.c_uint32))))
        return neighbour_lists_from(off, idx[:total.value], d2[:total.value], rad, points is None,
                                    tuple(int(v) for v in st) if with_stats else None, ev[:q] if with_stats else None)

    def neighbour_lists_times(self):
        """(build_ms, count_ms, fill_ms, sort_ms) of the last bh_neighbour_lists call (neighbours_within makes two; this is the
        filling one): HIP events around the index's build, the count pass, scan and fill, and the row sorts."""
        t = [C.c_double() for _ in range(4)]
        self._check(self._lib.bh_neighbour_lists_times(self._h, *[C.byref(v) for v in t]))
        return tuple(v.value for v in t)

    # -- pair counts ----------------------------------------------------------------------------
    def pair_counts_raw(self, edges, points=None):
        """(int64[nb + 2] = below, the nb bins, beyond; evals) of bh_pair_counts over this context's bodies."""
        p, q, pp = self._query_points(points)
        ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        nb = len(ed) - 1
        raw = np.zeros(nb + 2 if 1 <= nb <= PAIR_MAX_BINS else 3, dtype=np.int64)  # (else the call refuses before it writes)
        ev = C.c_int64()
        self._check(self._lib.bh_pair_counts(self._h, pp, q, _dptr(ed) if len(ed) else None, nb,
                                             raw.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ev)))
        return raw, ev.value

    def pair_counts(self, edges, points=None, with_evals: bool = False) -> BhPairCounts:
        """The pairs of bodies (points None: every unordered pair once) or of `points` (q, 2) and bodies (every combination)
        per separation bin between `edges` (nb + 1 ascending radii, see radial_edges), counted on the device in one
        traversal: the brute-force histogram bit for bit.  Reads the state only; the run is not perturbed."""
        raw, ev = self.pair_counts_raw(edges, points)
        return pair_counts_from(raw, edges, self.n, None if points is None else len(np.asarray(points).reshape(-1, 2)),
                                ev if with_evals else None)

    def pair_counts_times(self):
        """(build_ms, query_ms) of the last pair_counts(): HIP events around the structure's build and the traversals."""
        b, q = C.c_double(), C.c_double()
        self._check(self._lib.bh_pair_counts_times(self._h, C.byref(b), C.byref(q)))
        return b.value, q.value

    def correlation(self, edges, randoms):
        """(xi, dd, dr): the Davis-Peebles two-point correlation of the current state in the bins between `edges` from the
        auto counts dd and the cross counts dr of the random points `randoms` (n_r, 2) -- see correlation_from."""
        dd = self.pair_counts(edges)
        dr = self.pair_counts(edges, randoms)
        return correlation_from(dd.counts, dr.counts, self.n, dr.n_points), dd, dr

    # -- groups ---------------------------------------------------------------------------------
    def groups(self, linking_length: float, min_members: int = 2, raw: bool = False, with_stats: bool = False) -> BhGroups:
        """Friends-of-friends groups of the current state: bodies i, j are friends when d2 = dx * dx + dy * dy <= linking_length^2
        (fp64, nothing fused), a group is a connected component, its label the smallest caller index in it -- the brute-force
        definition bit for bit.  The catalogue holds the groups with at least min_members bodies.  raw: also the int64 sums and
        their exponents; with_stats: the work counters.  Reads the state only; the run is not perturbed."""
        n = self.n
        label = np.zeros(max(n, 1), dtype=np.int64)
        ng, nc = C.c_int64(), C.c_int64()
        st = (C.c_uint64 * 3)()
        i64 = C.POINTER(C.c_int64)
        self._check(self._lib.bh_groups(self._h, float(linking_length), int(min_members), label.ctypes.data_as(i64), C.byref(ng),
                                        C.byref(nc), st))
        g = nc.value
        ids, counts = np.zeros(max(g, 1), dtype=np.int64), np.zeros(max(g, 1), dtype=np.int64)
        sums, e = np.zeros((max(g, 1), 5), dtype=np.int64), np.zeros(5, dtype=np.int32)
        got = C.c_int64()
        self._check(self._lib.bh_groups_catalogue(self._h, g, ids.ctypes.data_as(i64), counts.ctypes.data_as(i64),
                                                  sums.ctypes.data_as(i64), e.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(got)))
        return groups_from_sums(label[:n], ng.value, linking_length, min_members, ids[:g], counts[:g], sums[:g], e, raw,
                                tuple(int(v) for v in st) if with_stats else None)

    def groups_times(self):
        """(build_ms, link_ms, catalogue_ms) of the last groups(): HIP events around the index's build, the linking and
        labelling, and the catalogue."""
        b, l, k = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.bh_groups_times(self._h, C.byref(b), C.byref(l), C.byref(k)))
        return b.value, l.value, k.value

    # -- spanning trees -------------------------------------------------------------------------
    def spanning_tree(self, with_stats: bool = False) -> BhSpanningTree:
        """The Euclidean minimum spanning tree of the current state under the edge order (d2, lo, hi) -- unique, the brute-force
        tree bit for bit -- by Boruvka rounds on the index of the neighbour queries.  groups_at(b) of the result equals
        groups(b).label at every b.  Reads the state only; the run is not perturbed."""
        n = self.n
        m = max(n - 1, 0)
        lo, hi, d2 = np.zeros(max(m, 1), dtype=np.int64), np.zeros(max(m, 1), dtype=np.int64), np.zeros(max(m, 1))
        st = (C.c_uint64 * 4)()
        i64 = C.POINTER(C.c_int64)
        self._check(self._lib.bh_spanning_tree(self._h, lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), _dptr(d2), st))
        return spanning_tree_from(lo[:m], hi[:m], d2[:m], n, tuple(int(v) for v in st) if with_stats else None)

    def spanning_tree_times(self):
        """(build_ms, rounds_ms, sort_ms) of the last spanning_tree(): HIP events around the index's build, the rounds and the
        sort of the edges (the host's ordering of equal d2 added); after subset_spanning_trees(): 0, the kernels, the host's sort of the rows."""
        b, r, s = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.bh_spanning_tree_times(self._h, C.byref(b), C.byref(r), C.byref(s)))
        return b.value, r.value, s.value

    def subset_spanning_trees(self, members):
        """(lo, hi, d2), each (n_sets, k - 1): the minimum spanning tree of every row of `members` (n_sets, k) caller indices,
        of those k bodies alone, under the edge order of spanning_tree, each row ascending; 2 <= k <= MST_SUBSET_MAX, no
        index twice in a row.  One wavefront per row."""
        mem = np.ascontiguousarray(members, dtype=np.int64)
        if mem.ndim != 2:
            raise ValueError("members must be (n_sets, k)")
        sets, k = mem.shape
        m = max(k - 1, 1)
        lo, hi, d2 = (np.zeros((max(sets, 1), m), dtype=np.int64), np.zeros((max(sets, 1), m), dtype=np.int64),
                      np.zeros((max(sets, 1), m)))
        i64 = C.POINTER(C.c_int64)
        self._check(self._lib.bh_spanning_tree_subsets(self._h, mem.ctypes.data_as(i64) if mem.size else (C.c_int64 * 1)(), sets, k,
                                                       lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), _dptr(d2)))
        return lo[:sets], hi[:sets], d2[:sets]

    def mass_segregation_sets(self, n_massive: int, n_random: int = 500, seed: int = 0, weights=None) -> np.ndarray:
        """(1 + n_random, n_massive) int64: row 0 the n_massive bodies of largest `weights` (default: the masses; ties go to the
        smaller index), row 1 + r the random set np.random.default_rng([seed, r]).choice(n, n_massive, replace=False)."""
        n, k, R = self.n, int(n_massive), int(n_random)
        if not (2 <= k <= min(n, MST_SUBSET_MAX)) or R < 1:
            raise ValueError(f"n_massive must be 2 .. min(n, {MST_SUBSET_MAX}) and n_random >= 1")
        w = self.masses() if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if len(w) != n:
            raise ValueError("one weight per body")
        rows = [np.argsort(-w, kind="stable")[:k]]
        rows += [np.random.default_rng([int(seed), r]).choice(n, k, replace=False) for r in range(R)]
        return np.stack(rows).astype(np.int64)

    def mass_segregation(self, n_massive: int, n_random: int = 500, seed: int = 0, weights=None) -> BhMassSegregation:
        """The mass segregation ratio of the current state: the spanning trees of the massive set and of n_random random sets in
        one subset_spanning_trees call -- see mass_segregation_sets and mass_segregation_from."""
        members = self.mass_segregation_sets(n_massive, n_random, seed, weights)
        return mass_segregation_from(self.subset_spanning_trees(members)[2], members)

    # -- binaries -------------------------------------------------------------------------------
    def binaries(self, max_separation: float, with_stats: bool = False) -> BhBinaries:
        """Bound pairs of the current state: every body's partner among the bodies within max_separation (inclusive; inf: no
        cut, and a body bound to nobody then searches everything) that are bound to it, eps_ij < 0, first in the order
        (eps_ij, caller index) -- the brute-force definition bit for bit --, and the catalogue of the mutual pairs with their
        Keplerian elements; see BhBinaries.  The softening does not enter.  Reads the state as it is (synchronised elements want
        a step_kdk state); the run is not perturbed."""
        n = self.n
        partner, eps = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1))
        npairs = C.c_int64()
        st = (C.c_uint64 * 4)()
        i64 = C.POINTER(C.c_int64)
        self._check(self._lib.bh_binaries(self._h, float(max_separation), partner.ctypes.data_as(i64), _dptr(eps), C.byref(npairs), st))
        p = npairs.value
        lo, hi, rec = np.zeros(max(p, 1), dtype=np.int64), np.zeros(max(p, 1), dtype=np.int64), np.zeros((max(p, 1), 11))
        self._check(self._lib.bh_binaries_catalogue(self._h, p, lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), _dptr(rec)))
        return binaries_from_records(partner[:n], eps[:n], lo[:p], hi[:p], rec[:p], max_separation,
                                     tuple(int(v) for v in st) if with_stats else None,
                                     (lambda: self.energy().kinetic / n) if n else None)

    def binaries_times(self):
        """(build_ms, search_ms, catalogue_ms) of the last binaries(): HIP events around the index's build with the sorted
        velocities, masses and mass bounds, the partner search, and the pairs with their elements (the host's ordering added)."""
        b, s, k = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.bh_binaries_times(self._h, C.byref(b), C.byref(s), C.byref(k)))
        return b.value, s.value, k.value

    def local_density(self, k: int = 6):
        """(sigma (n,), r_k (n,)): Casertano and Hut's k-th-neighbour density estimate in two dimensions from one
        neighbours(k) call and the masses -- see local_density_from."""
        idx, d2 = self.neighbours(_density_k(k))
        return local_density_from(idx, d2, self.masses())

    def density_centre(self, k: int = 6) -> np.ndarray:
        """(x, y): the density-weighted centre sum sigma_i x_i / sum sigma_i over the bodies with finite sigma (math.fsum)."""
        sigma, _ = self.local_density(k)
        return density_centre_from(sigma, self.download()[0])

    # -- tree output ------------------------------------------------------------------------
    def export_tree(self):
        """(nodes in DFS pre-order as TREE_NODE_DTYPE, depth)."""
        n = C.c_int64(0)
        rc = self._lib.bh_export_tree(self._h, None, None, 0, C.byref(n))
        if rc not in (0, -4):
            self._check(rc)
        nodes = np.zeros(max(n.value, 1), dtype=TREE_NODE_DTYPE)
        depth = np.zeros(max(n.value, 1), dtype=np.int32)
        self._check(self._lib.bh_export_tree(self._h, nodes.ctypes.data,
                                             depth.ctypes.data_as(C.POINTER(C.c_int32)), len(nodes),
                                             C.byref(n)))
        return nodes[: n.value], depth[: n.value]

    def write_quadtree_file(self, path: str) -> None:
        self._check(self._lib.bh_write_quadtree_file(self._h, os.fsencode(path)))

    # -- measurement ------------------------------------------------------------------------
    def stats(self) -> BhStats:
        s = _lib.bh_stats_t()
        self._check(self._lib.bh_stats(self._h, C.byref(s)))
        return BhStats(s.n_bodies, s.n_nodes, s.n_internal, s.steps_done, s.visits, s.interactions,
                       s.wave_nodes, s.last_step_ms, s.build_ms, s.walk_ms, s.device_bytes, s.keys_ms, s.sort_ms,
                       s.scan_ms, s.nodes_ms, s.build_bytes, s.walk_bytes, s.wave_quads, s.sort_spill_buckets,
                       s.let_tree_ms, s.let_pack_ms, s.sort_rerun_buckets, s.wave_accepts, s.walk_launches)

    def sort_snapshot(self) -> BhSortSnapshot:
        """The most recent build's sort (bh_sort_snapshot): whether direct input was offered, its geometry, the 65 decision
        words, range keys, crosser lists and input keys of that build, and its output.  Waits, then copies: the run is not
        perturbed."""
        info = (C.c_int64 * 8)()
        none = [None] * 6
        self._check(self._lib.bh_sort_snapshot(self._h, info, *none))
        offered, n, nb, L, cap, subcap, nsub, words = (int(v) for v in info)
        u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        ks, pm = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        if not offered:
            self._check(self._lib.bh_sort_snapshot(self._h, info, None, None, None, None, ks.ctypes.data_as(u64), pm.ctypes.data_as(u32)))
            return BhSortSnapshot(False, n, nb, L, cap, subcap, nsub, ks[:n], pm[:n])
        dec, rk = np.zeros(1 + words, dtype=np.uint32), np.zeros(nb, dtype=np.uint64)
        lst, kin = np.zeros(max(nsub * subcap, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self._lib.bh_sort_snapshot(self._h, info, dec.ctypes.data_as(u32), rk.ctypes.data_as(u64), lst.ctypes.data_as(u64),
                                               kin.ctypes.data_as(u64), ks.ctypes.data_as(u64), pm.ctypes.data_as(u32)))
        held = dec[1:1 + nsub].astype(np.int64)
        counting = bool(dec[0] != 0 or (held > subcap).any() or held.sum() > cap)
        return BhSortSnapshot(True, n, nb, L, cap, subcap, nsub, ks[:n], pm[:n], dec, rk, lst[:nsub * subcap].reshape(nsub, subcap),
                              kin[:n], counting)

    def sort_paths(self):
        """(placed, passed): buckets of the bucket sort finished by placement, and buckets that went through byte passes,
        both cumulative since the engine was created (bh_sort_paths)."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.bh_sort_paths(self._h, out))
        return int(out[0]), int(out[1])

    def step_times(self):
        """(step_ms[k], walk_ms[k]) of the steps of the last step() call (at most 4,096): HIP events per step."""
        n = C.c_int32(0)
        self._check(self._lib.bh_step_times(self._h, None, None, 0, C.byref(n)))
        st, wk = np.zeros(max(n.value, 1)), np.zeros(max(n.value, 1))
        self._check(self._lib.bh_step_times(self._h, _dptr(st), _dptr(wk), n.value, C.byref(n)))
        return st[:n.value], wk[:n.value]

    @staticmethod
    def build_info() -> str:
        """What the loaded library was built from (bh_build_info) and whether it is the product library."""
        info = (_lib.load().bh_build_info() or b"").decode()
        return info + ("" if _lib.is_product_library() else f" VARIANT={os.path.basename(_lib.LIB_PATH)}")

    # -- multi-GPU plumbing -----------------------------------------------------------------
    def set_owned_fraction(self, rank: int, world: int) -> None:
        self._check(self._lib.bh_set_owned_fraction(self._h, rank, world))

    def owned_range(self):
        lo, hi = C.c_int64(), C.c_int64()
        self._check(self._lib.bh_owned_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def step_local(self) -> None:
        self._check(self._lib.bh_step_local(self._h))

    def scatter_sorted(self) -> None:
        self._check(self._lib.bh_scatter_sorted(self._h))

    def device_sorted(self):
        """Device pointer of the sorted-order exchange buffer: {x, y, vx, vy} float32 per sorted body."""
        p = C.c_void_p()
        self._check(self._lib.bh_device_sorted(self._h, C.byref(p)))
        return p.value

    def device_state(self):
        p, v, m = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, eb = C.c_int64(), C.c_int32()
        self._check(self._lib.bh_device_state(self._h, C.byref(p), C.byref(v), C.byref(m), C.byref(n),
                                              C.byref(eb)))
        return p.value, v.value, m.value, n.value, eb.value

    # -- distributed step with locally-essential trees ----------------------------------------
    def let_local_quads(self) -> int:
        """Quads this context reserves for its own tree; the forest_base of let_configure must be the
        maximum of this over all ranks."""
        q = C.c_int64()
        self._check(self._lib.bh_let_local_quads(self._h, C.byref(q)))
        return q.value

    def let_configure(self, rank: int, world: int, let_cap: int, forest_base: int | None = None) -> None:
        """forest_base None: this context's own let_local_quads() -- only right when every rank's
        context has the same capacity."""
        if forest_base is None:
            forest_base = self.let_local_quads()
        self._check(self._lib.bh_let_configure(self._h, rank, world, let_cap, forest_base))
        self._let_world = world

    def let_bounds(self, quiet: bool = False) -> None:
        """quiet: for a diagnostic between two steps -- the walk's bounds records stay for the next let_bounds()."""
        self._check((self._lib.bh_let_bounds_quiet if quiet else self._lib.bh_let_bounds)(self._h))

    def let_pointers(self):
        """(lbounds, all_bounds, send, recv, block_bytes, boxes_per_rank): device pointers for the two
        collectives; lbounds holds boxes_per_rank x 4 doubles, all_bounds world times that."""
        a, b, s, r = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nb, k = C.c_int64(), C.c_int32()
        self._check(self._lib.bh_let_pointers(self._h, C.byref(a), C.byref(b), C.byref(s), C.byref(r), C.byref(nb),
                                              C.byref(k)))
        return a.value, b.value, s.value, r.value, nb.value, k.value

    def let_build(self, quiet: bool = False) -> None:
        """quiet: for a diagnostic between two steps -- no re-order, and everything a later step reads from an earlier
        one (build count, sort samples, walk counters, the order the ORB cost weights are indexed by) is put back."""
        self._check((self._lib.bh_let_build_quiet if quiet else self._lib.bh_let_build)(self._h))

    def let_walk(self) -> None:
        self._check(self._lib.bh_let_walk(self._h))

    def let_forces(self) -> None:
        self._check(self._lib.bh_let_forces(self._h))

    def let_walk_local(self) -> None:
        self._check(self._lib.bh_let_walk_local(self._h))

    def let_walk_remote(self, integrate: bool = True) -> None:
        self._check(self._lib.bh_let_walk_remote(self._h, 1 if integrate else 0))

    def let_potential(self, with_counts: bool = False):
        """Potential per unit mass of this rank's bodies (the order of download() / ids()) over the forest force walk's
        terms: the own tree, then the received LETs in rank order.  Needs what let_forces() needs: a let_build() of the
        current state and the peers' blocks delivered.  with_counts: also the terms summed per body."""
        self._check(self._lib.bh_let_potential(self._h))
        phi = np.zeros(max(self.n, 1))
        cnt = np.zeros(max(self.n, 1), dtype=np.uint32) if with_counts else None
        self._check(self._lib.bh_let_get_potential(self._h, _dptr(phi),
                                                   cnt.ctypes.data_as(C.POINTER(C.c_uint32)) if with_counts else None))
        return (phi[:self.n], cnt[:self.n]) if with_counts else phi[:self.n]

    def let_energy_sums(self) -> np.ndarray:
        """This rank's share of (sum m, sum m x, sum m y, sum m vx, sum m vy, sum Lz, sum m |v|^2, sum m phi): raw fp64
        sums of the deterministic device reduction (runs let_potential() unless the potential is current)."""
        q = np.zeros(8)
        self._check(self._lib.bh_let_energy(self._h, _dptr(q)))
        return q

    def let_counts(self, with_overflow: bool = False):
        """Per peer, the largest LET of any let_build since the previous let_counts / let_configure (waits
        for the stream), and whether any of those builds overflowed -- a LET beyond let_cap, or a local
        tree beyond node_capacity.  Reading starts a new interval.  Raises BhError(-4) on overflow, unless
        with_overflow: then returns (counts, overflow flag)."""
        arr = (C.c_uint32 * self._let_world)()
        if with_overflow:
            ov = C.c_int32()
            self._check(self._lib.bh_let_counts(self._h, arr, C.byref(ov)))
            return list(arr), bool(ov.value)
        self._check(self._lib.bh_let_counts(self._h, arr, None))
        return list(arr)

    # -- device-side migration and re-balancing (LET scheme) ------------------------------------
    def set_ids(self, ids) -> None:
        a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if len(a) != self.n:
            raise ValueError("one id per body")
        self._check(self._lib.bh_set_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_int64))))

    def ids(self) -> np.ndarray:
        a = np.empty(self.n, dtype=np.int64)
        self._check(self._lib.bh_get_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_int64))))
        return a

    @staticmethod
    def _cuts_struct(cuts):
        c = _lib.bh_orb_cuts()
        c.world, c.n_cuts = cuts.world, cuts.world - 1
        for k in range(4):
            c.box[k] = float(cuts.box[k])
        for k in range(cuts.world - 1):
            c.axis[k], c.value[k] = int(cuts.axis[k]), float(cuts.value[k])
        return c

    def orb_histogram(self, cuts, level: int):
        """(device pointer, number of uint64 words) of the weighted histograms of the cut tree's regions
        at `level` (row k = the region whose cut is k, ORB_BINS bins across the root box)."""
        c = self._cuts_struct(cuts)
        p, nw = C.c_void_p(), C.c_int64()
        self._check(self._lib.bh_orb_histogram(self._h, C.byref(c), level, C.byref(p), C.byref(nw)))
        return p.value, nw.value

    def migrate_pack(self, cuts):
        """Classify the local bodies by the cut tree and group them by destination in the send buffer;
        returns the number of bodies for every rank (waits for the stream)."""
        c = self._cuts_struct(cuts)
        cnt = (C.c_int64 * cuts.world)()
        self._check(self._lib.bh_migrate_pack(self._h, C.byref(c), cnt))
        return list(cnt)

    def migrate_pointers(self):
        """(send, recv device pointers, capacity in records of 6 doubles)."""
        s, r, cap = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._lib.bh_migrate_pointers(self._h, C.byref(s), C.byref(r), C.byref(cap)))
        return s.value, r.value, cap.value

    def migrate_unpack(self, n_new: int) -> None:
        self._check(self._lib.bh_migrate_unpack(self._h, n_new))
        self.n = n_new

    def set_stream(self, hip_stream: int) -> None:
        self._check(self._lib.bh_set_stream(self._h, C.c_void_p(hip_stream)))
