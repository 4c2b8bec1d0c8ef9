"""The two-pass reductions of csrc/bh_diag.hpp (energy sums) and csrc/bh_split.hpp (time-step argmax) beyond one
grid-stride trip -- a helper of tests/test_reductions_cpu.py, tests/test_gpu_reductions.py and tests/test_gpu_energy.py,
not a test file.

Both reductions run 256 workgroups of 256 threads, so thread l takes bodies l, l + 65,536, l + 131,072, ...: a second
body per thread, a ragged last trip, a tie between records of different trips and orig[] past 65,536 all begin at
n = 65,537.  SIZES are the sizes the tests use: one body past a trip plus a few (65,543), a ragged trip that spills
into a second workgroup (65,799 = 65,536 + 256 + 7), two trips (131,079) and three (196,909).

mirrored_state() is an input whose momentum and centre-of-mass sums nearly cancel, device_sum() the kernel's summation
tree in numpy, sum2_tolerance() the bound a compensated sum has to meet.  Measured here (tests/test_reductions_cpu.py
asserts what the table shows; seed 1, error against math.fsum divided by sum2_tolerance, the smallest and the largest
of the four cancelling terms m vx, m vy, m x, m y):

    n          exact tree   np.cumsum[-1]       np.sum              no c += c2 in fold   lanes without c
    65,543     0 .. 0       7.9e3 .. 7.6e4      3.2e2 .. 2.9e3      1.3e3 .. 4.6e3       0 .. 0
    65,799     0 .. 0       1.9e3 .. 8.0e4      9.3e2 .. 6.0e3      98 .. 2.0e3          0 .. 7.9
    131,079    0 .. 0       5.7e2 .. 1.6e4      91 .. 4.9e2         66 .. 1.1e3          4.8 .. 34
    196,909    0 .. 0       1.1e3 .. 1.7e4      37 .. 4.1e2         4.9 .. 1.9e2         4.8 .. 9.3

(the exact tree reproduces math.fsum bit for bit on these inputs; in absolute terms the tolerance is 7e-18 to 2e-16
here, a plain sum is off by 1e-13 to 5e-13, numpy's pairwise sum by 3e-15 to 7e-14).  A lane has one to four terms:
with a single trip its own compensation is exactly zero, and with two it has little to lose -- other seeds give less
than the tolerance there --, so that variant is held to a miss at 196,909 only."""
import functools
import math

import numpy as np

SIZES = [65543, 65799, 131079, 196909]
SEED = 1
STRIDE = 256 * 256                   # kDiagParts * kBlock = kTsParts * kBlock
MIN_CONDITION = 1e10                 # sum |t| / |sum t| of the momentum terms of mirrored_state
# The centre-of-mass terms cancel as exactly, but what is left is the planted bodies' m x ~ 1.5e-3 each against
# sum |m x| ~ n / 2: n / (2 * 8 * 1.5 * 2e-3) >= 1.3e6 at n = 65,536, taking every planted body at its largest.
MIN_CONDITION_POSITION = 1e6


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def mirrored_state(n, seed):
    """(m, p, v), every value exactly representable in fp32 (so one state serves all four precisions, and every
    product m * x of two of them is exact in fp64): h pairs of bodies with equal masses in [0.5, 1.5], velocities v1 in
    [-1, 1]^2 and -v1, positions x1 in [0.01, 1]^2 and -x1, whose m v and m x terms cancel exactly, and k = 7 or 8
    planted bodies (n - k is even) of masses in [0.5, 1.5], velocities in [1e-9, 2e-9]^2 and positions in
    [1e-3, 2e-3]^2, which are all that is left of the four sums.  One permutation shuffles everything.
    sum |t| / |sum t| at SIZES, seed 1: 2.7e12 to 9.4e12 for m vx and m vy, 3.1e6 to 1.0e7 for m x and m y (condition())."""
    k = 7 + ((n - 7) % 2)
    h = (n - k) // 2
    assert n >= k and k + 2 * h == n
    r = np.random.default_rng(seed)
    m1 = _f32(r.uniform(0.5, 1.5, h))
    v1 = _f32(r.uniform(-1.0, 1.0, (h, 2)))
    x1 = _f32(r.uniform(0.01, 1.0, (h, 2)))
    mp = _f32(r.uniform(0.5, 1.5, k))
    vp = _f32(r.uniform(1e-9, 2e-9, (k, 2)))
    xp = _f32(r.uniform(1e-3, 2e-3, (k, 2)))
    m = np.concatenate([m1, m1, mp])
    v = np.concatenate([v1, -v1, vp])
    x = np.concatenate([x1, -x1, xp])
    perm = r.permutation(n)
    return m[perm], x[perm], v[perm]


@functools.lru_cache(maxsize=None)
def state(n):
    """mirrored_state(n, SEED), built once and read-only."""
    out = mirrored_state(n, SEED)
    for a in out:
        a.setflags(write=False)
    return out


def terms(m, x, v, phi):
    """The eight per-body terms of energy_partial_kernel in its operation order, nothing fused (numpy rounds every
    product and sum on its own): m, m x, m y, m vx, m vy, m (x vy - y vx), m (vx vx + vy vy), m phi."""
    px, py, vx, vy = x[:, 0], x[:, 1], v[:, 0], v[:, 1]
    return [m, m * px, m * py, m * vx, m * vy, m * (px * vy - py * vx), m * (vx * vx + vy * vy), m * phi]


NAMES = ["mass", "m*x", "m*y", "m*vx", "m*vy", "Lz", "m*v2", "m*phi"]


def condition(t):
    """sum |t| / |sum t|, both by math.fsum."""
    return math.fsum(np.abs(t)) / abs(math.fsum(t))


def sum2_tolerance(ref, scale, n):
    """2 spacing(|ref|) + (2 n 2^-53)^2 scale -- derived, not measured.

    It is the bound of Ogita, Rump and Oishi (Accurate sum and dot product, SIAM J. Sci. Comput. 26, 2005, Prop. 4.5) for
    a compensated sum res of x_1 .. x_n: |res - s| <= u |s| + gamma^2 sum |x_i| with u = 2^-53, where gamma = k u / (1 - k u)
    counts the additions of the longest chain.  The tree of bh_diag.hpp performs fewer than 2 n additions in all -- n into the
    lanes' pairs, then one neumaier_add and one c += c2 per fold, 2 * 65,535 + 2 * 255 of them --, so gamma is taken
    over 2 n (2 n u <= 4.4e-11 for the sizes here: the denominator 1 - 2 n u is dropped, it changes the twelfth
    digit).  u |s| <= spacing(|ref|) / 2 rounded up to one spacing covers the rounding of the compensated result; the second
    spacing is the one further rounding of the closing `s + c` that the kernel performs when it hands a double to the host.
    `scale` is sum |x_i|, `ref` the exact sum (math.fsum)."""
    return 2.0 * float(np.spacing(abs(ref))) + (2.0 * n * 2.0 ** -53) ** 2 * scale


def quotient_tolerance(s1, s0, t1, t0):
    """The bound for com = q1 / q0 against s1 / s0 when |q1 - s1| <= t1 and |q0 - s0| <= t0 (s0 > t0 >= 0):

        q1 / q0 - s1 / s0 = ((q1 - s1) - (s1 / s0) (q0 - s0)) / q0,   |q0| >= |s0| - t0
        => |q1 / q0 - s1 / s0| <= (t1 + |s1 / s0| t0) / (|s0| - t0)

    plus one rounding, spacing(|s1 / s0|): half an ulp for the host's division of the two device sums and half for the
    division that forms the reference."""
    r = abs(s1 / s0)
    return (t1 + r * t0) / (abs(s0) - t0) + float(np.spacing(r))


# ---- the kernel's summation tree in numpy ------------------------------------------------------------------------------
def _neumaier_add(s, c, x):
    t = s + x
    c = c + np.where(np.abs(s) >= np.abs(x), (s - t) + x, (x - t) + s)
    return t, c


def _block_fold(s, c, drop_fold_c):
    """diag_block_fold over the last axis (256 lanes): lane l takes lane l + h for h = 128, 64, .. 1."""
    h = s.shape[-1] // 2
    while h > 0:
        a, b = _neumaier_add(s[..., :h], c[..., :h], s[..., h:2 * h])
        if not drop_fold_c:
            b = b + c[..., h:2 * h]
        s, c = a, b
        h //= 2
    return s[..., 0], c[..., 0]


def device_sum(t, drop_fold_c=False, drop_lane_c=False):
    """energy_partial_kernel + energy_final_kernel for one quantity: lane l of 65,536 adds t[l], t[l + 65,536], .. into its
    Neumaier pair (a lane without a body in the last trip adds nothing: adding 0.0 leaves a pair as it is), each
    workgroup of 256 lanes folds its pairs in the halving tree, a second launch folds the 256 records the same way, and
    s + c closes.  drop_fold_c: neumaier_fold without its `c += c2`; drop_lane_c: the lanes sum plainly, the folds are
    whole.  Only tests/test_reductions_cpu.py uses this, to show that sum2_tolerance tells the variants apart: the
    order of the device's summation is not an interface, and no GPU test compares bits with it."""
    t = np.asarray(t, dtype=np.float64)
    trips = -(-len(t) // STRIDE)
    x = np.zeros(trips * STRIDE)
    x[:len(t)] = t
    x = x.reshape(trips, 256, 256)
    s, c = np.zeros((256, 256)), np.zeros((256, 256))
    for k in range(trips):
        s, c = _neumaier_add(s, c, x[k])
    if drop_lane_c:
        c = np.zeros_like(c)
    s, c = _block_fold(s, c, drop_fold_c)                    # pass 1: one record per workgroup
    s, c = _block_fold(s, c, drop_fold_c)                    # pass 2
    return float(s + c)


# ---- what the GPU tests assert of a BhEnergy -----------------------------------------------------------------------------
def check_sums(q, tt, n, what=""):
    """q: the device's eight raw sums; tt: terms() of the downloaded state.  Each within sum2_tolerance of math.fsum."""
    for k, t in enumerate(tt):
        ref, scale = math.fsum(t), math.fsum(np.abs(t))
        tol = sum2_tolerance(ref, scale, n)
        err = abs(q[k] - ref)
        print(f"{what} n {n} {NAMES[k]}: |got - fsum| {err:.3g}, tolerance {tol:.3g}, condition {scale / abs(ref) if ref else math.inf:.3g}")
        assert err <= tol, (what, n, NAMES[k], q[k], ref, err, tol)


def check_energy(a, tt, n, what=""):
    """a: a BhEnergy; tt: terms() of the downloaded state.  mass, momentum, angular momentum, kinetic and potential
    as check_sums (2 * kinetic is the device's sum exactly: the host's factor 1/2 is a power of two), com as the quotient."""
    S = [math.fsum(t) for t in tt]
    A = [math.fsum(np.abs(t)) for t in tt]
    T = [sum2_tolerance(s, sc, n) for s, sc in zip(S, A)]
    got = {0: a.mass, 3: a.momentum[0], 4: a.momentum[1], 5: a.angular_momentum, 6: 2.0 * a.kinetic, 7: 2.0 * a.potential}
    for k, g in got.items():
        err = abs(g - S[k])
        print(f"{what} n {n} {NAMES[k]}: |got - fsum| {err:.3g}, tolerance {T[k]:.3g}")
        assert err <= T[k], (what, n, NAMES[k], g, S[k], err, T[k])
    for k in (1, 2):
        ref, tol = S[k] / S[0], quotient_tolerance(S[k], S[0], T[k], T[0])
        err = abs(a.com[k - 1] - ref)
        print(f"{what} n {n} com[{k - 1}]: |got - quotient| {err:.3g}, tolerance {tol:.3g}")
        assert err <= tol, (what, n, f"com[{k - 1}]", a.com[k - 1], ref, err, tol)
    assert a.total == a.kinetic + a.potential and a.n_bodies == n
