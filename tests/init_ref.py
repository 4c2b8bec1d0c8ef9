"""A numpy twin of the on-device initialiser (csrc/bh_init.hpp): Philox-4x32-10, the five coordinate streams of the box
distribution and the rejection loop of the projected Plummer sphere, body by body.

What the device does in IEEE arithmetic alone (the 53-bit uniforms, the linear range rule -- bh_engine.hip is built with
-ffp-contract=off, so u * (upper - lower) + lower is two roundings --, 2 u - 1, 2 pi u) is done here in fp64 and equals the
device bit for bit.  What goes through the device's libm (log10 / pow of the log-uniform rule, pow(u, -2/3), sqrt, cos, sin)
is done here in extended precision from the same fp64 inputs: the twin is the value, the device an approximation of it.

The generator is tied to Random123's published known-answer vectors in test_init_cpu.py before anything is compared with it.
numpy only: no GPU, no oracle."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the twin needs an extended-precision long double (x87: 64-bit significand)"

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)
COUNTER_TAG = 0x9E3779B9        # the fourth counter word of every draw
PLUMMER_STREAM0 = 16            # try t of the rejection loop draws from stream 16 + t
PLUMMER_TRIES = 64
TWO_PI = 6.283185307179586      # the kernel's literal
U_MIN = 1e-300                  # the kernel's clamp of the radius uniform
# (seed, n, a, hp): the Plummer cases that the device is compared on.  test_init_cpu.py asserts what makes them fit for it.
PLUMMER_CASES = [(1, 4099, 0.02, 0.2), (1, 1024, 0.02, 0.02), (1, 1024, 0.02, 0.006)]
F32_STATE = ("F32",)            # Precision names whose state arrays are fp32 (state64() in bh_engine.hip is mode != F32)


def philox4x32_10(counter, key, rounds=10):
    """Philox-4x32 (Salmon et al. 2011).  counter: four words, key: two words, each a scalar or an array (broadcast
    together); uint64 arithmetic masked to 32 bits.  Returns the four output words as uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & M32 for x in key]
    shape = np.broadcast(*c, *k).shape
    c = [np.broadcast_to(x, shape).copy() for x in c]
    k0, k1 = (np.broadcast_to(x, shape).copy() for x in k)
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]           # 32 x 32 -> 64 bits: no wrap in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & M32, (p0 >> S32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def draw(seed, i, stream):
    """The kernel's layout: counter [i_lo, i_hi, stream, 0x9E3779B9], key [seed_lo, seed_hi].  seed: a Python int below
    2^64; i, stream: ints or arrays."""
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    i = np.asarray(i, dtype=np.uint64)
    return philox4x32_10([i & M32, i >> S32, stream, COUNTER_TAG], [seed & 0xFFFFFFFF, seed >> 32])


def u01(hi, lo):
    """Uniform fp64 in [0, 1) from 53 bits: the 32 of `hi` above the upper 21 of `lo`.  Exact."""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    return ((hi << np.uint64(21)) ^ (lo >> np.uint64(11))).astype(np.float64) * (1.0 / 9007199254740992.0)


def is_log(lower, upper):
    return lower > 0 and upper > 0


def sample_range(u, lower, upper):
    """The reference's rule: both bounds positive -> log-uniform (returned in extended precision: it goes through libm on
    the device), anything else -> linear, in fp64 as the device evaluates it (bitwise)."""
    u = np.asarray(u, dtype=np.float64)
    lower, upper = float(lower), float(upper)
    if is_log(lower, upper):
        l0, l1 = np.log10(LD(lower)), np.log10(LD(upper))
        return np.power(LD(10), l0 + u.astype(LD) * (l1 - l0))
    return u * (upper - lower) + lower


def uniforms(n, seed):
    """The five raw uniforms of the box distribution: (n, 5) fp64 in the order mass, x, y, vx, vy."""
    i = np.arange(n, dtype=np.uint64)
    r, q, w = draw(seed, i, 0), draw(seed, i, 1), draw(seed, i, 2)
    return np.stack([u01(r[0], r[1]), u01(r[2], r[3]), u01(q[0], q[1]), u01(q[2], q[3]), u01(w[0], w[1])], axis=1)


def box_exact(n, seed, lm, hm, lp, hp, lv, hv):
    """(mass, pos, vel) as sample_range returns them: extended precision where the log rule applies, fp64 where linear."""
    u = uniforms(n, seed)
    m = sample_range(u[:, 0], lm, hm)
    pos = np.stack([sample_range(u[:, 1], lp, hp), sample_range(u[:, 2], lp, hp)], axis=1)
    vel = np.stack([sample_range(u[:, 3], lv, hv), sample_range(u[:, 4], lv, hv)], axis=1)
    return m, pos, vel


def box(n, seed, lm=1e-1, hm=5e-1, lp=-1e-1, hp=1e-1, lv=-1e-4, hv=1e-4):
    """(mass, pos, vel) in fp64 (the defaults are engine.initialize's)."""
    return tuple(np.asarray(x, dtype=np.float64) for x in box_exact(n, seed, lm, hm, lp, hp, lv, hv))


def plummer_exact(n, seed, a, hp, m):
    """The projected Plummer sphere, body by body as the kernel draws it.  Returns (mass, pos, vel, tries, rad, p, gap):
    pos in extended precision, tries = draws made (1..64), rad and p = u^(-2/3) of the draw that stands (extended), gap =
    the smallest |rad / hp - 1| over every draw the body made.  A body whose 64 draws were all beyond hp keeps the last
    one: tries == 64 and rad > hp."""
    i = np.arange(n, dtype=np.uint64)
    r = draw(seed, i, 0)
    a_l, hp_l = LD(a), LD(hp)
    rad, p, cz = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n)
    phi, gap, tries = np.zeros(n), np.full(n, np.inf, LD), np.zeros(n, np.int64)
    live = np.arange(n)
    for t in range(PLUMMER_TRIES):
        if not len(live):
            break
        w = draw(seed, i[live], PLUMMER_STREAM0 + t)
        u = np.maximum(u01(w[0], w[1]), U_MIN)
        pp = np.power(u.astype(LD), LD(-2.0 / 3.0))           # the kernel's exponent is the fp64 constant
        rr = a_l / np.sqrt(pp - LD(1))
        rad[live], p[live] = rr, pp
        cz[live] = 2.0 * u01(w[2], w[3]) - 1.0                                        # exact in fp64
        phi[live] = TWO_PI * u01((r[0][live] + np.uint64(t)) & M32, r[1][live])       # one fp64 rounding, as on the device
        tries[live] = t + 1
        if np.isfinite(hp):
            gap[live] = np.minimum(gap[live], np.abs(rr / hp_l - LD(1)))
        live = live[rr > hp_l]
    s = np.sqrt(LD(1) - cz.astype(LD) ** 2) * rad
    pos = np.stack([s * np.cos(phi.astype(LD)), s * np.sin(phi.astype(LD))], axis=1)
    return np.full(n, float(m)), pos, np.zeros((n, 2)), tries, rad, p, gap


def plummer(n, seed, a, hp, m):
    """plummer_exact with pos in fp64."""
    mass, pos, vel, tries, rad, p, gap = plummer_exact(n, seed, a, hp, m)
    return mass, np.asarray(pos, dtype=np.float64), vel, tries, rad, p, gap


def exhausted(tries, rad, hp):
    """The bodies that keep a radius beyond hp after 64 rejected draws."""
    return (tries == PLUMMER_TRIES) & (rad > LD(hp))


def to_state(x, precision):
    """What the state arrays hold of x and download() hands back: fp64 unchanged, an F32 state through np.float32."""
    name = getattr(precision, "name", precision)
    if name in F32_STATE:
        return np.asarray(x).astype(np.float32).astype(np.float64)
    return np.asarray(x, dtype=np.float64)


def plummer_exhaust_probability(a, hp):
    """(1 - M(hp))^64 with M(r) = r^3 / (r^2 + a^2)^(3/2): the chance that a body ends beyond hp."""
    return (1.0 - hp ** 3 / (hp * hp + a * a) ** 1.5) ** PLUMMER_TRIES


def plummer_projected_cdf(R, a, hp):
    """P(projected radius <= R) of a Plummer sphere of scale a cut at the THREE-dimensional radius hp:
    1 - a^2 / (R^2 + a^2) * (1 - R^2 / hp^2)^(3/2).  (Mass at radius r lies beyond the cylinder R with the fraction
    sqrt(1 - R^2 / r^2); integrate that against dM = 3 a^2 r^2 / (r^2 + a^2)^(5/2) dr from R to hp and divide by M(hp).)"""
    R = np.asarray(R, dtype=np.float64)
    t = np.clip(1.0 - (R / hp) ** 2, 0.0, 1.0) if np.isfinite(hp) else 1.0
    return 1.0 - a * a / (R * R + a * a) * t ** 1.5
