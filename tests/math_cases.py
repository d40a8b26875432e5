"""Input sets for the portable math (psin, pcos, plog, pexp, pfmod), shared by tests/test_oracle_math.py (the specification
against exact values, on the CPU) and tests/test_gpu_math.py (the device against the specification): both see the same arrays.

Plain integers and numpy only (no multi-precision library: the GPU tests use these sets too).  Every set is built once and cached;
callers must not modify the arrays they get.
"""
import functools

import numpy as np

# floor(pi/2 * 2^192): pi/2 to 192 fractional bits.  k * pi/2 for k < 2^20 is then known to better than 2^-170, far below the
# 2^-53 * 2^-61 that separates the hardest double of the domain from its multiple of pi/2.
PIO2_BITS = 192
PIO2_INT = 0x1921fb54442d18469898cc51701b839a252049c1114cf98e8

SIN_LIMIT = 2.0 ** 20                               # psin / pcos: |x| < 2^20
K_MAX = (1 << (20 + PIO2_BITS)) // PIO2_INT         # floor(2^20 * 2/pi) = 667544


def _nearest(n, frac_bits):
    """(the double nearest n / 2^frac_bits, |double - n / 2^frac_bits| * 2^frac_bits) by round-to-nearest-even on integers."""
    shift = n.bit_length() - 53
    q, rem = n >> shift, n & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
        rem -= 1 << shift
    return float(np.ldexp(float(q), shift - frac_bits)), abs(rem)


def nearest_multiple(k, unit_int=PIO2_INT):
    """The double nearest k * unit (unit = unit_int / 2^192; pi/2 by default)."""
    return _nearest(k * unit_int, PIO2_BITS)[0]


@functools.lru_cache(maxsize=None)
def _all_quarter_turns():
    """For every k in 1..K_MAX: the double nearest k*pi/2 and its distance from k*pi/2 (in units of 2^-192)."""
    near = np.empty(K_MAX + 1)
    dist = np.empty(K_MAX + 1)
    near[0], dist[0] = 0.0, np.inf
    for k in range(1, K_MAX + 1):
        n = k * PIO2_INT
        shift = n.bit_length() - 53
        q, rem = n >> shift, n & ((1 << shift) - 1)
        if rem > (1 << (shift - 1)):                 # (a tie cannot happen: pi/2 is irrational and known to 192 bits)
            q += 1
            rem = (1 << shift) - rem
        near[k] = q * 2.0 ** (shift - PIO2_BITS)     # q < 2^53 + 1: exact
        dist[k] = float(rem)
    return near, dist


@functools.lru_cache(maxsize=None)
def hard_k():
    """The k of the hard set: the 2000 whose nearest double lies closest to k*pi/2 (the worst cancellations of the whole domain),
    every k < 4000, and 4000 random ones."""
    _, dist = _all_quarter_turns()
    closest = np.argsort(dist)[:2000]
    rnd = np.random.default_rng(2020).integers(1, K_MAX + 1, 4000)
    return np.unique(np.concatenate([closest, np.arange(1, 4000), rnd])).astype(np.int64)


def _with_neighbours_and_negatives(d):
    x = np.concatenate([d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf)])
    x = np.concatenate([x, -x])
    return x[np.abs(x) < SIN_LIMIT]


@functools.lru_cache(maxsize=None)
def hard_sincos():
    """Doubles nearest k*pi/2, their two neighbours, and the negatives of all three, for the k of hard_k()."""
    near, _ = _all_quarter_turns()
    return _with_neighbours_and_negatives(near[hard_k()])


@functools.lru_cache(maxsize=None)
def hardest_quarter_turns(count=64, min_k=100000):
    """The `count` doubles nearest to a multiple k*pi/2 among those with k >= min_k, hardest first."""
    near, dist = _all_quarter_turns()
    order = np.argsort(dist)
    return near[order[order >= min_k][:count]]


@functools.lru_cache(maxsize=None)
def random_sincos():
    """name -> 50 000 uniform draws: the whole domain, the range the environments' tests use, one octant."""
    rng = np.random.default_rng(2021)
    return {"2^20": rng.uniform(-SIN_LIMIT, SIN_LIMIT, 50000), "200": rng.uniform(-200.0, 200.0, 50000),
            "pi/4": rng.uniform(-np.pi / 4, np.pi / 4, 50000)}


@functools.lru_cache(maxsize=None)
def edge_sincos():
    q = nearest_multiple(1) / 2                      # the double nearest pi/4 (halving is exact)
    around = [np.nextafter(np.nextafter(q, 0.0), 0.0), np.nextafter(q, 0.0), q, np.nextafter(q, 1.0), np.nextafter(np.nextafter(q, 1.0), 1.0)]
    pos = np.array([0.0, 5e-324, 1e-300, 2.0 ** -27, np.nextafter(SIN_LIMIT, 0.0)] + around)
    return np.concatenate([pos, -pos])


def sincos_sets():
    """name -> array: every in-domain sine / cosine set."""
    out = {"hard": hard_sincos(), "edge": edge_sincos()}
    out.update({"uniform " + k: v for k, v in random_sincos().items()})
    return out


OUTSIDE_SINCOS = np.array([SIN_LIMIT, -SIN_LIMIT, np.nextafter(SIN_LIMIT, np.inf), -np.nextafter(SIN_LIMIT, np.inf), 1e7, -1e300,
                           np.inf, -np.inf, np.nan])


# ---------------------------------------------------------------------------------------------------------- plog ---
@functools.lru_cache(maxsize=None)
def log_lattice():
    """What Box-Muller feeds plog: drand48 values j * 2^-48.  50 000 random j, the 3000 nearest below 1, and 2^-48 itself."""
    rng = np.random.default_rng(2022)
    j = np.concatenate([rng.integers(1, 1 << 48, 50000), (1 << 48) - np.arange(1, 3001), [1]])
    return j.astype(np.float64) * 2.0 ** -48         # j < 2^48: exact


@functools.lru_cache(maxsize=None)
def log_general():
    """name -> array: plog outside the values the kernels feed it."""
    rng = np.random.default_rng(2023)
    # one mantissa draw in each of 4000 random binades: biased exponent 0 (subnormal) .. 2046, 52 random mantissa bits
    e = rng.integers(0, 2047, 4000).astype(np.uint64)
    e[:8] = [0, 0, 0, 0, 1, 1, 2046, 2046]           # both ends of the exponent range are always in
    m = rng.integers(0, 1 << 52, 4000).astype(np.uint64)
    binades = ((e << np.uint64(52)) | m).view(np.float64)
    binades = binades[binades > 0]
    return {"uniform (0.5, 2)": rng.uniform(0.5, 2.0, 50000), "1 +- 1e-3": rng.uniform(1 - 1e-3, 1 + 1e-3, 50000),
            "binades": binades, "extremes": np.array([5e-324, np.finfo(np.float64).max, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)])}


def log_sets():
    out = {"lattice": log_lattice()}
    out.update(log_general())
    return out


# ---------------------------------------------------------------------------------------------------------- pexp ---
EXP_OVERFLOW = 709.782712893384                      # pexp: x > this -> +inf
EXP_UNDERFLOW = -745.2                               # pexp: x < this -> +0


def _around(v, n=2):
    out = [v]
    lo = hi = v
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def exp_sets():
    rng = np.random.default_rng(2024)
    ln2_half = float.fromhex("0x1.62e42fefa39efp-2")                 # RN(ln2 / 2): where the reduction's k changes
    edges = _around(ln2_half) + _around(-ln2_half) + _around(EXP_OVERFLOW) + _around(EXP_UNDERFLOW) + [0.0, -0.0, 5e-324, -5e-324]
    return {"uniform [-745.2, 709.78]": rng.uniform(-745.2, 709.78, 50000), "uniform +-1": rng.uniform(-1.0, 1.0, 50000),
            "subnormal results": rng.uniform(-745.2, -708.4, 5000), "edges": np.array(edges)}


# --------------------------------------------------------------------------------------------------------- pfmod ---
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")                   # the only divisor the kernels use: RN(2 pi)


@functools.lru_cache(maxsize=None)
def fmod_two_pi():
    """x for pfmod(x, 2 pi) over the whole range the environments can reach (|angle| < 2^19, plus the pi the observation adds):
    doubles nearest k * 2pi with their neighbours and both signs, |x| < y, x = +-y, +-0."""
    rng = np.random.default_rng(2025)
    kmax = int((2.0 ** 19 + np.pi) / (2 * np.pi))
    k = np.unique(np.concatenate([np.arange(1, 2000), rng.integers(1, kmax + 1, 4000), [kmax]]))
    d = np.array([nearest_multiple(4 * int(i)) for i in k])          # k * 2 pi = 4k * pi/2, from the TRUE pi
    e = k.astype(np.float64) * TWO_PI                                # ... and from the DOUBLE 2 pi, which is what fmod divides by
    big = np.concatenate([d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf), e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)])
    big = big[big <= 2.0 ** 19 + np.pi]
    small = np.concatenate([rng.uniform(0, TWO_PI, 4000), [0.0, 5e-324, TWO_PI, np.nextafter(TWO_PI, 0.0), np.nextafter(TWO_PI, 7.0),
                                                           2 * TWO_PI, np.nextafter(2 * TWO_PI, 0.0), np.nextafter(2 * TWO_PI, 13.0), 2.0 ** 19, 2.0 ** 19 + np.pi]])
    x = np.concatenate([big, small])
    return np.concatenate([x, -x])


@functools.lru_cache(maxsize=None)
def fmod_edges():
    """(x, y, expected) at the ends of pfmod's declared domain (grl_amd/csrc/grlx_math.h): any finite x and any y > 0, infinity
    included, give C's fmod -- exact by definition, so numpy's value is THE value; a non-finite x, a NaN, or y <= 0 (either zero;
    this is where pfmod departs from C's fmod, which takes |y|) give NaN.  The divisors: 2 pi, the smallest subnormal, the largest
    subnormal, the smallest normal 2^-1022, tiny, ordinary, huge, the largest double, infinity.  The dividends: zeros, the smallest
    subnormal, the neighbourhood of y and of 2 y (where the one-subtraction path ends), +-the largest double, and for every finite
    divisor the powers of two and random mantissas at exponent differences 999 to 1002 -- pfmod divides by itself up to a
    difference of 1000 and hands anything beyond, or a subnormal divisor, to the device library's fmod."""
    rng = np.random.default_rng(2027)
    big, tiny_sub, big_sub, small_norm = np.finfo(np.float64).max, 5e-324, np.nextafter(2.0 ** -1022, 0.0), 2.0 ** -1022
    ys = [TWO_PI, tiny_sub, 3 * tiny_sub, big_sub, small_norm, np.nextafter(small_norm, 1.0), 1e-300, 1e-3, 1.0, 3.0, 1e300, big, np.inf]
    x, y = [], []
    with np.errstate(over="ignore"):                                 # 2 * the largest double, and its upper neighbour
        for d in ys:
            xs = [0.0, tiny_sub, 1.0, 1e15, big, np.nextafter(big, 0.0), 2.0 ** 1000, 0.75 * 2.0 ** 1001]
            if np.isfinite(d):
                for m in (d, 2 * d, 3 * d, 0.5 * d, 1.5 * d):                 # (whatever overflows is dropped below)
                    xs += _around(m, 1)
                for diff in (999, 1000, 1001, 1002):                          # x / d near 2^diff, where it is representable
                    e = np.frexp(d)[1] + diff
                    if e <= 1024:
                        top = np.ldexp(0.5, e)                                # 2^(e-1): the exponent of d, plus diff
                        xs += [top, np.nextafter(top, 0.0), np.nextafter(top, np.inf)] + list(top * rng.uniform(1.0, 2.0, 4))
            xs = np.array(xs)
            xs = xs[np.isfinite(xs)]
            x += [xs, -xs]
            y += [np.full(2 * xs.size, d)]
    # outside the domain: NaN.  Non-finite x with every divisor; y = +-0, y < 0, NaN with several x
    for d in ys:
        x += [np.array([np.inf, -np.inf, np.nan])]
        y += [np.full(3, d)]
    for d in (0.0, -0.0, -tiny_sub, -TWO_PI, -1.0, -big, -np.inf, np.nan):
        xs = np.array([0.0, -0.0, 1.0, -7.0, 2.0 ** 19, big, -big, np.inf, np.nan])
        x += [xs]
        y += [np.full(xs.size, d)]
    x, y = np.concatenate(x), np.concatenate(y)
    inside = np.isfinite(x) & (y > 0)
    with np.errstate(invalid="ignore"):
        expected = np.where(inside, np.fmod(x, np.where(inside, y, 1.0)), np.nan)
    return x, y, expected


# ------------------------------------------------------------------------------------------------------- helpers ---
def whole_waves(x, wave=64):
    """x cut to a whole number of waves."""
    return x[: (x.size // wave) * wave]


@functools.lru_cache(maxsize=None)
def small_angle_waves():
    """Waves (64 consecutive values) for the small-angle-aware forms, which decide per WAVE: whole waves of quarter-turn arguments
    (the short path), whole waves of hard cases (the general path), and waves of small arguments in which exactly one lane --
    0, 31, 32 or 63 -- holds a hard case with large k (one lane must take the whole wave to the general path)."""
    rng = np.random.default_rng(2026)
    q = nearest_multiple(1) / 2
    small = rng.uniform(-q, q, 64 * 40)
    hard = whole_waves(rng.permutation(hard_sincos()))[: 64 * 40]
    lone = []
    hardest = hardest_quarter_turns(16)
    for i, lane in enumerate([0, 31, 32, 63] * 4):
        w = rng.uniform(-q, q, 64)
        w[lane] = hardest[i] * (1 if i % 2 == 0 else -1)
        lone.append(w)
    return np.concatenate([small, hard] + lone)
