"""The device's portable math (grl_amd/csrc/grlx_math.h, through grlx_math) against its specification (oracle/portable_math.c),
bit for bit, on the input sets of tests/math_cases.py -- the same arrays on which tests/test_oracle_math.py holds the specification
to the exact functions.  Every FORM the kernels call is reached: the checked sine and cosine, the small-angle-aware forms of the
compass walker, the unchecked forms with their constants in registers that the rollout kernels and the environment servers call
(one of them sets the sign by an integer add), and pexp.  The sets carry the arguments where a slip in one side's argument reduction
shows: the doubles next to k*pi/2 over the whole domain |x| < 2^20 (a uniform sample does not find them)."""
import math

import numpy as np
import pytest

from tests import math_cases as mc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(a, b, what=""):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    bad = np.nonzero(bits(a) != bits(b))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.flat[bad[0]]!r} vs {b.flat[bad[0]]!r}"


_reference = {}


def want(oracle, name, key, x):
    """The oracle's values on a set: one call per element from Python, computed once per session and shared."""
    if (name, key) not in _reference:
        f = getattr(oracle, name)
        _reference[(name, key)] = np.array([f(float(v)) for v in x])
    return _reference[(name, key)]


# ---------------------------------------------------------------- math -----
@pytest.mark.parametrize("op,name,lo,hi", [(0, "orc_psin", -200.0, 200.0), (1, "orc_pcos", -200.0, 200.0),
                                           (2, "orc_plog", 1e-300, 1e3)])
def test_device_math_bit_exact(grlx, oracle, op, name, lo, hi):
    rng = np.random.default_rng(op)
    x = np.concatenate([rng.uniform(lo, hi, 200000), rng.uniform(-1e-3, 1e-3, 20000) if op < 2 else rng.uniform(0, 1, 20000) ** 8,
                        np.array([0.0, -0.0, 1e-30, 0.5, 1.0, np.pi, -np.pi, 2 * np.pi, 1e5, -1e5, 1048575.0])])
    if op == 2:
        x = np.abs(x) + 1e-308
    got = grlx.runner.device_math(op, x)
    assert_bit_equal(got, want(oracle, name, "range of the first tests", x), name)


def test_small_angle_forms_equal_the_general_ones(grlx, oracle):
    """psin_s / pcos_s / psincos_s take a short path when every lane of a wave has |x| within a quarter turn: it
    must give the bits of the general path.  Whole waves of small arguments, mixed waves, boundaries, zeros."""
    rng = np.random.default_rng(12)
    small = rng.uniform(-0.78, 0.78, 64 * 300)
    edge = np.concatenate([np.full(64, 0.0), np.full(64, -0.0), np.full(64, 0.7853981633974483), np.full(64, -0.7853981633974483),
                           np.full(64, 0.7853981633974484), np.full(64, 0.78539816339744828), np.full(64, 1e-300), np.full(64, -5e-324)])
    mixed = rng.uniform(-7, 7, 64 * 200)
    tiny = rng.uniform(-1e-9, 1e-9, 64 * 20)
    x = np.concatenate([small, edge, mixed, tiny, np.nextafter(0.7853981633974483, [0.0, 1.0] * 32)])
    want_s = want(oracle, "orc_psin", "small-angle waves of the first tests", x)
    want_c = want(oracle, "orc_pcos", "small-angle waves of the first tests", x)
    assert_bit_equal(grlx.runner.device_math(6, x), want_s, "psin_s")
    assert_bit_equal(grlx.runner.device_math(7, x), want_c, "pcos_s")
    assert_bit_equal(grlx.runner.device_math(8, x), want_s + want_c, "psincos_s")


def test_device_fmod_sqrt_exact(grlx):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-500, 500, 100000), rng.uniform(-7, 7, 100000), [0.0, -0.0, 2 * np.pi, -2 * np.pi, 1e15]])
    y = np.full_like(x, 2 * np.pi)
    assert_bit_equal(grlx.runner.device_math(3, x, y), np.fmod(x, y), "fmod")
    y2 = rng.uniform(1e-3, 50, x.size)
    assert_bit_equal(grlx.runner.device_math(3, x, y2), np.fmod(x, y2), "fmod general")
    z = rng.uniform(0, 1e6, 100000)
    assert_bit_equal(grlx.runner.device_math(4, z), np.sqrt(z), "sqrt")


def test_div6_equals_ieee_division(grlx):
    """RK4's (k1+2k2+2k3+k4)/6 (modeled.cpp:272) uses a 3-operation form proven to be correctly
    rounded; check it against the true division on random, structured and extreme inputs."""
    rng = np.random.default_rng(9)
    m = rng.integers(1 << 52, 1 << 53, 400000).astype(np.float64)          # every mantissa pattern class
    e = rng.integers(-300, 300, m.size)
    x = np.concatenate([np.ldexp(m, e - 52) * rng.choice([-1.0, 1.0], m.size), rng.uniform(-1e3, 1e3, 200000),
                        np.arange(-3000, 3000, dtype=np.float64), np.arange(1, 4000, dtype=np.float64) * (2.0 ** -60),
                        [0.0, -0.0, 1e-310, -1e-310, 5e-324, 1e308, -1e308, 6.0, 3.0, 1.0 / 3.0]])
    assert_bit_equal(grlx.runner.device_math(5, x), x / 6.0, "x/6")


def test_device_log_sqrt_for_box_muller(grlx, oracle):
    """Rand::getNormal (utils.h:120-125) = sqrt(-2 log U1) cos(2 pi U2): log on drand48 values k * 2^-48"""
    rng = np.random.default_rng(17)
    u = np.concatenate([rng.integers(1, 1 << 48, 200000).astype(np.float64) * 2.0 ** -48, [2.0 ** -48, 1 - 2.0 ** -48, 0.5]])
    got = grlx.runner.device_math(2, u)
    w = want(oracle, "orc_plog", "uniform draws of the first tests", u)
    assert_bit_equal(got, w, "plog on uniform draws")
    assert_bit_equal(grlx.runner.device_math(4, -2 * w), np.sqrt(-2 * w), "sqrt")


# ------------------------------------------------- every form, every set -----
# op -> what it must equal: (sine, cosine) weights of the oracle's values (op 8 and 12 return sine + cosine)
SIN_COS_FORMS = {0: "psin_checked", 1: "pcos_checked", 6: "psin_s", 7: "pcos_s", 8: "psincos_s", 9: "psin<false>, pinned constants",
                 10: "psin<true>, additive constants pinned", 11: "pcos, pinned constants", 12: "psincos, pinned constants"}


def _want_form(oracle, op, key, x):
    s, c = want(oracle, "orc_psin", key, x), want(oracle, "orc_pcos", key, x)
    return {0: s, 6: s, 9: s, 10: s, 1: c, 7: c, 11: c}.get(op, s + c)


@pytest.mark.parametrize("op", sorted(SIN_COS_FORMS))
def test_sin_cos_forms_on_the_uniform_and_edge_sets(grlx, oracle, op):
    for key, x in mc.sincos_sets().items():
        if key != "hard":
            assert_bit_equal(grlx.runner.device_math(op, x), _want_form(oracle, op, key, x), f"{SIN_COS_FORMS[op]} on {key}")


@pytest.mark.parametrize("op", sorted(SIN_COS_FORMS))
def test_sin_cos_forms_on_the_hard_cases(grlx, oracle, op):
    """The doubles nearest k*pi/2 with their neighbours, both signs: the 2000 worst cancellations of |x| < 2^20, every k < 4000,
    4000 random k.  This is where the third part of pi/2, or one wrong digit of the second, decides the result."""
    x = mc.hard_sincos()
    assert_bit_equal(grlx.runner.device_math(op, x), _want_form(oracle, op, "hard", x), f"{SIN_COS_FORMS[op]} on the hard cases")


@pytest.mark.parametrize("op", [6, 7, 8])
def test_small_angle_forms_wave_by_wave(grlx, oracle, op):
    """The _s forms choose their path per wave: whole waves of quarter-turn arguments (short path), whole waves of hard cases
    (general path), and waves of small arguments in which one lane alone -- 0, 31, 32 or 63 -- holds a hard case with large k."""
    x = mc.small_angle_waves()
    assert x.size % 64 == 0
    assert_bit_equal(grlx.runner.device_math(op, x), _want_form(oracle, op, "small-angle waves", x), SIN_COS_FORMS[op])


@pytest.mark.parametrize("op", [0, 1])
def test_checked_forms_return_nan_outside_the_domain(grlx, op):
    inside = np.array([np.nextafter(mc.SIN_LIMIT, 0.0), -np.nextafter(mc.SIN_LIMIT, 0.0)])
    got = grlx.runner.device_math(op, np.concatenate([mc.OUTSIDE_SINCOS, inside]))
    assert np.isnan(got[:-2]).all() and np.isfinite(got[-2:]).all()


@pytest.mark.parametrize("op", [9, 10, 11, 12])
def test_unchecked_forms_are_refused_outside_the_domain(grlx, op):
    """Ops 9 to 12 have no domain check on the device: the host lets nothing through that is outside |x| < 2^20 or not finite,
    wherever in the batch it stands."""
    for bad in mc.OUTSIDE_SINCOS:
        for x in ([bad], [0.5] * 64 + [bad], [bad] + [0.5] * 64, [0.5] * 40 + [bad] + [0.5] * 40):
            with pytest.raises(grlx.capi.GrlxError) as e:
                grlx.runner.device_math(op, np.array(x))
            assert e.value.code == grlx.capi.ERR_INVALID
    assert np.isfinite(grlx.runner.device_math(op, [np.nextafter(mc.SIN_LIMIT, 0.0), -np.nextafter(mc.SIN_LIMIT, 0.0)])).all()
    with pytest.raises(grlx.capi.GrlxError) as e:
        grlx.runner.device_math(14, [0.5])
    assert e.value.code == grlx.capi.ERR_INVALID


def _assert_same_values(got, ref, what):
    """Bit for bit, but any NaN equals any NaN (the payload is not specified)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), what
    ok = ~np.isnan(ref)
    assert_bit_equal(got[ok], ref[ok], what)


def test_device_log_on_every_set(grlx, oracle):
    for key, x in mc.log_sets().items():
        assert_bit_equal(grlx.runner.device_math(2, x), want(oracle, "orc_plog", key, x), f"plog on {key}")
    special = np.array([0.0, -0.0, -1.0, -5e-324, np.nan, np.inf, -np.inf, 1.0])
    got = grlx.runner.device_math(2, special)
    _assert_same_values(got, want(oracle, "orc_plog", "special", special), "plog special values")
    assert got[0] == -np.inf and got[1] == -np.inf and np.isnan(got[2:5]).all() and got[5] == np.inf and np.isnan(got[6])
    assert got[7] == 0.0 and not np.signbit(got[7])


def test_device_exp_on_every_set(grlx, oracle):
    """pexp is what the batch path's logistic is pinned on (pexp_batch restates it stage by stage); the scalar form is reached
    through grlx_math only."""
    for key, x in mc.exp_sets().items():
        assert_bit_equal(grlx.runner.device_math(13, x), want(oracle, "orc_pexp", key, x), f"pexp on {key}")
    special = np.array([np.nan, np.inf, -np.inf, 710.0, 1e300, -746.0, -1e300, np.nextafter(mc.EXP_OVERFLOW, np.inf), np.nextafter(mc.EXP_UNDERFLOW, -np.inf)])
    got = grlx.runner.device_math(13, special)
    _assert_same_values(got, want(oracle, "orc_pexp", "special", special), "pexp special values")
    assert math.isnan(got[0]) and (got[[1, 3, 4, 7]] == np.inf).all() and (got[[2, 5, 6, 8]] == 0.0).all() and not np.signbit(got[[2, 5, 6, 8]]).any()
    sub = grlx.runner.device_math(13, mc.exp_sets()["subnormal results"])
    assert (sub < 2.0 ** -1022).all() and (sub > 0).any()


def test_device_fmod_two_pi_over_the_whole_range(grlx):
    """pfmod(x, 2 pi) -- the observation wrap and the reward's angle -- up to the largest argument an accepted state gives it,
    2^19 + pi: next to the multiples of the TRUE 2 pi (where the states of test_gpu_env_domain.py sit) and of the DOUBLE 2 pi
    (where the quotient changes), |x| < y, x = +-y, +-0.  fmod is exact by definition: the C library's value is THE value."""
    x = mc.fmod_two_pi()
    y = np.full_like(x, mc.TWO_PI)
    got = grlx.runner.device_math(3, x, y)
    assert_bit_equal(got, np.fmod(x, y), "fmod(x, 2 pi)")
    assert (np.signbit(got) == np.signbit(x)).all()                  # the sign of x, zeros included
    # whole waves inside two periods take pfmod's one-subtraction path, mixed waves the long division: both on the same values
    inside = mc.whole_waves(x[np.abs(x) < 2 * mc.TWO_PI])
    assert inside.size >= 64
    assert_bit_equal(grlx.runner.device_math(3, inside, np.full_like(inside, mc.TWO_PI)), np.fmod(inside, mc.TWO_PI), "fmod, short path")


def test_device_fmod_at_the_ends_of_its_declared_domain(grlx):
    """Everything pfmod's header declares beyond the kernels' own use: the largest double over 2 pi and over tiny divisors,
    subnormal divisors and the smallest normal one (the device library's fmod takes over), exponent differences of 999 to 1002
    around the 1000 at which the long division hands over, an infinite divisor, and NaN for a non-finite x, a NaN, y = +-0 and
    y < 0.  Once as one batch (mixed waves: the long division) and once with every pair filling a wave of its own, so that a pair
    the one-subtraction path accepts really takes it."""
    x, y, expected = mc.fmod_edges()
    assert (np.isnan(expected) == ~(np.isfinite(x) & (y > 0))).all() and np.isnan(expected).sum() > 80
    _assert_same_values(grlx.runner.device_math(3, x, y), expected, "fmod at the ends of its domain")
    ok = ~np.isnan(expected)
    got = grlx.runner.device_math(3, x[ok], y[ok])
    assert (np.signbit(got) == np.signbit(x[ok])).all()              # the sign of x, zeros included
    _assert_same_values(grlx.runner.device_math(3, np.repeat(x, 64), np.repeat(y, 64)), np.repeat(expected, 64), "fmod, one pair per wave")
