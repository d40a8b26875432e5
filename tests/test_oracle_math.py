"""The portable arithmetic (oracle/portable_math.c, restated for the device in grl_amd/csrc/grlx_math.h) against EXACT values.

Every GPU result of this project is compared with the oracle bit for bit, and both sides evaluate the same hand-written psin, pcos,
plog and pexp: if that shared specification were wrong, both would be wrong alike and every parity test would pass.  Here the
specification itself is held to the true functions (mpmath at 240 bits), over its whole declared domain and on the arguments where
such code goes wrong: the doubles next to a multiple of pi/2, where the three-part argument reduction cancels 60 and more bits.

The error is measured in ulp of the exact result (subnormal spacing below 2^-1022).  Bounds: 1 ulp is the documented claim; where it
does not hold the bound is the next whole number above the worst error MEASURED on these sets (the sets are samples: the supremum
may lie a little above), and DESIGN.md section 2 quotes the measured figure and its argument.  Every test prints what it measured.
"""
import math

import numpy as np
import pytest

from tests import math_cases as mc
from tests import oracle_binding as ob

mpmath = pytest.importorskip("mpmath")
mpmath.mp.prec = 240


@pytest.fixture(scope="module")
def L():
    return ob.load()


def _apply(f, x):
    return np.array([f(float(v)) for v in x])


def ulp_errors(got, x, exact_fn):
    """|got - exact_fn(x)| in ulp of the exact value, per element."""
    out = np.empty(len(x))
    for i, (g, v) in enumerate(zip(got, x)):
        exact = exact_fn(mpmath.mpf(float(v)))
        _, man, exp, bc = exact._mpf_
        ulp_exp = max(exp + bc - 53, -1074) if man else -1074
        out[i] = float(mpmath.ldexp(abs(mpmath.mpf(float(g)) - exact), -ulp_exp))
    return out


def _report(name, what, x, err):
    i = int(np.argmax(err))
    print(f"{name:10s} {what:28s} n={len(x):6d}  worst {err[i]:.4f} ulp at x = {float(x[i])!r} ({float(x[i]).hex()})  > 1/2 ulp: {100.0 * np.mean(err > 0.5):.2f} %")
    return float(err[i])


# ------------------------------------------------------------------------------------------------------ psin, pcos ---
@pytest.mark.parametrize("name,exact", [("orc_psin", "sin"), ("orc_pcos", "cos")])
def test_sin_cos_within_one_ulp_over_the_whole_domain(L, name, exact):
    f, exact_fn = getattr(L, name), getattr(mpmath, exact)
    for what, x in mc.sincos_sets().items():
        got = _apply(f, x)
        assert np.isfinite(got).all(), what
        assert _report(name, what, x, ulp_errors(got, x, exact_fn)) < 1.0, what


@pytest.mark.parametrize("name,exact", [("orc_psin", "sin"), ("orc_pcos", "cos")])
def test_sin_cos_hard_cases_keep_their_sign(L, name, exact):
    """Next to k*pi/2 one of the two functions is as small as 6e-19: a reduction that loses the third part of pi/2 returns 0 or
    the wrong sign there."""
    x = mc.hard_sincos()
    got = _apply(getattr(L, name), x)
    want = np.array([float(getattr(mpmath, exact)(mpmath.mpf(float(v)))) for v in x])
    print(f"{name}: smallest |exact result| on the hard set {np.abs(want).min():.3e}")
    assert (want != 0).all() and (got != 0).all()
    assert (np.signbit(got) == np.signbit(want)).all()


def test_sin_cos_domain_ends_at_2_to_20(L):
    for f in (L.orc_psin, L.orc_pcos):
        assert all(math.isnan(f(float(v))) for v in mc.OUTSIDE_SINCOS)
        inside = float(np.nextafter(mc.SIN_LIMIT, 0.0))
        assert math.isfinite(f(inside)) and math.isfinite(f(-inside))         # (their error: the edge set of the test above)
    assert L.orc_psin(0.0) == 0.0 and L.orc_pcos(0.0) == 1.0 and L.orc_pcos(-0.0) == 1.0


# ------------------------------------------------------------------------------------------------------------ plog ---
# measured worst 1.4985 ulp (set "1 +- 1e-3", x = 1.0000038116033731): the next whole number
PLOG_GENERAL_BOUND_ULP = 2.0


def test_log_within_one_ulp_on_the_lattice_the_kernels_use(L):
    x = mc.log_lattice()
    assert _report("orc_plog", "lattice j*2^-48", x, ulp_errors(_apply(L.orc_plog, x), x, mpmath.log)) < 1.0


def test_log_general_arguments(L):
    """Outside the drand48 lattice the documented 1 ulp does NOT hold: just above 1 the error reaches 1.47 ulp (f = m - 1 is small,
    2s + lo rounds twice).  No kernel evaluates plog there; the bound is the measured worst, rounded up."""
    worst = 0.0
    for what, x in mc.log_general().items():
        worst = max(worst, _report("orc_plog", what, x, ulp_errors(_apply(L.orc_plog, x), x, mpmath.log)))
    assert 1.0 < worst < PLOG_GENERAL_BOUND_ULP         # above 1: the documentation must not claim 1 ulp again


def test_log_special_values(L):
    assert L.orc_plog(0.0) == -math.inf and L.orc_plog(-0.0) == -math.inf
    assert math.isnan(L.orc_plog(-1.0)) and math.isnan(L.orc_plog(math.nan)) and math.isnan(L.orc_plog(-math.inf))
    assert L.orc_plog(math.inf) == math.inf
    assert L.orc_plog(1.0) == 0.0 and not math.copysign(1.0, L.orc_plog(1.0)) < 0


# ------------------------------------------------------------------------------------------------------------ pexp ---
def test_exp_within_one_ulp(L):
    for what, x in mc.exp_sets().items():
        inside = x[(x >= mc.EXP_UNDERFLOW) & (x <= mc.EXP_OVERFLOW)]
        got = _apply(L.orc_pexp, inside)
        assert np.isfinite(got).all()
        assert _report("orc_pexp", what, inside, ulp_errors(got, inside, mpmath.exp)) < 1.0, what
    sub = mc.exp_sets()["subnormal results"]
    assert (_apply(L.orc_pexp, sub) < 2.0 ** -1022).all()                       # subnormal results really are in the sets


def test_exp_thresholds(L):
    assert L.orc_pexp(float(np.nextafter(mc.EXP_OVERFLOW, np.inf))) == math.inf and math.isfinite(L.orc_pexp(mc.EXP_OVERFLOW))
    below = L.orc_pexp(float(np.nextafter(mc.EXP_UNDERFLOW, -np.inf)))
    assert below == 0.0 and not math.copysign(1.0, below) < 0
    assert L.orc_pexp(mc.EXP_UNDERFLOW) == 0.0                                  # exp(-745.2) = 0.94 * 2^-1075 rounds to zero anyway
    assert L.orc_pexp(-745.13) == 5e-324 and L.orc_pexp(-745.14) == 0.0         # ... the last subnormal ends at ln(2^-1075) = -745.1332
    assert math.isnan(L.orc_pexp(math.nan)) and L.orc_pexp(math.inf) == math.inf and L.orc_pexp(-math.inf) == 0.0
    assert L.orc_pexp(0.0) == 1.0 and L.orc_pexp(-0.0) == 1.0


# ------------------------------------------------------------------------------------------- portable against libm ---
def _ulp_distance(a, b):
    """|a - b| in units of the spacing of the larger operand."""
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_portable_differs_from_libm_by_at_most_one_ulp(L):
    """ORC_MATH_LIBM pins the reference's golden file, ORC_MATH_PORTABLE is what the GPU is compared with: on the random sets the
    two differ in the last bit of a few percent of arguments (3.1 % for sin and cos over the whole domain, 5.1 % for log on the
    drand48 lattice, with glibc 2.35) and never by more.  The share depends on the C library: only "below 10 %" is asserted.
    Both numpy's functions and the C library's own (through `math`) are compared: numpy evaluates some functions, log among
    them, with vector kernels of its own where the processor has the instructions."""
    cases = [("orc_psin", np.sin, math.sin, mc.random_sincos()), ("orc_pcos", np.cos, math.cos, mc.random_sincos()),
             ("orc_plog", np.log, math.log, {"lattice": mc.log_lattice()})]
    for name, np_fn, libm_fn, sets in cases:
        for what, x in sets.items():
            got = _apply(getattr(L, name), x)
            for lib, ref in (("numpy", np_fn(x)), ("libm", _apply(libm_fn, x))):
                d = _ulp_distance(got, ref)
                share = float(np.mean(got != ref))
                print(f"{name} vs {lib:5s} {what:18s}: differ at {100 * share:.2f} % of arguments, by at most {d.max():.0f} ulp")
                assert d.max() <= 1.0, (name, lib, what)
                assert share < 0.10, (name, lib, what)


def test_log_general_arguments_against_libm(L):
    """Where plog is off by up to 1.5 ulp (test_log_general_arguments) it cannot stay within one ulp of a library that is within
    one ulp of the truth on the other side: 2 ulp measured on (0.5, 2) and on 1 +- 1e-3.  Bound by reasoning, not by the figure:
    |plog - log| < PLOG_GENERAL_BOUND_ULP = 2 (asserted above) and |libm - log| < 1 give a distance below 3 spacings, and a
    distance between doubles is a whole number of them.  The share of differing arguments (11 % and 19 %) is printed only."""
    for what, x in mc.log_general().items():
        got = _apply(L.orc_plog, x)
        for lib, ref in (("numpy", np.log(x)), ("libm", _apply(math.log, x))):
            d = _ulp_distance(got, ref)
            print(f"orc_plog vs {lib:5s} {what:18s}: differ at {100 * float(np.mean(got != ref)):.2f} % of arguments, by at most {d.max():.0f} ulp")
            assert d.max() <= PLOG_GENERAL_BOUND_ULP, (lib, what)


# ------------------------------------------------------------------------- one environment step in both arithmetics ---
# largest component-wise difference measured between the two modes after ONE step, in units of the spacing of the larger operand
# (4000 random states each; the bound asserted is twice the measured figure, because the sample is random)
ENV_STEP_MEASURED_ULP = {"pendulum": 24, "acrobot": 8, "cart_pole": 16}


def _env_cases():
    from tests import configs
    n = 4000
    rng = np.random.default_rng(31)
    spec = configs.pendulum(None, 1)[1]
    state = np.stack([rng.uniform(-30, 30, n), rng.uniform(-40, 40, n), rng.uniform(0, 2.97, n)], axis=1)
    yield "pendulum", spec, state, rng.choice([-3.0, 0.0, 3.0], n), lambda s, spec=spec: [s[:, 2] - spec.timeout]
    spec = configs.acrobot(None, 1)[1]
    state = np.stack([np.pi + rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-15, 15, n),
                      rng.uniform(-30, 30, n), rng.uniform(0, 19.9, n)], axis=1)
    lim = 12 * np.pi / 180
    yield "acrobot", spec, state, rng.choice([-1.0, 0.0, 1.0], n), lambda s: [np.abs(s[:, 0] - np.pi) - lim, np.abs(s[:, 1]) - lim, s[:, 4] - 20.0]
    spec = configs.cart_pole_ac(None, 1)[1]
    spec.end_stop_penalty = spec.action_penalty = 1                              # so that |x| > 2.4 decides the terminal code
    state = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-20, 20, n), rng.uniform(-8, 8, n),
                      rng.uniform(-15, 15, n), rng.uniform(0, 9.97, n)], axis=1)
    yield "cart_pole", spec, state, rng.uniform(-15, 15, n), lambda s, spec=spec: [np.abs(s[:, 0]) - 2.4, s[:, 4] - spec.timeout]


def test_one_env_step_in_both_arithmetic_modes():
    """The only link between the mode the goldens pin (libm) and the mode the GPU is compared with (portable), for anything but the
    pendulum run of tests/test_oracle_golden.py.  The compass walker is left out: its heel-strike search takes discrete decisions
    (which bracket to replace, when to stop) on heights of 1e-11, and one ulp in a sine may flip them."""
    for name, spec, state, action, margins in _env_cases():
        res = {}
        for mode in (ob.MATH_LIBM, ob.MATH_PORTABLE):
            spec.math = mode
            res[mode] = ob.env_step(spec, state, action)
        a, b = res[ob.MATH_LIBM], res[ob.MATH_PORTABLE]
        close = np.zeros(len(action), bool)                                      # a terminal threshold met to within 1e-9
        for r in (a, b):
            for m in margins(r[0]):
                close |= np.abs(m) < 1e-9
        assert close.mean() < 0.01, name
        keep = ~close
        assert (a[3][keep] == b[3][keep]).all(), name
        assert len(set(a[3][keep])) > 1, name                                    # the sample does reach a terminal code
        worst = max(float(_ulp_distance(a[i][keep], b[i][keep]).max()) for i in range(3))
        print(f"{name}: dropped {int(close.sum())} of {len(action)}; state / observation / reward differ by at most {worst:.1f} ulp")
        assert worst <= 2 * ENV_STEP_MEASURED_ULP[name], name
