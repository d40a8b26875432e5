"""grlx_env_step across each environment's whole domain, and GRLX_ERR_DOMAIN at its edge.

The four *_env_step_bit_exact tests of tests/test_gpu_parity.py keep their angles within +-40; here the angles run up to the bound
Env<ENV>::in_domain accepts (pendulum and cart-pole 2^19, acrobot 2^18 for both angles, compass walker |SLA|, |HA| < 8 and
|SLAR| < 1e6) and sit on the doubles nearest k*pi/2 and k*2pi, which takes the sines' argument reduction, the observation wrap
pfmod(x + pi, 2 pi) and the rewards' pfmod(|x|, 2 pi) to large arguments.  Everything is compared with the oracle in portable
arithmetic, bit for bit.  The bound itself is a status flag and an error code: nothing here faults, and every value is finite.

The oracle's checked sines return NaN outside |x| < 2^20, the device's unchecked ones an unspecified number: a state that the oracle
steps to a finite state inside the bound has had every sine evaluated inside its domain, and must give the same bits on the device;
any other state must give GRLX_ERR_DOMAIN.
"""
import numpy as np
import pytest

from tests import configs
from tests import math_cases as mc
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

SLA, HA, SLAR = 0, 1, 2                      # compass walker: stance leg angle, hip angle, stance leg rate (compass_walker.h:40-42)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(a, b, what=""):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    bad = np.nonzero(bits(a) != bits(b))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.flat[bad[0]]!r} vs {b.flat[bad[0]]!r}"


# name -> (guarded components, their bounds): Env<ENV>::in_domain, grl_amd/csrc/grlx_envs.h
GUARD = {"pendulum": {0: 2.0 ** 19}, "cart_pole": {1: 2.0 ** 19}, "acrobot": {0: 2.0 ** 18, 1: 2.0 ** 18}, "walker": {SLA: 8.0, HA: 8.0, SLAR: 1e6}}


def make(grlx, name):
    if name == "pendulum":
        return configs.pendulum(grlx, 1)
    if name == "cart_pole":
        return configs.cart_pole_ac(grlx, 1, end_stop_penalty=1, action_penalty=1)
    if name == "acrobot":
        return configs.acrobot(grlx, 1)
    return configs.compass_walker(grlx, 1)


def base_states(name, n, rng):
    """States and actions from the ranges of the existing *_env_step_bit_exact tests (far inside the domain)."""
    if name == "pendulum":
        return np.stack([rng.uniform(-30, 30, n), rng.uniform(-40, 40, n), rng.uniform(0, 2.8, n)], axis=1), rng.choice([-3.0, 0.0, 3.0], n)
    if name == "cart_pole":
        return np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-15, 15, n),
                         rng.uniform(0, 9.8, n)], axis=1), rng.uniform(-15, 15, n)
    if name == "acrobot":
        return np.stack([np.pi + rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-15, 15, n), rng.uniform(-30, 30, n),
                         rng.uniform(0, 19.8, n)], axis=1), rng.choice([-1.0, 0.0, 1.0], n)
    state = np.zeros((n, 11))
    state[:, :4] = np.array([0.1534, 2.0 * 0.1534, -0.1561, -0.0073]) * (1 + rng.uniform(-0.2, 0.2, (n, 4)))
    state[:, 6] = -np.sin(state[:, 0])
    state[:, 10] = 100.0
    return state, rng.choice([-1.2, 0.0, 1.2], n)


def compare_steps(grlx, cfg, spec, state, action, steps=1, what=""):
    """grlx_env_step returns OK (it raises otherwise) and gives the oracle's bits, `steps` times in a chain."""
    for it in range(steps):
        gs, gobs, grew, gterm = grlx.runner.env_step(cfg, state, action)
        os_, oobs, orew, oterm = ob.env_step(spec, state, action)
        assert np.isfinite(os_).all(), what
        assert_bit_equal(gs, os_, f"{what} state, step {it}"); assert_bit_equal(gobs, oobs, f"{what} obs, step {it}")
        assert_bit_equal(grew, orew, f"{what} reward, step {it}"); assert (gterm == oterm).all(), what
        state = gs
    return state


def expect_domain_error(grlx, cfg, state, action):
    with pytest.raises(grlx.capi.GrlxError) as e:
        grlx.runner.env_step(cfg, state, action)
    assert e.value.code == grlx.capi.ERR_DOMAIN


# ------------------------------------------------------------------------------------------------- large angles ---
# How far the angles go: "just below the bound, with room for one step's motion" (three chained steps here).
#   pendulum, acrobot: rates stay below 50 rad/s, three steps move an angle by less than 5: 16 below the bound.
#   compass walker: the model wraps both angles into [-pi, pi) after every sub-step: 7.5.
#   cart-pole: 2^14.  Its equations read the ANGLE where the pole's rate belongs (cart_pole.cpp:65, reproduced on purpose), so
#     the pole accelerates by up to (15 + 0.05 theta^2) / 1.1 / 0.62 = 0.073 theta^2 rad/s^2: at theta = 2^14 three steps
#     (0.15 s) move it by up to 0.073 * 2^28 * 0.15^2 / 2 = 2.2e5, which leaves it below 2^19; from 2^17 on ONE step can take a
#     stage past 2^20 (test_cart_pole_from_2_to_14_to_the_bound, which covers the rest of the way to the bound one step at a time).
TOP = {"pendulum": 2.0 ** 19 - 16, "acrobot": 2.0 ** 18 - 16, "cart_pole": 2.0 ** 14, "walker": 7.5}


def special_angles(top, n, rng):
    """Doubles nearest k*pi/2 and k*2pi (= 4k * pi/2) with the largest k that `top` allows, both signs."""
    kmax = int(top / (np.pi / 2))
    k = np.concatenate([rng.integers(max(1, kmax // 2), kmax + 1, n // 2), 4 * rng.integers(max(1, kmax // 8), kmax // 4 + 1, n - n // 2)])
    return np.array([mc.nearest_multiple(int(i)) for i in k]) * rng.choice([-1.0, 1.0], n)


@pytest.mark.parametrize("name,n", [("pendulum", 2000), ("acrobot", 2000), ("cart_pole", 2000), ("walker", 1000)])
def test_env_step_bit_exact_up_to_the_domain_bound(grlx, name, n):
    cfg, spec = make(grlx, name)
    rng = np.random.default_rng(41)
    state, action = base_states(name, n, rng)
    top = TOP[name]
    for c in GUARD[name]:
        if name == "walker" and c == SLAR:
            continue                                                   # a rate, not an angle: the existing tests' range
        mag = np.exp(rng.uniform(np.log(1e-3), np.log(top), n))       # log-uniform magnitude, both signs
        state[:, c] = mag * rng.choice([-1.0, 1.0], n)
        state[: n // 4, c] = special_angles(top, n // 4, rng)
        assert (np.abs(state[:, c]) <= top).all() and np.abs(state[:, c]).max() > 0.9 * top
    final = compare_steps(grlx, cfg, spec, state, action, steps=3, what=name)
    for c, bound in GUARD[name].items():
        assert (np.abs(final[:, c]) < bound).all()


def test_cart_pole_from_2_to_14_to_the_bound(grlx):
    """The rest of the cart-pole's domain, |theta| in [2^14, 2^19), one step at a time: its pole moves by up to 9e-5 theta^2 in
    a step (TOP above), so up here a step may leave the domain, and which states do is the oracle's word: a next state that is
    finite and inside the bound has had every sine inside its domain (the oracle's checked sines return NaN outside it) and must
    give the same bits on the device; every other state must give GRLX_ERR_DOMAIN.
    From |theta| >= 2^17 one step can take an RK4 stage beyond 2^20 -- where the device's unchecked sine is unspecified -- and
    still end below 2^19: looking at step ends alone lets such a step pass as OK (4 % of uniform states in [2^17, 2^19)).
    grlx_env_step therefore checks the stage arguments themselves."""
    cfg, spec = make(grlx, "cart_pole")
    rng = np.random.default_rng(43)
    n = 2000
    state, action = base_states("cart_pole", n, rng)
    mag = np.exp(rng.uniform(np.log(2.0 ** 14), np.log(2.0 ** 19), n))                    # log-uniform magnitude, both signs
    state[:, 1] = mag * rng.choice([-1.0, 1.0], n)
    quarter_turns = rng.integers(int(2.0 ** 14 / (np.pi / 2)) + 1, int(2.0 ** 19 / (np.pi / 2)), n // 4)
    state[: n // 4, 1] = np.array([mc.nearest_multiple(int(k)) for k in quarter_turns]) * rng.choice([-1.0, 1.0], n // 4)
    assert ((np.abs(state[:, 1]) >= 2.0 ** 14) & (np.abs(state[:, 1]) < 2.0 ** 19)).all()
    nxt = ob.env_step(spec, state, action)[0]
    left_sine_domain = np.isnan(nxt).any(axis=1)
    beyond_bound = ~left_sine_domain & ~(np.abs(nxt[:, 1]) < 2.0 ** 19)
    good = ~left_sine_domain & ~beyond_bound
    assert left_sine_domain.sum() > 100 and beyond_bound.sum() > 20 and good.sum() > 500
    for octave in range(14, 19):                                                           # accepted states all the way up
        assert (good & (np.abs(state[:, 1]) >= 2.0 ** octave) & (np.abs(state[:, 1]) < 2.0 ** (octave + 1))).sum() > 100
    compare_steps(grlx, cfg, spec, state[good], action[good], what="cart-pole, |theta| in [2^14, 2^19)")
    g = np.nonzero(good)[0][:64]
    for bad in list(np.nonzero(left_sine_domain)[0][:12]) + list(np.nonzero(beyond_bound)[0][:4]):
        for at in (0, 63, 64):
            idx = np.insert(g, at, bad)
            expect_domain_error(grlx, cfg, state[idx], action[idx])


# ---------------------------------------------------------------------------------------------------- the bound ---
def inward(name, c, sign):
    """(component -> value, action): rate and action that move component c away from sign * bound within the step."""
    if name == "pendulum":
        return {1: -sign * 40.0}, -sign * 3.0
    if name == "acrobot":
        return {2 + c: -sign * 10.0}, 0.0
    if name == "cart_pole":
        return {3: -sign * 15.0}, -sign * 15.0       # (the oracle steps this one to theta = -+3.6e5, finite: every sine inside its domain)
    return {(SLAR if c == SLA else 3): -sign * 0.15}, 0.0


BOUND_CASES = [(name, c) for name in ("pendulum", "cart_pole", "acrobot", "walker") for c in GUARD[name]]


@pytest.mark.parametrize("name,c", BOUND_CASES)
def test_domain_bound(grlx, name, c):
    """Batches of 65 states (a second wave exists) with the offending state at index 0, 63 or 64.
    (a) the guarded component equals the bound: GRLX_ERR_DOMAIN.  (b) it is nextafter(bound, 0) and moves inward: OK, the
    oracle's bits.  (d) the 64 in-domain states of a failing batch alone: the oracle's bits.
    The compass walker's SLAR is a RATE bound: at nextafter(1e6, 0) the stance leg turns by 1e4 rad per sub-step and |SLA| < 8
    fails at the step's end whatever the action -- no state at that bound steps to an accepted one, and (b) for it asserts
    GRLX_ERR_DOMAIN, which is what the guard has to answer there; the rates that do step to an accepted state are in
    test_walker_stance_leg_rates_up_to_the_bound."""
    cfg, spec = make(grlx, name)
    bound = GUARD[name][c]
    rng = np.random.default_rng(47 + c)
    state, action = base_states(name, 65, rng)
    compare_steps(grlx, cfg, spec, state, action, what=f"{name}: the 65 base states")
    for at in (0, 63, 64):
        for sign in (1.0, -1.0):
            s, a = state.copy(), action.copy()
            s[at, c] = sign * bound                                                        # (a)
            expect_domain_error(grlx, cfg, s, a)
            s[at, c] = sign * np.nextafter(bound, 0.0)                                     # (b)
            moves, a[at] = inward(name, c, sign)
            for k, v in moves.items():
                s[at, k] = v
            if name == "walker" and c == SLAR:
                expect_domain_error(grlx, cfg, s, a)
            else:
                final = compare_steps(grlx, cfg, spec, s, a, what=f"{name}: component {c} just inside {sign * bound}")
                assert abs(final[at, c]) < abs(s[at, c])
        rest = np.delete(np.arange(65), at)                                                # (d)
        compare_steps(grlx, cfg, spec, state[rest], action[rest], what=f"{name}: the batch without state {at}")


def test_walker_stance_leg_rates_up_to_the_bound(grlx):
    """The OK side of the compass walker's rate guard.  No state near |SLAR| = 1e6 steps to an accepted one (test_domain_bound),
    so the rates run log-uniformly from 1 rad/s to the bound and the oracle sorts them, as for the cart-pole: a sub-step is 0.01 s
    and wraps an angle by one turn at most, so the stance leg leaves |SLA| < 8 from about 650 rad/s, and the hip, which the stance
    leg whirls round, leaves |HA| < 8 at most rates above 300.  The states the oracle accepts -- rates of several hundred rad/s
    among them, with sines of the hip's angle at arguments of hundreds on the way -- must give its bits; the others
    GRLX_ERR_DOMAIN."""
    cfg, spec = make(grlx, "walker")
    rng = np.random.default_rng(59)
    n = 1000
    state, action = base_states("walker", n, rng)
    state[:, SLAR] = np.exp(rng.uniform(0.0, np.log(GUARD["walker"][SLAR]), n)) * rng.choice([-1.0, 1.0], n)
    assert (np.abs(state[:, SLAR]) < GUARD["walker"][SLAR]).all() and np.abs(state[:, SLAR]).max() > 0.9 * GUARD["walker"][SLAR]
    nxt = ob.env_step(spec, state, action)[0]
    good = np.isfinite(nxt).all(axis=1) & (np.abs(nxt[:, SLA]) < 8.0) & (np.abs(nxt[:, HA]) < 8.0) & (np.abs(nxt[:, SLAR]) < GUARD["walker"][SLAR])
    fast = np.abs(state[:, SLAR]) > 100.0
    assert good.sum() > 300 and (good & fast).sum() > 20 and (~good).sum() > 300
    compare_steps(grlx, cfg, spec, state[good], action[good], what="compass walker, |SLAR| up to 1e6")
    g = np.nonzero(good)[0][:64]
    rejected = np.nonzero(~good)[0]
    for bad in list(rejected[np.argsort(np.abs(state[rejected, SLAR]))][[0, 1, 2, -3, -2, -1]]) + list(rejected[:6]):
        for at in (0, 63, 64):
            idx = np.insert(g, at, bad)
            expect_domain_error(grlx, cfg, state[idx], action[idx])


@pytest.mark.parametrize("name", ["pendulum", "cart_pole"])
def test_step_that_crosses_the_bound(grlx, name):
    """(c) the angle sits a little below the bound with a positive rate and the step itself carries it across (or, for the
    cart-pole, takes a stage out of the sine's domain on the way): GRLX_ERR_DOMAIN.  The oracle confirms the premise."""
    cfg, spec = make(grlx, name)
    c, bound = next(iter(GUARD[name].items()))
    rng = np.random.default_rng(53)
    state, action = base_states(name, 65, rng)
    for sign in (1.0, -1.0):
        crossing = None
        for act in (0.0, 3.0, -3.0, 1.5, -1.5):                       # the first action under which the oracle's step leaves the domain
            s = state[0].copy()
            s[c] = sign * (bound - 0.25)
            s[1 if name == "pendulum" else 3] = sign * (40.0 if name == "pendulum" else 15.0)
            nxt = ob.env_step(spec, [s], [act])[0][0]
            if np.isnan(nxt).any() or not abs(nxt[c]) < bound:
                crossing = (s, act)
                break
        assert crossing is not None
        for at in (0, 63, 64):
            s, a = state.copy(), action.copy()
            s[at], a[at] = crossing
            expect_domain_error(grlx, cfg, s, a)
