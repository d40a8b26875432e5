"""The acrobot's, the cart-pole's, the pendulum's and the compass walker's kernels against the reference's OWN code, through recorded
fixtures.

tests/golden/ref_envs_{acrobot,walker,cart_pole,pendulum}.npz hold the inputs of tests/ref_env_cases.py and what oracle/_ref/ref_envs
-- the reference's acrobot.cpp, cart_pole.cpp, pendulum.cpp, SWModel.cpp and compass_walker.cpp compiled unmodified, evaluated call by
call -- answered on them;
tests/golden/ref_envs_bounds.json holds, per output group, the largest deviation of the portable-mode oracle from those answers
(tools/record_ref_envs.py; tests/test_oracle_ref_envs.py keeps all three fresh).  Nothing here reads the reference, and no number compared here comes from the oracle.

One grlx_env_step per environment on the fixture's rows: every continuous output within TWICE the recorded bound of the reference's
(the margin for a libm on the recording machine other than the one the bound was taken with; the kernels equal the portable oracle
bit for bit elsewhere in the suite, so the true deviation is the recorded one), every terminal code and strike flag equal.  One
grlx_env_start pair (first learning start, the test start after it) on a 64-replica context per environment under the same rule.
The cart-pole's rows run under the task variant each names (end-stop penalty and action penalty, each off and on: one launch per
variant on its rows), and the cart-pole and the pendulum start one context per randomization (0 and 1).
Rows are excluded only where the portable ORACLE and the reference differ in a discrete outcome (the fixture's mask, at most 1 %,
asserted by the CPU test with the oracle alone): a terminal code, the strike flag, the turn an observed angle was wrapped on.
"""
import json

import numpy as np
import pytest

from tests import configs
from tests import ref_env_cases as rc

pytestmark = pytest.mark.gpu

FACTOR = 2.0


def load(env):
    fx = np.load(rc.FIXTURE[env])
    with open(rc.BOUNDS) as f:
        return fx, json.load(f)[env]


ENVS = ["acrobot", "walker", "cart_pole", "pendulum"]


def make(grlx, env, n, variant=0):
    cfg = rc.CONFIGS[env](grlx, n)[0]
    if env == "cart_pole":
        cfg.end_stop_penalty, cfg.action_penalty = int(variant) & 1, (int(variant) >> 1) & 1
    return cfg


@pytest.mark.parametrize("env", ENVS)
def test_env_step_within_twice_the_recorded_bound_of_the_reference(grlx, env):
    fx, recorded = load(env)
    excluded = fx["excluded"]
    assert excluded.sum() <= len(excluded) // 100 and len(excluded) <= rc.MAX_ROWS
    variant = fx["variant"] if "variant" in fx.files else np.zeros(len(excluded), np.int32)
    state, obs, reward, term = fx["state"].copy(), np.zeros_like(fx["obs"]), np.zeros_like(fx["reward"]), np.zeros_like(fx["term"])
    for v in np.unique(variant):
        rows = variant == v
        state[rows], obs[rows], reward[rows], term[rows] = grlx.runner.env_step(make(grlx, env, 1, v), fx["state"][rows], fx["action"][rows])
    ref = dict(next=fx["next"], obs=fx["obs"], reward=fx["reward"], term=fx["term"])
    got = dict(next=state, obs=obs, reward=reward, term=term)
    found = rc.deviations(env, ref, got, excluded)
    print(f"{env}: deviations {found}, recorded {recorded['bounds']}")
    bad = np.nonzero(rc.discrete_mismatch(env, ref, got) & ~excluded)[0]
    assert bad.size == 0, f"terminal code or strike flag differs in rows {bad[:8]}, tags {sorted({rc.TAGS[t] for t in fx['tag'][bad]})}"
    assert rc.within(env, ref, got, excluded, recorded["bounds"], FACTOR) == []


@pytest.mark.parametrize("env", ENVS)
def test_env_start_within_twice_the_recorded_bound_of_the_reference(grlx, env):
    fx, recorded = load(env)
    n = rc.N_STARTS
    rands = rc.START_RANDOMIZATION.get(env, (None,))
    assert len(fx["start_test"]) == 2 * n * len(rands)
    for at, rand in enumerate(rands):
        cfg = make(grlx, env, n)
        cfg.projector.memory = rc.START_MEMORY
        if env == "cart_pole":                                            # the actor-critic draws a second table's initial weights
            cfg.actor_projector.memory = rc.START_MEMORY
        if rand is not None:
            cfg.randomization = rand
            assert (fx["start_randomization"][2 * n * at: 2 * n * (at + 1)] == rand).all()
        runner = grlx.Runner(cfg, rc.START_SEEDS)
        _starts_of_one_context(runner, env, fx, recorded, 2 * n * at)
        runner.close()


def _starts_of_one_context(runner, env, fx, recorded, first):
    n = rc.N_STARTS
    stream = 1 if env in rc.THREAD_LOCAL_STARTS else 0
    for test in (0, 1):
        rows = slice(first + test * n, first + (test + 1) * n)
        assert (fx["start_test"][rows] == test).all()
        before = np.array([runner.rng(k)[stream] for k in range(n)], np.uint64)
        assert (before == fx["start_position"][rows]).all(), "the context's stream is not where the fixture was recorded"
        obs = runner.env_start(test)
        x = np.array([runner.env_state(k) for k in range(n)])
        after = np.array([runner.rng(k)[stream] for k in range(n)], np.uint64)
        excluded = fx["start_excluded"][rows]
        assert excluded.sum() <= n // 100
        assert (after == fx["start_position_after"][rows])[~excluded].all(), "a start consumed another number of draws than the reference's"
        ref = dict(x=fx["start_x"][rows], obs=fx["start_obs"][rows])
        got = dict(x=x, obs=obs)
        print(f"{env} starts, test = {test}: deviations {rc.start_deviations(env, ref, got, excluded)}, recorded {recorded['start_bounds']}")
        assert (got["obs"][:, -1] == ref["obs"][:, -1])[~excluded].all()
        assert rc.starts_within(env, ref, got, excluded, recorded["start_bounds"], FACTOR) == []
