"""The acrobot's and the compass walker's kernels against the reference's OWN code, through recorded fixtures.

tests/golden/ref_envs_{acrobot,walker}.npz hold the inputs of tests/ref_env_cases.py and what oracle/_ref/ref_envs -- the reference's
acrobot.cpp, SWModel.cpp and compass_walker.cpp compiled unmodified, evaluated call by call -- answered on them;
tests/golden/ref_envs_bounds.json holds, per output group, the largest deviation of the portable-mode oracle from those answers
(tools/record_ref_envs.py; tests/test_oracle_ref_envs.py keeps all three fresh).  Nothing here reads the reference, and no number compared here comes from the oracle.

One grlx_env_step per environment on the fixture's rows: every continuous output within TWICE the recorded bound of the reference's
(the margin for a libm on the recording machine other than the one the bound was taken with; the kernels equal the portable oracle
bit for bit elsewhere in the suite, so the true deviation is the recorded one), every terminal code and strike flag equal.  One
grlx_env_start pair (first learning start, the test start after it) on a 64-replica context per environment under the same rule.
Rows are excluded only where the portable ORACLE and the reference differ in a discrete outcome (the fixture's mask, at most 1 %,
asserted by the CPU test with the oracle alone).
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


def make(grlx, env, n):
    return (configs.acrobot if env == "acrobot" else configs.compass_walker)(grlx, n)[0]


@pytest.mark.parametrize("env", ["acrobot", "walker"])
def test_env_step_within_twice_the_recorded_bound_of_the_reference(grlx, env):
    fx, recorded = load(env)
    excluded = fx["excluded"]
    assert excluded.sum() <= len(excluded) // 100
    state, obs, reward, term = grlx.runner.env_step(make(grlx, env, 1), fx["state"].copy(), fx["action"].copy())
    ref = dict(next=fx["next"], obs=fx["obs"], reward=fx["reward"], term=fx["term"])
    got = dict(next=state, obs=obs, reward=reward, term=term)
    found = rc.deviations(env, ref, got, excluded)
    print(f"{env}: deviations {found}, recorded {recorded['bounds']}")
    bad = np.nonzero(rc.discrete_mismatch(env, ref, got) & ~excluded)[0]
    assert bad.size == 0, f"terminal code or strike flag differs in rows {bad[:8]}, tags {sorted({rc.TAGS[t] for t in fx['tag'][bad]})}"
    assert rc.within(env, ref, got, excluded, recorded["bounds"], FACTOR) == []


@pytest.mark.parametrize("env", ["acrobot", "walker"])
def test_env_start_within_twice_the_recorded_bound_of_the_reference(grlx, env):
    fx, recorded = load(env)
    n = rc.N_STARTS
    cfg = make(grlx, env, n)
    cfg.projector.memory = rc.START_MEMORY
    runner = grlx.Runner(cfg, rc.START_SEEDS)
    for test in (0, 1):
        rows = slice(test * n, (test + 1) * n)
        assert (fx["start_test"][rows] == test).all()
        before = np.array([runner.rng(k)[1 if env == "acrobot" else 0] for k in range(n)], np.uint64)
        assert (before == fx["start_position"][rows]).all(), "the context's stream is not where the fixture was recorded"
        obs = runner.env_start(test)
        x = np.array([runner.env_state(k) for k in range(n)])
        after = np.array([runner.rng(k)[1 if env == "acrobot" else 0] for k in range(n)], np.uint64)
        excluded = fx["start_excluded"][rows]
        assert excluded.sum() <= n // 100
        assert (after == fx["start_position_after"][rows])[~excluded].all(), "a start consumed another number of draws than the reference's"
        ref = dict(x=fx["start_x"][rows], obs=fx["start_obs"][rows])
        got = dict(x=x, obs=obs)
        print(f"{env} starts, test = {test}: deviations {rc.start_deviations(env, ref, got, excluded)}, recorded {recorded['start_bounds']}")
        assert (got["obs"][:, -1] == ref["obs"][:, -1])[~excluded].all()
        assert rc.starts_within(env, ref, got, excluded, recorded["start_bounds"], FACTOR) == []
    runner.close()
