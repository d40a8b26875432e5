"""The oracle half of the kernel-plan cases, without a device: every launched case of tests/kernel_plan_cases.py builds a spec the oracle
accepts and that agrees with the case's grlx_config field by field (so tests/test_gpu_kernel_plan_parity.py compares a kernel with the
oracle of the SAME experiment), and the rows of the kernel table that no launched case reaches are a literal set with reasons."""
import math
import os
import re

import pytest

from tests import kernel_plan_cases as kc
from tests import oracle_binding as ob

# config field -> spec field, where the two structs spell it differently
RENAMED = {"projector.safe": "safe"}
# the scalars both halves hold; the arrays of a projector are compared over its `dims`
SHARED = ["env", "agent", "trace", "alpha", "gamma", "lambda_", "epsilon", "timeout", "control_step", "integration_steps",
          "action_min", "action_max", "action_steps", "projector.safe", "target_interval", "target_tau",
          "projector.tilings", "projector.memory", "projector.dims", "projector.resolution", "projector.wrapping",
          # beyond what chooses a row: everything else of the experiment that both structs spell out
          "test_interval", "test_trials", "randomization", "decay_rate", "decay_min", "tap_starts",
          "representation.init_min", "representation.init_max", "representation.output_min", "representation.output_max", "representation.limit"]
# read only by the graphs with a second table (actor-critic: the actor; QV: the state values) -- and by advantage learning, kappa
SECOND_TABLE = ["actor_projector.tilings", "actor_projector.memory", "actor_projector.dims", "actor_projector.resolution", "actor_projector.wrapping",
                "actor_representation.init_min", "actor_representation.init_max", "actor_representation.output_min",
                "actor_representation.output_max", "actor_representation.limit"]
AC_ONLY = ["actor_alpha", "sigma", "theta", "ac_decay_rate", "ac_decay_min", "ac_update_method", "ac_step_limit"]
ENV_ONLY = {ob.ENV_CART_POLE: ["end_stop_penalty", "action_penalty"],
            ob.ENV_COMPASS_WALKER: ["slope_angle", "initial_state_variation", "negative_reward"]}


def _get(obj, path):
    for part in path.split("."):
        obj = getattr(obj, part)
    return obj


def assert_halves_agree(cfg, spec, fields, what):
    for f in fields:
        a, b = _get(cfg, f), _get(spec, RENAMED.get(f, f))
        if hasattr(a, "__len__"):
            dims = _get(cfg, f.rsplit(".", 1)[0]).dims
            a, b = list(a[:dims]), list(b[:dims])
        assert a == b, f"{what}: {f} is {a!r} in the grlx_config and {b!r} in the oracle's spec"


_RAN = {}       # the bytes of a spec -> its two trials: cases that differ only in the kernel they choose share one oracle run


def _two_trials(spec):
    s = ob.Spec.from_buffer_copy(spec)
    s.test_interval = -1                     # a row for every trial (online_learning.cpp:160,238): both trials learn and both report
    key = bytes(s)
    if key not in _RAN:
        e = ob.Experiment(s, seed=1)         # raises where orc_create returns NULL
        try:
            _RAN[key] = [(x.trial, x.steps, x.reward) for x in e.run(2)[0]]
        finally:
            e.close()
    return _RAN[key]


@pytest.mark.parametrize("case", kc.LAUNCHED, ids=[c[0] for c in kc.LAUNCHED])
def test_every_launched_case_has_an_oracle(grlx, oracle, case):
    name, builder, n, over, flags = case[:5]
    cfg, spec = kc.build_pair(grlx, builder, n, over)
    fields = list(SHARED)
    if spec.agent in (ob.AGENT_AC, ob.AGENT_QV):
        fields += SECOND_TABLE
    if spec.agent == ob.AGENT_AC:
        fields += AC_ONLY
    if spec.agent == ob.AGENT_QV:
        fields += ["beta"]
    if spec.agent == ob.AGENT_ADVANTAGE:
        fields += ["kappa"]
    fields += ENV_ONLY.get(spec.env, [])
    assert_halves_agree(cfg, spec, fields, name)
    for k, v in over.items():                # every override reached the half (or halves) it belongs to
        if k in kc.RESULT_KEYS:
            assert _get(spec, "safe" if k == "safe" else k) == v and _get(cfg, "projector.safe" if k == "safe" else k) == v, (name, k)
        else:
            assert getattr(cfg, k) == v and not hasattr(spec, k), (name, k)
    spec.math = ob.MATH_PORTABLE
    rows = _two_trials(spec)
    assert [t for t, _, _ in rows] == [0, 1] and all(s > 0 and math.isfinite(r) for _, s, r in rows), (name, rows)


def test_build_pair_refuses_a_key_it_cannot_classify(oracle):
    with pytest.raises(KeyError, match="lambda_"):
        kc.build_pair(None, "pendulum", 5, dict(replicas_per_wave=4, lambda_=0.5))
    assert not set(kc.RESULT_KEYS) & set(kc.KERNEL_KEYS)
    assert {k for c in kc.CASES for k in c[3]} <= set(kc.RESULT_KEYS) | set(kc.KERNEL_KEYS)


def test_five_actions_keep_the_projector(grlx, oracle):
    """action_steps = 5 changes the action grid (uniform.cpp:60-95, from action_min / action_max in both halves), not the tile coding: the
    action coordinate's resolution stays that of the three-action configuration, in the library's own builder as in the spec."""
    cfg5, cfg3 = grlx.pendulum_sarsa_config(1, action_steps=5), grlx.pendulum_sarsa_config(1)
    spec = kc.build_pair(None, "pendulum", 5, dict(action_steps=5))[1]
    assert spec.action_steps == 5 and (spec.action_min, spec.action_max) == (cfg5.action_min, cfg5.action_max) == (-3.0, 3.0)
    assert list(cfg5.projector.resolution[:3]) == list(cfg3.projector.resolution[:3]) == list(spec.projector.resolution[:3])


# ---- the rows of the table that no launched case reaches, each with its reason.  A row added to grlx_kernel_table.h fails this test until it
# has a launched case in tests/kernel_plan_cases.py -- and with it a parity case -- or a reason here.
UNLAUNCHED_ROLLOUT = {
    "rollout_wide_served_kernel<GRLX_ENV_COMPASS_WALKER, SpecNone>":
        "the generic walker pair needs 384 + 160 registers: beside its server it does not fit the register file, the device runs the unserved row",
}
UNLAUNCHED_SERVER = {
    "env_server_walker_kernel<SpecNone>": "the server half of the same pair",
}


def table_rows():
    """(rollout row, server row or "") of every row of grlx_kernel_table.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grl_amd", "csrc", "grlx_kernel_table.h")
    with open(path) as f:
        return re.findall(r"^\s*\{FAM_\w+,.*?GRLX_K\((.*?)\), (?:GRLX_UNSERVED|GRLX_K\((.*?)\), k\w+)\},$", f.read(), flags=re.M)


def test_unlaunched_rows_are_named():
    rows = table_rows()
    assert len(rows) > 80
    launched_rollouts = {c[7][1] for c in kc.LAUNCHED}
    launched_servers = {c[7][2] for c in kc.LAUNCHED} - {""}
    assert {r for r, _ in rows} - launched_rollouts == set(UNLAUNCHED_ROLLOUT)
    assert {s for _, s in rows if s} - launched_servers == set(UNLAUNCHED_SERVER)
    assert launched_rollouts <= {r for r, _ in rows} and launched_servers <= {s for _, s in rows}
    # a pair is launched as a pair: the server a launched case names stands in the row of its rollout kernel
    assert {(c[7][1], c[7][2]) for c in kc.LAUNCHED if c[7][2]} <= set(rows)
    # ... and the unlaunched rows do have a case that plans them (tests/test_kernel_plan.py), so only the device's answer is missing
    planned = {c[7][1] for c in kc.CASES} | {c[7][2] for c in kc.CASES}
    assert set(UNLAUNCHED_ROLLOUT) | set(UNLAUNCHED_SERVER) <= planned
