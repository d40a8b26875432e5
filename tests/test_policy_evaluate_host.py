"""The host-side pieces of the greedy evaluation episodes (grlx_evaluate) that need no device: the reference helper on a hand-made dense
table and an episode worked out by hand, the declarations and bindings of the new entry point, and what `grlxd -E` refuses before it looks
for a device."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_helper_on_a_hand_made_table_and_a_two_step_episode():
    """A dense table in which the slots of (obs0, action 3) hold 16, those of (obs1, action -3) hold 64 and every other slot 0; the start
    state one step short of two steps before the timeout.  The helper must act 3, then -3, stop at the timeout, count no tie -- and its
    sums must be the expressions written out here on the oracle's own step results."""
    from tests import oracle_binding as ob
    from tests import policy_evaluate_ref as ev
    from tests import policy_query_ref as ref
    spec = ob.pendulum_sarsa_spec(math=ob.MATH_PORTABLE)
    spec.projector.memory = 1 << 20
    acts = ref.actions_of(spec)
    assert acts == [-3.0, 0.0, 3.0]
    # 30 rad/s: one step turns the pendulum by about three tile widths, so obs1 shares no tile (and no slot) with obs0
    start = np.array([np.pi, 30.0, spec.timeout - 1.5 * spec.control_step])
    obs0, code0 = ev.observe(spec, start)
    assert code0 == 0 and obs0.shape == (2,)
    x1, o1, r1, t1 = ob.env_step(spec, start, 3.0)
    x2, o2, r2, t2 = ob.env_step(spec, x1[0], -3.0)
    assert (int(t1[0]), int(t2[0])) == (0, 1), "the hand-made episode was meant to time out at its second step"
    w = np.zeros(spec.projector.memory)
    s0 = ob.tile_project(spec.projector, [list(obs0) + [3.0]])[0]
    s1 = ob.tile_project(spec.projector, [list(o1[0]) + [-3.0]])[0]
    at0 = set(int(s) for a in acts for s in ob.tile_project(spec.projector, [list(obs0) + [a]])[0])
    at1 = set(int(s) for a in acts for s in ob.tile_project(spec.projector, [list(o1[0]) + [a]])[0])
    assert not at0 & at1, "the two observations were meant to share no slot"
    w[s0] = 16.0
    w[s1] = 64.0
    actions = []
    ret, disc, steps, code, ties, final = ev.episode([w], spec, start, actions_out=actions)
    assert actions == [3.0, -3.0] and (steps, code, ties) == (2, 1, 0)
    assert ret == 0.0 + float(r1[0]) + float(r2[0])
    assert disc == (0.0 + 1.0 * float(r1[0])) + (1.0 * spec.gamma) * float(r2[0])
    assert final.tobytes() == x2[0].tobytes()
    # cut at max_steps: code 0 after one step, with the first step's sums
    ret, disc, steps, code, ties, final = ev.episode([w], spec, start, max_steps=1)
    assert (ret, disc, steps, code, ties) == (float(r1[0]), float(r1[0]), 1, 0, 0) and final.tobytes() == x1[0].tobytes()
    # an all-zero table: every step is a tie and the first action acts; a state already past the timeout still takes one step
    actions = []
    late = np.array([np.pi, 0.0, spec.timeout + 1.0])
    assert ev.observe(spec, late)[1] == 1
    ret, disc, steps, code, ties, _ = ev.episode([np.zeros(spec.projector.memory)], spec, late, actions_out=actions, gamma=0.5)
    assert actions == [-3.0] and (steps, code, ties) == (1, 1, 1) and ret == disc
    # a replica's own gamma
    out = ev.evaluate([w], spec, [start], gamma=0.5)
    assert out["disc"][0] == (0.0 + 1.0 * float(r1[0])) + (1.0 * 0.5) * float(r2[0]) and out["steps"][0] == 2
    # the domain exit (code 3) outranks the task's code
    assert ev.in_domain(spec, [2.0 ** 19 - 1.0, 0.0, 0.0]) and not ev.in_domain(spec, [-2.0 ** 19, 0.0, 0.0])


def test_the_evaluate_entry_point_is_declared_and_bound():
    """include/grlx.h declares grlx_evaluate with the reference lines it replaces; the binding has its signature, the package the named
    tuple and Runner.evaluate (tests/test_capi_symbols.py holds header, exports and binding to each other once the library is built)"""
    import grl_amd
    from grl_amd import capi
    with open(os.path.join(ROOT, "include", "grlx.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+grlx_evaluate\(grlx_ctx \*ctx, int first_replica, int n_replicas,\s*const double \*states", header)
    for cite in ("online_learning.cpp:172-213", "online_learning.cpp:202", "greedy.cpp:", "GRLX_MAX_EPISODE_STEPS", "2^17"):
        assert cite in header, cite
    res, args = capi._SIGS["grlx_evaluate"]
    assert len(args) == 12
    assert grl_amd.Evaluation._fields == ("ret", "disc", "steps", "terminal", "ties", "final_state")
    assert callable(grl_amd.Runner.evaluate)
    assert "#define GRLX_ABI_VERSION 2" in header
    from grl_amd import _build
    assert "grlx_evaluate.hip" in _build.SOURCES and "grlx_evaluate.hip" in _build.UNIT_DEPS


# ---- grlxd -E: refused before any device is looked for (without a GPU, a run that got as far as the device would say "no HIP device") ----
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(GOLDEN, "pendulum-sarsa-tc.yaml")


@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def run(grlxd, args, cwd):
    return subprocess.run([grlxd, "-s", "1", "-q"] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def test_grlxd_usage_mentions_the_evaluation(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-E states]" in res.stdout + res.stderr


@pytest.mark.parametrize("content,word", [(None, "could not open"), ("3.14 0 0\n1 2\n", "line 2 has 2 columns"), ("0 x 0\n", "'x' is not a finite number"),
                                          ("0 inf 0\n", "not a finite number"), ("# nothing\n\n", "no states"),
                                          ("0 0\n", "2 columns, the model's state has 3")])
def test_grlxd_evaluate_refuses_a_missing_or_malformed_file(grlxd, tmp_path, content, word):
    if content is not None:
        (tmp_path / "e.txt").write_text(content)
    res = run(grlxd, ["-r", "4", "-t", "12", "-E", "e.txt", YAML], tmp_path)
    assert res.returncode != 0 and word in res.stderr + res.stdout, res.stderr + res.stdout
    assert res.stderr.count("-E") + res.stdout.count("-E") >= 1
    assert "no HIP device" not in res.stderr + res.stdout, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*returns*"))


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-g", "2"], "pendulum-sarsa-tc.yaml", "-g 2 is not built"),
    (["-r", "1"], "pendulum-sarsa-tc.yaml", "divides by n - 1"),
    (["-r", "4"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
])
def test_grlxd_evaluate_refusals_name_their_reason(grlxd, tmp_path, args, yaml, word):
    (tmp_path / "states.txt").write_text("# angle velocity time\n3.14159 0 0\n0 0 0   # upright\n\n1 -2 1.5\n")
    res = run(grlxd, args + ["-t", "12", "-E", "states.txt", os.path.join(GOLDEN, yaml)], tmp_path)
    assert res.returncode != 0 and word in res.stderr + res.stdout, res.stderr + res.stdout
    assert "-E" in res.stderr + res.stdout
    assert "no HIP device" not in res.stderr + res.stdout, "refused only after a device was looked for"
