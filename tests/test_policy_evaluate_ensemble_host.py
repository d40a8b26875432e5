"""The host-side pieces of the ensemble evaluation episodes (grlx_evaluate_ensemble) that need no device: the reference helper on three
hand-made dense tables and two episodes worked out by hand, the declaration and bindings of the entry point, and what `grlxd -V` refuses
before it looks for a device."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(GOLDEN, "pendulum-sarsa-tc.yaml")


def test_reference_helper_on_three_hand_made_tables():
    """Three members, every slot 0 but these (Q = the value where all 16 slots hold it):
         at obs0 (the start):             member 0 and 1: Q(obs0, -3) = 1            member 2: Q(obs0, +3) = 10
         at obs1 (after -3 from there):   member 0: Q(obs1, 0) = 5, member 1: Q(obs1, +3) = 5, member 2: nothing (all three actions tie)
       Step 1: votes [2, 0, 1] take -3, the summed Q [2, 0, 10] takes +3 -- the two rules part at the first step.
       VOTE, step 2 at obs1: votes [1, 1, 1], a three-way tie: the first action acts, ties = 1, member 2's own tie counts once.
       MEAN_Q, step 2 at the observation after +3, where every table is 0: every member ties, votes [3, 0, 0], summed Q [0, 0, 0] ties.
       The start is a step and a half before the timeout: both episodes have two steps and time out."""
    from tests import oracle_binding as ob
    from tests import policy_evaluate_ensemble_ref as ens
    from tests import policy_evaluate_ref as ev
    from tests import policy_query_ref as ref
    spec = ob.pendulum_sarsa_spec(math=ob.MATH_PORTABLE)
    spec.projector.memory = 1 << 20
    acts = ref.actions_of(spec)
    assert acts == [-3.0, 0.0, 3.0]
    # 30 rad/s: one step turns the pendulum by about three tile widths, so the observations of the two steps share no tile
    start = np.array([np.pi, 30.0, spec.timeout - 1.5 * spec.control_step])
    obs0, _ = ev.observe(spec, start)
    xm, om, rm, tm = ob.env_step(spec, start, -3.0)         # after -3: the vote's way
    xp, op, rp, tp = ob.env_step(spec, start, 3.0)          # after +3: the mean's way
    xm2, _, rm2, tm2 = ob.env_step(spec, xm[0], -3.0)
    xp2, _, rp2, tp2 = ob.env_step(spec, xp[0], -3.0)
    assert (int(tm[0]), int(tp[0]), int(tm2[0]), int(tp2[0])) == (0, 0, 1, 1), "both episodes were meant to time out at their second step"

    def slots(obs, a):
        return [int(s) for s in ob.tile_project(spec.projector, [list(obs) + [a]])[0]]

    def every(obs):
        return set(s for a in acts for s in slots(obs, a))

    assert not every(obs0) & every(om[0]) and not every(obs0) & every(op[0]) and not every(om[0]) & every(op[0]), \
        "the three observations were meant to share no slot"
    assert all(len(set(slots(o, a))) == 16 for o in (obs0, om[0]) for a in acts)
    M = spec.projector.memory
    w = [np.zeros(M), np.zeros(M), np.zeros(M)]
    w[0][slots(obs0, -3.0)] = 1.0
    w[1][slots(obs0, -3.0)] = 1.0
    w[2][slots(obs0, 3.0)] = 10.0
    w[0][slots(om[0], 0.0)] = 5.0
    w[1][slots(om[0], 3.0)] = 5.0

    # one observation: the columns, and the serial order of the sums
    assert ens.combine(w, spec, obs0, ens.VOTE) == (0, 1, [2, 0, 1], [2.0, 0.0, 10.0], 0)
    assert ens.combine(w, spec, obs0, ens.MEAN_Q) == (2, 1, [2, 0, 1], [2.0, 0.0, 10.0], 0)
    assert ens.combine(w, spec, om[0], ens.VOTE) == (0, 3, [1, 1, 1], [0.0, 5.0, 5.0], 1)
    assert ens.combine(w, spec, om[0], ens.MEAN_Q) == (1, 2, [1, 1, 1], [0.0, 5.0, 5.0], 1)
    assert ens.combine(w, spec, op[0], ens.MEAN_Q) == (0, 3, [3, 0, 0], [0.0, 0.0, 0.0], 3)
    thirds = [np.zeros(M), np.zeros(M), np.zeros(M)]
    for m, v in enumerate((0.1, 0.2, 0.3)):                 # ((0 + a) + b) + c is not a + (b + c) for these
        thirds[m][slots(obs0, 0.0)] = v
    q = [float(ref.query_q(t, spec, [obs0])[0][0, 1]) for t in thirds]
    assert ens.combine(thirds, spec, obs0, ens.MEAN_Q)[3][1] == ((0.0 + q[0]) + q[1]) + q[2]
    assert ens.combine(thirds[::-1], spec, obs0, ens.MEAN_Q)[3][1] == ((0.0 + q[2]) + q[1]) + q[0]

    # the two episodes
    actions = []
    ret, disc, steps, code, ties, mties, agree, final = ens.episode(w, spec, start, ens.VOTE, actions_out=actions)
    assert actions == [-3.0, -3.0] and (steps, code, ties, mties, agree) == (2, 1, 1, 1, 2 + 1)
    assert ret == 0.0 + float(rm[0]) + float(rm2[0])
    assert disc == (0.0 + 1.0 * float(rm[0])) + (1.0 * spec.gamma) * float(rm2[0])
    assert final.tobytes() == xm2[0].tobytes()
    actions = []
    ret, disc, steps, code, ties, mties, agree, final = ens.episode(w, spec, start, ens.MEAN_Q, actions_out=actions, gamma=0.5)
    assert actions == [3.0, -3.0] and (steps, code, ties, mties, agree) == (2, 1, 1, 3, 1 + 3)
    assert ret == 0.0 + float(rp[0]) + float(rp2[0])
    assert disc == (0.0 + 1.0 * float(rp[0])) + (1.0 * 0.5) * float(rp2[0])
    assert final.tobytes() == xp2[0].tobytes()
    # cut at max_steps: code 0 after the first step
    out = ens.evaluate(w, spec, [start, start], ens.VOTE, max_steps=1)
    assert list(out["steps"]) == [1, 1] and list(out["terminal"]) == [0, 0] and list(out["agreement"]) == [2, 2]
    assert out["final_state"][1].tobytes() == xm[0].tobytes()
    # a group of one is the single policy's episode: its ties are the member's, one vote never ties, the member always agrees
    for rule in (ens.VOTE, ens.MEAN_Q):
        one = ens.episode(w[2:], spec, start, rule)
        single = ev.episode([w[2]], spec, start)
        assert one[:4] == single[:4] and one[5] == single[4] == 1 and one[6] == one[2] and one[7].tobytes() == single[5].tobytes()
        assert one[4] == (0 if rule == ens.VOTE else single[4])


def test_the_entry_point_is_declared_and_bound():
    import grl_amd
    from grl_amd import capi
    with open(os.path.join(ROOT, "include", "grlx.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+grlx_evaluate_ensemble\(grlx_ctx \*ctx, int first_replica, int n_replicas, int group_size, int rule,", header)
    assert re.search(r"enum \{ GRLX_ENSEMBLE_VOTE = 0, GRLX_ENSEMBLE_MEAN_Q = 1 \};", header)
    for cite in ("multi_discrete.cpp:120-235", "FIRST replica", "softmax(votes)", "ASCENDING", "member_ties", "agreement"):
        assert cite in header, cite
    assert "ensemble votes" not in header, "grlx_evaluate's NOT BUILT line still lists the ensemble"
    res, args = capi._SIGS["grlx_evaluate_ensemble"]
    assert len(args) == 16
    assert (capi.ENSEMBLE_VOTE, capi.ENSEMBLE_MEAN_Q) == (0, 1)
    assert grl_amd.EnsembleEvaluation._fields == ("ret", "disc", "steps", "terminal", "ties", "member_ties", "agreement", "final_state")
    assert callable(grl_amd.Runner.evaluate_ensemble)


# ---- grlxd -V: refused before any device is looked for (without a GPU, a run that got as far as the device would say "no HIP device") ----
@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def test_grlxd_usage_mentions_the_ensemble(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-V vote|mean]" in res.stdout + res.stderr


@pytest.mark.parametrize("args,yaml,states,word", [
    (["-r", "4", "-V", "vote"], "pendulum-sarsa-tc.yaml", None, "needs the start states of -E"),
    (["-r", "4", "-E", "states.txt", "-V", "median"], "pendulum-sarsa-tc.yaml", "3.14159 0 0\n", "unknown rule 'median'"),
    (["-r", "4", "-E", "states.txt", "-V", "vote"], "cart_pole-ac-tc.yaml", "0 3.14159 0 0 0\n", "not built for the actor-critic"),
    (["-r", "1", "-E", "states.txt", "-V", "mean"], "pendulum-sarsa-tc.yaml", "3.14159 0 0\n", "divides by n - 1"),
    (["-r", "4", "-E", "states.txt", "-V", "mean"], "pendulum-sarsa-tc.yaml", "3.14159 0\n", "2 columns, the model's state has 3"),
    (["-r", "4", "-g", "2", "-E", "states.txt", "-V", "vote"], "pendulum-sarsa-tc.yaml", "3.14159 0 0\n", "-g 2 is not built"),
    (["-r", "4", "-E", "states.txt", "-V", "vote"], "pendulum-fqi-ann.yaml", "3.14159 0 0\n", "not for experiment/batch_learning"),
])
def test_grlxd_ensemble_refusals_name_their_reason(grlxd, tmp_path, args, yaml, states, word):
    if states is not None:
        (tmp_path / "states.txt").write_text(states)
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12"] + args + [os.path.join(GOLDEN, yaml)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    out = res.stderr + res.stdout
    assert res.returncode != 0 and word in out, out
    assert "no HIP device" not in out, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*ensemble*")) and not list(tmp_path.glob("*returns*"))
