"""The host-side pieces of the per-step trajectories (grlx_evaluate_trajectory, grlx_evaluate_ensemble_trajectory) that need no device:
the reference helper on a hand-made dense table and an episode worked out by hand, the helper against the episode references it was
written out from, the declarations and bindings of the entry points, and what `grlxd -T` refuses before it looks for a device."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(GOLDEN, "pendulum-sarsa-tc.yaml")


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def test_reference_records_on_a_hand_made_table_and_a_two_step_episode():
    """test_policy_evaluate_host.py's table, rebuilt: the slots of (obs0, action 3) hold 16, those of (obs1, action -3) hold 64, every
    other slot 0; the start a step and a half before the timeout.  The two records are written out here from the oracle's own step results."""
    from tests import oracle_binding as ob
    from tests import policy_evaluate_ref as ev
    from tests import policy_query_ref as ref
    from tests import policy_trajectory_ref as tr
    spec = ob.pendulum_sarsa_spec(math=ob.MATH_PORTABLE)
    spec.projector.memory = 1 << 20
    assert ref.actions_of(spec) == [-3.0, 0.0, 3.0] and tr.dims(spec) == (2, 3) and tr.record_words(spec) == 11 and tr.record_words(spec, True) == 13
    start = np.array([np.pi, 30.0, spec.timeout - 1.5 * spec.control_step])
    obs0, _ = ev.observe(spec, start)
    x1, o1, r1, t1 = ob.env_step(spec, start, 3.0)
    x2, o2, r2, t2 = ob.env_step(spec, x1[0], -3.0)
    assert (int(t1[0]), int(t2[0])) == (0, 1)
    w = np.zeros(spec.projector.memory)
    w[ob.tile_project(spec.projector, [list(obs0) + [3.0]])[0]] = 16.0
    w[ob.tile_project(spec.projector, [list(o1[0]) + [-3.0]])[0]] = 64.0

    records, sums = tr.episode([w], spec, start, 5)
    assert records.shape == (5, 11)
    want0 = [3.0, float(r1[0]), 16.0, 2.0, 1.0, 0.0] + list(obs0) + list(x1[0])
    want1 = [-3.0, float(r2[0]), 64.0, 0.0, 1.0, 1.0] + list(o1[0]) + list(x2[0])
    assert bits(records[0]) == bits(want0) and bits(records[1]) == bits(want1)
    assert bits(records[2:]) == bytes(3 * 11 * 8), "records behind the episode's end are all-zero bits"
    assert sums[:5] == ev.episode([w], spec, start, 5)[:5] and bits(sums[5]) == bits(x2[0])
    # cut at max_steps = 1: one record, code 0
    records, sums = tr.episode([w], spec, start, 1)
    assert records.shape == (1, 11) and bits(records[0]) == bits(want0) and sums[2:5] == (1, 0, 0)
    # the all-zero table: a three-way tie, the first action acts, Q = 0; a state past the timeout still takes one step
    late = np.array([np.pi, 0.0, spec.timeout + 1.0])
    xl, _, rl, tl = ob.env_step(spec, late, -3.0)
    records, sums = tr.episode([np.zeros(spec.projector.memory)], spec, late, 4)
    assert bits(records[0]) == bits([-3.0, float(rl[0]), 0.0, 0.0, 3.0, 1.0] + list(ev.observe(spec, late)[0]) + list(xl[0]))
    assert sums[2:5] == (1, 1, 1) and not records[1:].any()
    # the ensemble's record on the same table as a group of one, both rules: two more words, the score in the value word
    from tests import policy_evaluate_ensemble_ref as ens
    for rule, scores in ((ens.VOTE, (1.0, 1.0)), (ens.MEAN_Q, (16.0, 64.0))):
        records, sums = tr.ensemble_episode([w], spec, start, rule, 3)
        assert records.shape == (3, 13)
        assert bits(records[0]) == bits([3.0, float(r1[0]), scores[0], 2.0, 1.0, 0.0, 1.0, 0.0] + list(obs0) + list(x1[0]))
        assert bits(records[1]) == bits([-3.0, float(r2[0]), scores[1], 0.0, 1.0, 1.0, 1.0, 0.0] + list(o1[0]) + list(x2[0]))
        assert not records[2].any()


@pytest.fixture(scope="module")
def trained(grlx):
    """graph -> (spec, start states, max_steps, [dense tables per member]) of the oracle after 3 trials; seeds as the GPU tests'"""
    from tests import oracle_binding as ob
    from tests import policy_evaluate_ref as ev
    from tests.test_gpu_policy_evaluate import start_states
    from tests.test_gpu_policy_query import SEED0, build
    out = {}
    for graph, members in (("pendulum_sarsa", 3), ("ac_twin", 1)):
        _, spec = build(grlx, graph, 1)
        tables = []
        for m in range(members):
            e = ob.Experiment(spec, seed=SEED0 + m)
            e.run(3)
            tables.append([np.array(t) for t in ev.tables_of(e)])
            e.close()
        out[graph] = (spec, start_states(graph, spec), 12, tables)
    return out


@pytest.mark.parametrize("graph", ["pendulum_sarsa", "ac_twin"])
def test_reference_sums_are_the_episode_references(trained, graph):
    """for every start state: the sums equal policy_evaluate_ref.episode's bit for bit, the reward column added up in step order is ret,
    the last record's state is the final state, the records behind the end are zero"""
    from tests import policy_evaluate_ref as ev
    from tests import policy_trajectory_ref as tr
    spec, states, ms, tables = trained[graph]
    D, S = tr.dims(spec)
    lengths = set()
    for s in states:
        records, sums = tr.episode(tables[0], spec, s, ms)
        want = ev.episode(tables[0], spec, s, ms)
        assert sums[2:5] == want[2:5] and bits(sums[:2]) == bits(want[:2]) and bits(sums[5]) == bits(want[5])
        steps = sums[2]
        ret = 0.0
        for t in range(steps):
            ret += records[t, tr.REWARD]
        assert bits(ret) == bits(sums[0])
        assert bits(records[steps - 1, tr.OBS + D:]) == bits(sums[5]) and records[steps - 1, tr.TERMINAL] == sums[3]
        assert not records[:steps - 1, tr.TERMINAL].any() and not records[steps:].any()
        assert int((records[:steps, tr.N_MAX] > 1).sum()) == sums[4]
        lengths.add(steps)
    assert 1 in lengths and ms in lengths


@pytest.mark.parametrize("rule", [0, 1])
def test_reference_ensemble_sums_are_the_ensemble_references(trained, rule):
    """a group of 3 under both rules: sums against policy_evaluate_ensemble_ref.episode; the per-step agreement and member_ties add up"""
    from tests import policy_evaluate_ensemble_ref as ens
    from tests import policy_trajectory_ref as tr
    spec, states, ms, tables = trained["pendulum_sarsa"]
    members = [t[0] for t in tables]
    D, S = tr.dims(spec)
    for s in states:
        records, sums = tr.ensemble_episode(members, spec, s, rule, ms)
        want = ens.episode(members, spec, s, rule, ms)
        assert sums[2:7] == want[2:7] and bits(sums[:2]) == bits(want[:2]) and bits(sums[7]) == bits(want[7])
        steps = sums[2]
        ret = 0.0
        for t in range(steps):
            ret += records[t, tr.REWARD]
        assert bits(ret) == bits(sums[0])
        assert int(records[:, tr.ENS_AGREEMENT].sum()) == sums[6] and int(records[:, tr.ENS_MEMBER_TIES].sum()) == sums[5]
        assert bits(records[steps - 1, tr.ENS_OBS + D:]) == bits(sums[7]) and not records[steps:].any()
        if rule == ens.VOTE:
            assert bits(records[:, tr.VALUE]) == bits(records[:, tr.ENS_AGREEMENT])


def test_the_entry_points_are_declared_and_bound():
    import grl_amd
    from grl_amd import capi
    with open(os.path.join(ROOT, "include", "grlx.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+grlx_evaluate_trajectory\(grlx_ctx \*ctx, int first_replica, int n_replicas,\s*const double \*states", header)
    assert re.search(r"\bint\s+grlx_evaluate_ensemble_trajectory\(grlx_ctx \*ctx, int first_replica, int n_replicas, int group_size, int rule,", header)
    assert re.search(r"\bint\s+grlx_trajectory_record_words\(grlx_ctx \*ctx, int ensemble\);", header)
    offsets = dict(GRLX_TRAJ_ACTION=0, GRLX_TRAJ_REWARD=1, GRLX_TRAJ_VALUE=2, GRLX_TRAJ_ACTION_INDEX=3, GRLX_TRAJ_N_MAX=4, GRLX_TRAJ_TERMINAL=5,
                   GRLX_TRAJ_OBS=6, GRLX_TRAJ_ENS_AGREEMENT=6, GRLX_TRAJ_ENS_MEMBER_TIES=7, GRLX_TRAJ_ENS_OBS=8)
    for name, value in offsets.items():
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert (capi.TRAJ_ACTION, capi.TRAJ_REWARD, capi.TRAJ_VALUE, capi.TRAJ_ACTION_INDEX, capi.TRAJ_N_MAX, capi.TRAJ_TERMINAL, capi.TRAJ_OBS,
            capi.TRAJ_ENS_AGREEMENT, capi.TRAJ_ENS_MEMBER_TIES, capi.TRAJ_ENS_OBS) == tuple(offsets.values())
    not_built = re.findall(r"NOT BUILT:.*?\*/", header, flags=re.S)
    assert len(not_built) >= 3 and not any("per-step trajectories" in s for s in not_built), "a NOT BUILT line still lists the trajectories"
    assert [len(capi._SIGS[n][1]) for n in ("grlx_evaluate_trajectory", "grlx_evaluate_ensemble_trajectory", "grlx_trajectory_record_words")] == [13, 17, 2]
    assert "#define GRLX_ABI_VERSION 2" in header and capi.ABI_VERSION == 2
    assert grl_amd.Trajectory._fields == grl_amd.Evaluation._fields + ("records",)
    assert grl_amd.EnsembleTrajectory._fields == grl_amd.EnsembleEvaluation._fields + ("records",)
    assert callable(grl_amd.Runner.evaluate_trajectory) and callable(grl_amd.Runner.evaluate_ensemble_trajectory)
    assert "Trajectory" in grl_amd.__all__ and "EnsembleTrajectory" in grl_amd.__all__


def test_the_views_cut_the_records_by_name():
    import grl_amd
    rec = np.arange(2 * 3 * 4 * 11, dtype=np.float64).reshape(2, 3, 4, 11)
    steps = np.full((2, 3), 2, np.int32)
    t = grl_amd.Trajectory(None, None, steps, None, None, np.zeros((2, 3, 3)), rec)
    assert t.action.shape == (2, 3, 4) and t.obs.shape == (2, 3, 4, 2) and t.state.shape == (2, 3, 4, 3)
    assert t.code[1, 2, 3] == rec[1, 2, 3, 5] and t.obs[0, 1, 2, 0] == rec[0, 1, 2, 6] and t.state[0, 0, 0, 2] == rec[0, 0, 0, 10]
    assert t.episode(1, 2).shape == (2, 11) and t.episode(1, 2)[1, 0] == rec[1, 2, 1, 0]
    with pytest.raises(ValueError):
        t.reward[0, 0, 0] = 1.0
    rec = np.arange(1 * 2 * 3 * 13, dtype=np.float64).reshape(1, 2, 3, 13)
    e = grl_amd.EnsembleTrajectory(None, None, np.ones((1, 2), np.int32), None, None, None, None, np.zeros((1, 2, 3)), rec)
    assert e.step_agreement[0, 1, 2] == rec[0, 1, 2, 6] and e.step_member_ties[0, 1, 2] == rec[0, 1, 2, 7]
    assert e.obs.shape == (1, 2, 3, 2) and e.obs[0, 0, 0, 0] == rec[0, 0, 0, 8] and e.state[0, 0, 0, 0] == rec[0, 0, 0, 10]


# ---- grlxd -T: refused before any device is looked for (without a GPU, a run that got as far as the device would say "no HIP device") ----
@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def test_grlxd_usage_mentions_the_trajectories(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-T steps]" in res.stdout + res.stderr and "[-E states]" in res.stdout + res.stderr


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-T", "12"], "pendulum-sarsa-tc.yaml", "need the start states of -E"),
    (["-r", "4", "-E", "states.txt", "-T", "0"], "pendulum-sarsa-tc.yaml", "outside 1 ... GRLX_MAX_EPISODE_STEPS"),
    (["-r", "4", "-E", "states.txt", "-T", "-3"], "pendulum-sarsa-tc.yaml", "outside 1 ... GRLX_MAX_EPISODE_STEPS"),
    (["-r", "4", "-E", "states.txt", "-T", "100001"], "pendulum-sarsa-tc.yaml", "outside 1 ... GRLX_MAX_EPISODE_STEPS"),
    (["-r", "4", "-g", "2", "-E", "states.txt", "-T", "12"], "pendulum-sarsa-tc.yaml", "-g 2 is not built"),
    (["-r", "1", "-E", "states.txt", "-T", "12"], "pendulum-sarsa-tc.yaml", "divides by n - 1"),
    (["-r", "4", "-E", "states.txt", "-T", "12"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
    (["-r", "4", "-E", "states.txt", "-V", "vote", "-T", "12"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
])
def test_grlxd_trajectory_refusals_name_their_reason(grlxd, tmp_path, args, yaml, word):
    (tmp_path / "states.txt").write_text("# angle velocity time\n3.14159 0 0\n0 0 0   # upright\n\n1 -2 1.5\n")
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12"] + args + [os.path.join(GOLDEN, yaml)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    said = res.stderr + res.stdout
    assert res.returncode != 0 and word in said, said
    assert "-T" in said
    assert "no HIP device" not in said, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*trajectories*"))
