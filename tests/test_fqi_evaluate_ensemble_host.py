"""The host-side pieces of the batch path's ensemble (grlx_fqi_query_ensemble, grlx_fqi_evaluate_ensemble,
grlx_fqi_ensemble_trajectory_record_words, grlx_fqi_evaluate_ensemble_trajectory) that need no device: declarations and bindings, the
header's NOT BUILT blocks, the refusal of a null context, the record layout the Python side assumes, and the reference helper on the
oracle's untrained networks."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grlx_fqi_query_ensemble", "grlx_fqi_evaluate_ensemble", "grlx_fqi_ensemble_trajectory_record_words",
         "grlx_fqi_evaluate_ensemble_trajectory")


def header():
    with open(os.path.join(ROOT, "include", "grlx.h")) as f:
        return f.read()


def test_the_entry_points_are_declared_and_bound(grlx):
    from grl_amd import capi
    text = header()
    sums = (r"const double \*states[^,]*, int n_starts, int max_steps,\s*double \*ret, double \*disc, int32_t \*steps, int32_t \*terminal, "
            r"int32_t \*ties,\s*int64_t \*member_ties, int64_t \*agreement, double \*final_state")
    group = r"\(grlx_fqi_ctx \*ctx, int first_replica, int n_replicas, int group_size, "
    assert re.search(r"\bint\s+grlx_fqi_query_ensemble" + group + r"const double \*obs[^,]*, int n_obs,\s*double \*out\);", text)
    assert re.search(r"\bint\s+grlx_fqi_evaluate_ensemble" + group + r"int rule,\s*" + sums + r"\);", text)
    assert re.search(r"\bint\s+grlx_fqi_ensemble_trajectory_record_words\(grlx_fqi_ctx \*ctx\);", text)
    assert re.search(r"\bint\s+grlx_fqi_evaluate_ensemble_trajectory" + group + r"int rule,\s*" + sums + r",\s*double \*records[^,)]*\);", text)
    assert re.search(r"\bint\s+grlx_fqi_trajectory_record_words\(grlx_fqi_ctx \*ctx\);", text), "the single policy's keeps its one argument"
    assert [len(capi._SIGS[n][1]) for n in NAMES] == [7, 16, 1, 17]
    assert capi._SIGS["grlx_fqi_query_ensemble"] == capi._SIGS["grlx_query_ensemble"], "the online sibling's list: the context types are both void *"
    assert capi._SIGS["grlx_fqi_evaluate_ensemble"] == capi._SIGS["grlx_evaluate_ensemble"]
    assert capi._SIGS["grlx_fqi_evaluate_ensemble_trajectory"] == capi._SIGS["grlx_evaluate_ensemble_trajectory"]
    # the declarations themselves differ from the online siblings' in the context type and the width the comments give, nothing else
    def declaration(name):
        m = re.search(r"\bint\s+" + name + r"\((.*?)\);", text, flags=re.S)
        return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))).strip()
    for fqi, online in (("grlx_fqi_evaluate_ensemble", "grlx_evaluate_ensemble"),
                        ("grlx_fqi_evaluate_ensemble_trajectory", "grlx_evaluate_ensemble_trajectory"),
                        ("grlx_fqi_query_ensemble", "grlx_query_ensemble")):
        assert declaration(fqi) == declaration(online).replace("grlx_ctx *ctx", "grlx_fqi_ctx *ctx"), fqi
    lib = capi.load()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in capi._NEWER_SIGS, n
    for m in ("query_ensemble_raw", "query_ensemble", "evaluate_ensemble", "ensemble_trajectory_record_words", "evaluate_ensemble_trajectory"):
        assert callable(getattr(grlx.FqiRunner, m)), m


def test_no_not_built_block_lists_an_ensemble_of_fqi_replicas():
    blocks = re.findall(r"NOT BUILT:.*?\*/", header(), flags=re.S)
    assert len(blocks) >= 3
    for b in blocks:
        assert "batch path" not in b, b
        assert "grlx_fqi_ctx" not in b, b
        assert not re.search(r"ensemble\s+over\s+the\s+replicas", b), b
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "grlx_fqi_evaluate_ensemble" in readme
    assert not re.search(r"ensemble[^.\n]*of FQI replicas", readme.split("Not built")[-1]), "README's Not built list still names it"


def test_a_null_context_is_refused_without_a_device(grlx):
    from grl_amd import capi
    lib = capi.load()
    states, obs = np.array([[np.pi, 0.0, 0.0]]), np.array([[np.pi, 0.0]])
    out, cols, rec = np.full(1, 7.0), np.full(8, 7.0), np.full(13, 7.0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.grlx_fqi_query_ensemble(None, 0, 1, 1, p(obs), 1, p(cols)) == capi.ERR_INVALID
    assert "grlx_fqi_query_ensemble: ctx is null" in lib.grlx_last_error().decode()
    assert lib.grlx_fqi_evaluate_ensemble(None, 0, 1, 1, 0, p(states), 1, 0, p(out), None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert "grlx_fqi_evaluate_ensemble: ctx is null" in lib.grlx_last_error().decode()
    assert lib.grlx_fqi_ensemble_trajectory_record_words(None) == capi.ERR_INVALID
    assert "ctx is null" in lib.grlx_last_error().decode()
    assert lib.grlx_fqi_evaluate_ensemble_trajectory(None, 0, 1, 1, 0, p(states), 1, 1, p(out), None, None, None, None, None, None, None,
                                                     p(rec)) == capi.ERR_INVALID
    assert "grlx_fqi_evaluate_ensemble_trajectory: ctx is null" in lib.grlx_last_error().decode()
    assert out[0] == 7.0 and (cols == 7.0).all() and (rec == 7.0).all()


def test_the_record_has_eight_words_the_observation_and_the_state(grlx):
    from grl_amd import capi
    from tests import fqi_evaluate_ensemble_ref as er
    assert er.WORDS == 8 + 2 + 3 == capi.TRAJ_ENS_OBS + 2 + grlx.FqiRunner.STATE_DIMS
    assert (er.ACTION, er.REWARD, er.VALUE, er.ACTION_INDEX, er.N_MAX, er.TERMINAL, er.ENS_AGREEMENT, er.ENS_MEMBER_TIES, er.ENS_OBS) == (
        capi.TRAJ_ACTION, capi.TRAJ_REWARD, capi.TRAJ_VALUE, capi.TRAJ_ACTION_INDEX, capi.TRAJ_N_MAX, capi.TRAJ_TERMINAL, capi.TRAJ_ENS_AGREEMENT,
        capi.TRAJ_ENS_MEMBER_TIES, capi.TRAJ_ENS_OBS)
    assert (er.VOTE, er.MEAN_Q) == (capi.ENSEMBLE_VOTE, capi.ENSEMBLE_MEAN_Q)
    rec = np.arange(2 * 3 * 4 * er.WORDS, dtype=np.float64).reshape(2, 3, 4, er.WORDS)
    z = np.zeros((2, 3))
    t = grlx.EnsembleTrajectory(None, None, np.full((2, 3), 2, np.int32), None, None, z, z, np.zeros((2, 3, 3)), rec)
    assert t.obs.shape == (2, 3, 4, 2) and t.state.shape == (2, 3, 4, 3) and t.value[1, 2, 3] == rec[1, 2, 3, er.VALUE]
    assert t.obs[1, 2, 3, 0] == rec[1, 2, 3, er.ENS_OBS] and t.state[1, 2, 3, 0] == rec[1, 2, 3, er.ENS_OBS + 2]
    assert t.step_agreement[1, 2, 3] == rec[1, 2, 3, er.ENS_AGREEMENT] and t.step_member_ties[0, 1, 2] == rec[0, 1, 2, er.ENS_MEMBER_TIES]
    assert t.episode(1, 2).shape == (2, er.WORDS)


def test_the_reference_on_the_untrained_networks():
    """the oracle before any batch.  A group of one is fqi_evaluate_ref's episode record for record with two words inserted (under VOTE the
    one vote never ties and the score is 1); the sums are the records' sums; max_steps cuts; the sums run in the members' order"""
    from tests import fqi_evaluate_ensemble_ref as er
    from tests import fqi_evaluate_ref as fr
    from tests import oracle_binding as ob
    from tests import policy_evaluate_ref as ev
    spec = ob.pendulum_fqi_spec(batch_size=50, iterations=1, epochs=1)
    es = [ob.FqiExperiment(spec, seed=s) for s in (3, 4, 5)]
    start = [np.pi, 0.0, 0.0]
    for e in es[:2]:
        single, ssums = fr.episode(e, start, 7)
        for rule in (er.VOTE, er.MEAN_Q):
            rec, (ret, disc, steps, code, ties, mties, agree, x) = er.episode([e], start, rule, 7)
            assert rec.shape == (7, er.WORDS) and (ret, disc, steps, code) == ssums[:4] and x.tobytes() == ssums[5].tobytes()
            assert mties == ssums[4] and agree == steps and ties == (0 if rule == er.VOTE else ssums[4])
            same = [er.ACTION, er.REWARD, er.ACTION_INDEX, er.TERMINAL] + ([er.VALUE, er.N_MAX] if rule == er.MEAN_Q else [])
            assert rec[:, same].tobytes() == single[:, same].tobytes()
            assert rec[:, er.ENS_OBS:].tobytes() == single[:, fr.OBS:].tobytes()
            assert (rec[:, er.ENS_AGREEMENT] == 1.0).all() and (rec[:, er.ENS_MEMBER_TIES] == (single[:, fr.N_MAX] > 1)).all()
            if rule == er.VOTE:
                assert (rec[:, er.VALUE] == 1.0).all() and (rec[:, er.N_MAX] == 1.0).all()
    # three members: the columns at one observation, and the order of the sums
    obs, _ = ev.observe(spec.base, start)
    actions = fr.actions_of(spec)
    q = [er.member_q(e, obs, actions) for e in es]
    mai, man, votes, sumq, mties = er.combine(es, obs, er.MEAN_Q)
    assert sumq == [((0.0 + q[0][k]) + q[1][k]) + q[2][k] for k in range(3)] and (mai, man) == er.findmax(sumq)
    assert er.combine(es[::-1], obs, er.MEAN_Q)[3] == [((0.0 + q[2][k]) + q[1][k]) + q[0][k] for k in range(3)]
    assert sum(votes) == 3 and votes == [sum(1 for m in q if er.findmax(m)[0] == k) for k in range(3)]
    assert mties == sum(1 for m in q if er.findmax(m)[1] > 1)
    assert er.combine(es, obs, er.VOTE)[:2] == er.findmax(votes)
    assert er.findmax([1, 3, 3]) == (1, 2) and er.findmax([2.0, 2.0, 2.0]) == (0, 3) and er.findmax([5, 1, 0]) == (0, 1)
    # the sums are the records' sums, for both rules
    for rule in (er.VOTE, er.MEAN_Q):
        rec, (ret, disc, steps, code, ties, mties, agree, x) = er.episode(es, start, rule, 5)
        assert (steps, code) == (5, 0) and not rec[:, er.TERMINAL].any()
        acc, dsum, g = 0.0, 0.0, 1.0
        for t in range(steps):
            acc += rec[t, er.REWARD]
            dsum += g * rec[t, er.REWARD]
            g = g * spec.gamma_tau
        assert acc == ret and dsum == disc and list(rec[steps - 1, er.ENS_OBS + 2:]) == list(x)
        assert rec[:, er.ENS_AGREEMENT].sum() == agree and rec[:, er.ENS_MEMBER_TIES].sum() == mties and (rec[:, er.N_MAX] > 1).sum() == ties
        assert ((rec[:, er.ENS_AGREEMENT] >= 1) & (rec[:, er.ENS_AGREEMENT] <= 3)).all()
        full, sums = er.episode(es, start, rule)
        assert full.shape == (100, er.WORDS) and sums[2:4] == (100, 1) and full[:5].tobytes() == rec.tobytes()
    # past the timeout: exactly one step, zeros behind it
    rec, sums = er.episode(es, [1.0, -2.0, spec.base.timeout + 1.0], er.VOTE, 4)
    assert sums[2:4] == (1, 1) and not rec[1:].any() and rec[0, er.TERMINAL] == 1.0
    out, recs = er.evaluate_groups(es, 1, [start, start], er.MEAN_Q, 3)
    assert out["ret"].shape == (3, 2) and out["final_state"].shape == (3, 2, 3) and len(recs) == 3 and recs[2][1].shape == (3, er.WORDS)
    for e in es:
        e.close()
