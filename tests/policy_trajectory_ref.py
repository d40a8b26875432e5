"""Reference of the per-step trajectories (grlx_evaluate_trajectory, grlx_evaluate_ensemble_trajectory): policy_evaluate_ref.episode's
loop written out again, because that function keeps no steps.  Per step one record of R doubles (include/grlx.h: GRLX_TRAJ_*):

  single policy, R = 6 + D + S:  action, reward, value, action_index, n_max, terminal | obs acted on [D] | model state after the step [S]
  ensemble,      R = 8 + D + S:  ... terminal, agreement, member_ties | obs [D] | state [S]

  value: Q agents Q(obs, chosen action) = query_q's value; actor-critic the actor's read before the action clip = query_state(table 1);
         ensemble the combined score of the action taken, votes[mai] (VOTE) or sumq[mai] (MEAN_Q)
  terminal: the episode's code after the step (0 while it goes on and in the last record of an episode cut at max_steps)
Records at index >= steps stay zero.
"""
import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_ref as ens
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref

ACTION, REWARD, VALUE, ACTION_INDEX, N_MAX, TERMINAL, OBS = 0, 1, 2, 3, 4, 5, 6
ENS_AGREEMENT, ENS_MEMBER_TIES, ENS_OBS = 6, 7, 8


def dims(spec):
    """(D, S): observation and model state dimensions of the spec's environment"""
    L = ob.load()
    return int(L.orc_env_obs_dims(spec.env)), int(L.orc_env_state_dims(spec.env))


def record_words(spec, ensemble=False):
    D, S = dims(spec)
    return (ENS_OBS if ensemble else OBS) + D + S


def _act(tables, spec, obs):
    """(action, value, action_index, n_max) of the test agent at obs"""
    if spec.agent == ob.AGENT_AC:           # ev.greedy_action's lines, keeping the read before the clip
        a = float(ref.query_state(tables[1], spec, 1, [obs])[0])
        return min(max(a, spec.action_min), spec.action_max), a, -1, 1
    _, value, greedy, n_max = ref.query_q(tables[0], spec, [obs])
    return ref.actions_of(spec)[int(greedy[0])], float(value[0]), int(greedy[0]), int(n_max[0])


def episode(tables, spec, state, max_steps, gamma=None):
    """(records [max_steps][R], (ret, disc, steps, terminal, ties, final_state)) of one episode from `state`"""
    assert max_steps >= 1
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    D, S = dims(spec)
    records = np.zeros((max_steps, OBS + D + S))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, ties, code = 0.0, 0.0, 1.0, 0, 0, 0
    while True:
        action, value, mai, man = _act(tables, spec, obs)
        before = obs
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        x, obs, reward = nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        ties += 1 if man > 1 else 0
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        rec = records[steps - 1]
        rec[ACTION], rec[REWARD], rec[VALUE], rec[ACTION_INDEX], rec[N_MAX], rec[TERMINAL] = action, reward, value, mai, man, code
        rec[OBS:OBS + D] = before[:D]
        rec[OBS + D:] = x[:S]
        if code != 0 or steps >= max_steps:
            break
    return records, (ret, disc, steps, code, ties, x)


def ensemble_episode(members, spec, state, rule, max_steps, gamma=None):
    """(records [max_steps][R], (ret, disc, steps, terminal, ties, member_ties, agreement, final_state)) of one episode of the group"""
    assert rule in (ens.VOTE, ens.MEAN_Q) and max_steps >= 1
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    D, S = dims(spec)
    acts = ref.actions_of(spec)
    records = np.zeros((max_steps, ENS_OBS + D + S))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, ties, mties, agree, code = 0.0, 0.0, 1.0, 0, 0, 0, 0, 0
    while True:
        mai, man, votes, sumq, mt = ens.combine(members, spec, obs, rule)
        action, before = acts[mai], obs
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        x, obs, reward = nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        ties += 1 if man > 1 else 0
        mties += mt
        agree += votes[mai]
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        rec = records[steps - 1]
        rec[ACTION], rec[REWARD], rec[ACTION_INDEX], rec[N_MAX], rec[TERMINAL] = action, reward, mai, man, code
        rec[VALUE] = float(votes[mai]) if rule == ens.VOTE else sumq[mai]
        rec[ENS_AGREEMENT], rec[ENS_MEMBER_TIES] = votes[mai], mt
        rec[ENS_OBS:ENS_OBS + D] = before[:D]
        rec[ENS_OBS + D:] = x[:S]
        if code != 0 or steps >= max_steps:
            break
    return records, (ret, disc, steps, code, ties, mties, agree, x)


def _collect(fields, states, results, int64=()):
    n = states.shape[0]
    out = {f: np.zeros(n, np.int64 if f in int64 else np.int32) for f in fields if f not in ("ret", "disc", "final_state")}
    out.update(ret=np.zeros(n), disc=np.zeros(n), final_state=np.zeros_like(states))
    for s, (_, sums) in enumerate(results):
        for f, v in zip(fields, sums):
            out[f][s] = v
    out["records"] = np.stack([rec for rec, _ in results])
    return out


def evaluate(tables, spec, states, max_steps, gamma=None):
    """one replica: policy_evaluate_ref.evaluate's dict and records [n][max_steps][R]"""
    states = np.asarray(states, np.float64)
    return _collect(ev.FIELDS, states, [episode(tables, spec, s, max_steps, gamma) for s in states])


def evaluate_ensemble(members, spec, states, rule, max_steps, gamma=None):
    """one group: policy_evaluate_ensemble_ref.evaluate's dict and records [n][max_steps][R]"""
    states = np.asarray(states, np.float64)
    return _collect(ens.FIELDS, states, [ensemble_episode(members, spec, s, rule, max_steps, gamma) for s in states], ("member_ties", "agreement"))


FIELDS = ev.FIELDS + ("records",)
ENSEMBLE_FIELDS = ens.FIELDS + ("records",)
