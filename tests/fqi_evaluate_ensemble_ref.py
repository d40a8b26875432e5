"""Reference of the batch path's ensemble evaluation episodes (grlx_fqi_evaluate_ensemble, grlx_fqi_evaluate_ensemble_trajectory) and of
grlx_fqi_query_ensemble: a plain Python loop over a LIST of oracle experiments (oracle_binding.FqiExperiment), the members of one group in
ascending replica order, on top of fqi_evaluate_ref (actions, the record words) and policy_evaluate_ref (observe, in_domain, the cap).

  obs = observe(state)                       the start state's terminal code is ignored: an episode has at least one step
  repeat: for the members m in ASCENDING order: q_m[k] = e_m.q(obs, actions[k]); mai_m, man_m = findmax(q_m) (strict >, counting ==)
              votes[mai_m] += 1; sumq[k] += q_m[k] (one accumulator per action, from 0.0); member ties += (man_m > 1)
          mai, man = findmax(votes) (VOTE) or findmax(sumq) (MEAN_Q);  action = actions[mai]; no draw
          ties += (man > 1); agreement += votes[mai]
          state, obs, reward, terminal = step(state, action)
          ret += reward; disc += g * reward; g = g * gamma_tau; steps += 1
  until terminal != 0, the step ended outside the portable math's domain (code 3), or steps == max_steps (code 0)

One record per step taken (include/grlx.h: GRLX_TRAJ_*, GRLX_TRAJ_ENS_*): action, reward, the combined score of the action taken
((double)votes[mai] or sumq[mai]), mai, man, the code after the step, votes[mai], the members with a tie at this step, the observation
acted on, the model state after the step; records behind the episode's end are zero.
"""
import numpy as np

from tests import fqi_evaluate_ref as fr
from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev

VOTE, MEAN_Q = 0, 1                 # include/grlx.h: GRLX_ENSEMBLE_VOTE, GRLX_ENSEMBLE_MEAN_Q
ACTION, REWARD, VALUE, ACTION_INDEX, N_MAX, TERMINAL = fr.ACTION, fr.REWARD, fr.VALUE, fr.ACTION_INDEX, fr.N_MAX, fr.TERMINAL
ENS_AGREEMENT, ENS_MEMBER_TIES, ENS_OBS = 6, 7, 8
D, S = fr.D, fr.S
WORDS = ENS_OBS + D + S
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "member_ties", "agreement", "final_state")


def findmax(v):
    """GreedySampler::findmax (greedy.cpp:47-61): the first maximum and the number of maxima"""
    mai, man = 0, 1
    for k in range(1, len(v)):
        if v[k] > v[mai]:
            mai, man = k, 1
        elif v[k] == v[mai]:
            man += 1
    return mai, man


def member_q(e, obs, actions):
    return [e.q(obs, a) for a in actions]


def combine(members, obs, rule):
    """(mai, man, votes, sumq, member ties) of the group `members` (FqiExperiments, ascending) at one observation"""
    actions = fr.actions_of(members[0].spec)
    votes, sumq, mties = [0] * len(actions), [0.0] * len(actions), 0
    for e in members:
        q = member_q(e, obs, actions)
        mai_m, man_m = findmax(q)
        votes[mai_m] += 1
        for k in range(len(actions)):
            sumq[k] += q[k]
        mties += 1 if man_m > 1 else 0
    mai, man = findmax(votes if rule == VOTE else sumq)
    return mai, man, votes, sumq, mties


def episode(members, state, rule, max_steps=0):
    """(records[max_steps or steps][WORDS], (ret, disc, steps, terminal, ties, member_ties, agreement, final_state)) of one episode of the
    group from `state`; with max_steps == 0 (the cap) the records are as long as the episode"""
    assert rule in (VOTE, MEAN_Q)
    spec = members[0].spec
    cap = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    actions = fr.actions_of(spec)
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec.base, x)
    rows = []
    ret, disc, g, steps, ties, mties, agree, code = 0.0, 0.0, 1.0, 0, 0, 0, 0, 0
    while True:
        mai, man, votes, sumq, mt = combine(members, obs, rule)
        action = actions[mai]
        nx, nobs, reward, term = ob.env_step(spec.base, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * float(spec.gamma_tau)
        steps += 1
        ties += 1 if man > 1 else 0
        mties += mt
        agree += votes[mai]
        code = ev.DOMAIN if not ev.in_domain(spec.base, x) else int(term[0])
        value = float(votes[mai]) if rule == VOTE else sumq[mai]
        rows.append([action, reward, value, float(mai), float(man), float(code), float(votes[mai]), float(mt)] + list(before) + list(x))
        if code != 0 or steps >= cap:
            break
    records = np.zeros((max_steps if max_steps else steps, WORDS))
    records[:steps] = rows
    return records, (ret, disc, steps, code, ties, mties, agree, x)


def evaluate(members, states, rule, max_steps=0):
    """one group: (dict of the eight outputs, [n] each (final_state [n][3]), list of the n episodes' records)"""
    states = np.asarray(states, np.float64)
    n = states.shape[0]
    out = dict(ret=np.zeros(n), disc=np.zeros(n), steps=np.zeros(n, np.int32), terminal=np.zeros(n, np.int32), ties=np.zeros(n, np.int32),
               member_ties=np.zeros(n, np.int64), agreement=np.zeros(n, np.int64), final_state=np.zeros_like(states))
    records = []
    for s in range(n):
        rec, res = episode(members, states[s], rule, max_steps)
        for f, v in zip(FIELDS, res):
            out[f][s] = v
        records.append(rec)
    return out, records


def evaluate_groups(es, group_size, states, rule, max_steps=0):
    """the experiments es in groups of group_size consecutive ones: (dict of [group][start] arrays, records[group][start])"""
    assert group_size >= 1 and len(es) % group_size == 0
    outs, recs = zip(*[evaluate(es[g:g + group_size], states, rule, max_steps) for g in range(0, len(es), group_size)])
    return {k: np.stack([o[k] for o in outs]) for k in FIELDS}, recs
