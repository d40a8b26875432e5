"""Reference of the ensemble evaluation episodes (grlx_evaluate_ensemble): a plain Python loop over policy_query_ref.query_q / findmax on
the members' DENSE parameter vectors, the oracle's environment step and its first observation (policy_evaluate_ref.observe).

  obs = observe(state)                       the start state's terminal code is ignored: an episode has at least one step
  repeat: for the members m in ASCENDING order: q_m, mai_m, man_m = query_q(table of m, obs)
              votes[mai_m] += 1; sumq[a] += q_m[a] (one accumulator per action, from 0.0); member_ties += (man_m > 1)
          mai, man = findmax(votes) (VOTE) or findmax(sumq) (MEAN_Q);  action = actions[mai]
          ties += (man > 1); agreement += votes[mai]
          state, obs, reward, terminal = step(state, action)
          ret += reward; disc += g * reward; g = g * gamma; steps += 1
  until terminal != 0, the step ended outside the portable math's domain (code 3), or steps == max_steps (code 0)
"""
import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref

VOTE, MEAN_Q = 0, 1                 # include/grlx.h: GRLX_ENSEMBLE_VOTE, GRLX_ENSEMBLE_MEAN_Q
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "member_ties", "agreement", "final_state")


def combine(members, spec, obs, rule):
    """(mai, man, votes, sumq, member ties) of the group whose members' tables 0 are the dense vectors `members`, at one observation"""
    A = int(spec.action_steps)
    votes, sumq, mties = [0] * A, [0.0] * A, 0
    for w in members:
        q, _, greedy, n_max = ref.query_q(w, spec, [obs])
        votes[int(greedy[0])] += 1
        for a in range(A):
            sumq[a] += float(q[0, a])
        mties += 1 if int(n_max[0]) > 1 else 0
    mai, man = ref.findmax(votes if rule == VOTE else sumq)
    return mai, man, votes, sumq, mties


def episode(members, spec, state, rule, max_steps=0, gamma=None, actions_out=None):
    """(ret, disc, steps, terminal, ties, member_ties, agreement, final_state) of one episode of the group from `state`"""
    assert rule in (VOTE, MEAN_Q)
    max_steps = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    acts = ref.actions_of(spec)
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, ties, mties, agree, code = 0.0, 0.0, 1.0, 0, 0, 0, 0, 0
    while True:
        mai, man, votes, _, mt = combine(members, spec, obs, rule)
        action = acts[mai]
        if actions_out is not None:
            actions_out.append(action)
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
        if code != 0 or steps >= max_steps:
            break
    return ret, disc, steps, code, ties, mties, agree, x


def evaluate(members, spec, states, rule, max_steps=0, gamma=None):
    """one group: dict of the eight outputs, [n] each (final_state [n][S])"""
    states = np.asarray(states, np.float64)
    n = states.shape[0]
    out = dict(ret=np.zeros(n), disc=np.zeros(n), steps=np.zeros(n, np.int32), terminal=np.zeros(n, np.int32), ties=np.zeros(n, np.int32),
               member_ties=np.zeros(n, np.int64), agreement=np.zeros(n, np.int64), final_state=np.zeros_like(states))
    for s in range(n):
        res = episode(members, spec, states[s], rule, max_steps, gamma)
        for f, v in zip(FIELDS, res):
            out[f][s] = v
    return out
