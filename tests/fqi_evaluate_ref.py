"""Reference of the batch path's greedy evaluation episodes (grlx_fqi_evaluate, grlx_fqi_evaluate_trajectory): a plain Python loop over the
oracle's own pieces -- its first observation (orc_env_observe), FqiExperiment.q (orc_fqi_q: the projector's normalisation and the
network's forward pass on the experiment's current parameters), its environment step (orc_env_step).

  obs = observe(state)                       the start state's terminal code is ignored: an episode has at least one step
  repeat: q[k] = Q(obs, actions[k]); mai, man = the first maximum and the number of maxima (strict >, counting ==); no draw
          state, obs, reward, terminal = step(state, actions[mai])
          ret += reward; disc += g * reward; g = g * gamma_tau; steps += 1; ties += man > 1
  until terminal != 0, the step ended outside the portable math's domain (code 3), or steps == max_steps (code 0)

One record per step taken (include/grlx.h: GRLX_TRAJ_*): action, reward, q[mai], mai, man, the code after the step, the observation
acted on, the model state after the step; records behind the episode's end are zero.
"""
import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev

ACTION, REWARD, VALUE, ACTION_INDEX, N_MAX, TERMINAL, OBS = 0, 1, 2, 3, 4, 5, 6
D, S = 2, 3
WORDS = OBS + D + S
FIELDS = ev.FIELDS


def actions_of(spec):
    """discretizer/uniform over the task's action range, as orc_fqi_create and grlx_fqi_create build the list"""
    b = spec.base
    delta = (b.action_max - b.action_min) / (float(b.action_steps) - 1) if b.action_steps != 1 else 0.0
    return [b.action_min + delta * k for k in range(b.action_steps)]


def episode(e, state, max_steps=0):
    """(records[max_steps or steps][WORDS], (ret, disc, steps, terminal, ties, final_state)) of one episode of FqiExperiment e from `state`;
    with max_steps == 0 (the cap) the records are as long as the episode"""
    spec = e.spec
    cap = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    actions = actions_of(spec)
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec.base, x)
    rows = []
    ret, disc, g, steps, ties, code = 0.0, 0.0, 1.0, 0, 0, 0
    while True:
        q = [e.q(obs, a) for a in actions]
        mai, man = 0, 1
        for k in range(1, len(q)):
            if q[k] > q[mai]:
                mai, man = k, 1
            elif q[k] == q[mai]:
                man += 1
        action = actions[mai]
        nx, nobs, reward, term = ob.env_step(spec.base, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * float(spec.gamma_tau)
        steps += 1
        ties += 1 if man > 1 else 0
        code = ev.DOMAIN if not ev.in_domain(spec.base, x) else int(term[0])
        rows.append([action, reward, q[mai], float(mai), float(man), float(code)] + list(before) + list(x))
        if code != 0 or steps >= cap:
            break
    records = np.zeros((max_steps if max_steps else steps, WORDS))
    records[:steps] = rows
    return records, (ret, disc, steps, code, ties, x)


def evaluate(e, states, max_steps=0):
    """one replica: (dict of ret / disc / steps / terminal / ties [n] and final_state [n][3], list of the n episodes' records)"""
    states = np.asarray(states, np.float64)
    n = states.shape[0]
    out = dict(ret=np.zeros(n), disc=np.zeros(n), steps=np.zeros(n, np.int32), terminal=np.zeros(n, np.int32), ties=np.zeros(n, np.int32),
               final_state=np.zeros_like(states))
    records = []
    for s in range(n):
        rec, (r, d, k, c, t, x) = episode(e, states[s], max_steps)
        out["ret"][s], out["disc"][s], out["steps"][s], out["terminal"][s], out["ties"][s] = r, d, k, c, t
        out["final_state"][s] = x
        records.append(rec)
    return out, records
