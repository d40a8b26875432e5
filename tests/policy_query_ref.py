"""Reference of the policy queries (grlx_query_q / _state / _ensemble), from an oracle experiment's DENSE parameter vectors and the
oracle's projector.  Plain Python float loops, no vectorised sums: the serial order is the specification.

  q[a]     = clip(((w0 + w1) + ... + w15) / 16, output_min, output_max) over the slots of project(obs, action a)   (q.cpp:94-107)
  findmax  = first maximum and number of maxima                                                                    (greedy.cpp:47-61)
  value    = v = 0; for a in order: v += q[a] * dist[a], dist[a] = 1. / man at the maxima, 0 elsewhere       (q.cpp:56-68, greedy.cpp:88-98)
  state    = the same read over project(obs) of a table whose projector takes the observation alone
  ensemble = {sum value, sum value * value, sum q[a], votes[a]} over the group's replicas in ascending order, one accumulator each
"""
import ctypes as C

import numpy as np

from tests import oracle_binding as ob


def actions_of(spec):
    """UniformDiscretizer::configure (uniform.cpp:60-95)"""
    n = int(spec.action_steps)
    delta = (spec.action_max - spec.action_min) / (float(n) - 1) if n != 1 else 0.0
    return [spec.action_min + delta * k for k in range(n)]


def dense(e, table=0):
    """the oracle's dense parameter vector of `table` as it stands (a view, not a copy: 64 MiB at the default memory)"""
    n = e.spec.actor_projector.memory if table == 1 else e.spec.projector.memory
    return np.ctypeslib.as_array(e.L.orc_weights(e.h, table), shape=(n,))


def lin_read(w, slots, lin):
    s = 0.0
    for j in slots:
        s += float(w[int(j)])
    s /= float(len(slots))
    return min(max(s, lin.output_min), lin.output_max)


def findmax(q):
    mai, man = 0, 1
    for ii in range(1, len(q)):
        if q[ii] > q[mai]:
            mai, man = ii, 1
        elif q[ii] == q[mai]:
            man += 1
    return mai, man


def value_of(q):
    mai, man = findmax(q)
    v = 0.0
    for ii in range(len(q)):
        v += q[ii] * (1.0 / man if q[ii] == q[mai] else 0.0)
    return v


def query_q(w, spec, obs):
    """(q[n][A], value[n], greedy[n], n_max[n]) of one replica whose table 0 is the dense vector w"""
    acts = actions_of(spec)
    obs = np.asarray(obs, np.float64)
    q = np.zeros((obs.shape[0], len(acts)), np.float64)
    value = np.zeros(obs.shape[0], np.float64)
    greedy = np.zeros(obs.shape[0], np.int32)
    n_max = np.zeros(obs.shape[0], np.int32)
    for o in range(obs.shape[0]):
        rows = [list(obs[o]) + [a] for a in acts]
        slots = ob.tile_project(spec.projector, rows)
        qa = [lin_read(w, slots[a], spec.representation) for a in range(len(acts))]
        q[o] = qa
        greedy[o], n_max[o] = findmax(qa)
        value[o] = value_of(qa)
    return q, value, greedy, n_max


def query_state(w, spec, table, obs):
    """the read of table 0 (spec.projector / representation) or 1 (actor_projector / actor_representation) over obs alone"""
    ts, lin = (spec.actor_projector, spec.actor_representation) if table == 1 else (spec.projector, spec.representation)
    obs = np.asarray(obs, np.float64)
    slots = ob.tile_project(ts, obs)
    return np.array([lin_read(w, slots[o], lin) for o in range(obs.shape[0])], np.float64)


def ensemble(q, value, greedy, group_size):
    """raw sums [group][obs][2 + 2A] from per-replica results q[R][n][A], value[R][n], greedy[R][n]"""
    R, n, A = q.shape
    assert R % group_size == 0
    out = np.zeros((R // group_size, n, 2 + 2 * A), np.float64)
    for g in range(R // group_size):
        for o in range(n):
            sv = svv = 0.0
            sq = [0.0] * A
            votes = [0.0] * A
            for r in range(g * group_size, (g + 1) * group_size):
                v = float(value[r, o])
                sv += v
                svv += v * v
                for a in range(A):
                    sq[a] += float(q[r, o, a])
                    votes[a] += 1.0 if int(greedy[r, o]) == a else 0.0
            out[g, o] = [sv, svv] + sq + votes
    return out


def scaling(ts):
    """TileCodingProjector::configure (tile_coding.cpp:45-80): tilings / resolution"""
    return [ts.tilings / ts.resolution[i] for i in range(ts.dims)]


def observation_set(ts, obs_dims, visited):
    """The 11 observations every test queries (11 x 3, 5 or 13 replicas is no multiple of 4: the last wave has dead groups):
    3 the oracle visited, 2 far from anything visited, 3 with negative / beyond-one-wrap angles on the wrapped dimensions (any sign
    elsewhere), 2 on exact tile boundaries k / scaling, and zero."""
    sc = scaling(ts)
    visited = [list(v)[:obs_dims] for v in visited]
    assert len(visited) >= 3
    pick = [visited[0], visited[len(visited) // 2], visited[-1]]
    far = [[1000.37 + 3 * i for i in range(obs_dims)], [-977.21 - 5 * i for i in range(obs_dims)]]
    wrapped = [i for i in range(obs_dims) if ts.wrapping[i] != 0]
    ang = []
    for base, neg, beyond in ((0.11, -1.3, 7.9), (-0.42, -13.0, 20.5), (0.27, -0.001, 6.2831)):
        row = [base * (i + 1) * (-1) ** i for i in range(obs_dims)]
        for n, i in enumerate(wrapped):
            row[i] = neg if n % 2 == 0 else beyond
        if not wrapped:
            row[0] = neg
        ang.append(row)
    ang[1] = [(-x if i not in wrapped else 20.5) for i, x in enumerate(ang[1])]
    bound = [[(5 - 2 * i) / sc[i] for i in range(obs_dims)], [(-3 + i) / sc[i] for i in range(obs_dims)]]
    rows = pick + far + ang + bound + [[0.0] * obs_dims]
    assert len(rows) == 11
    return np.array(rows, np.float64)


def visited_observations(spec, seed, trials=3, cap=400):
    """observations the oracle's taps recorded in `trials` trials of a fresh experiment"""
    e = ob.Experiment(spec, seed=int(seed))
    taps = e.run(trials, tap_cap=cap)[1]
    D = e.L.orc_env_obs_dims(spec.env)
    e.close()
    return [list(t.obs[:D]) for t in taps]
