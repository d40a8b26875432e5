#!/usr/bin/env python3
"""evaluate_ensemble_throughput.py [replicas [starts-per-side [trials [group-size [composed-groups]]]]] -- what an ensemble evaluation
costs: seconds per call, episodes/s, episode-steps/s (one environment step of one (group, start state) episode) and member-steps/s
(episode-steps x group size: the table probes of one member at one step) of
(a) grlx_evaluate_ensemble under both rules: all groups x all start states, whole episodes, one call each
    (evaluate_ensemble_kernel<pendulum, 3>), host arrays in and out,
(b) the path it replaces, composed from the entry points there were: per control step one grlx_query_ensemble per group (a query takes the
    cross product groups x observations, and every episode is at an observation of its own), the first maximum of its vote or sum-q
    columns in numpy, and one grlx_env_step over all episodes; on the first `composed-groups` groups (all by default).  It has no
    member_ties: grlx_query_ensemble does not return the members' n_max.
(c) grlx_evaluate on the same replicas and start states: the yardstick per member-step (the ensemble does the same probes and 1 / group
    size of the distinct environment steps).
on 4096 pendulum SARSA replicas after 100 trials in groups of 64, from a 16 x 16 grid of start states at time 0, by default.
Three runs of each, alternated in one process on one context after a warm-up call of each; legs (a) and (b) are compared bit for bit on
the groups both ran.  Run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner


def composed(r, cfg, states, actions, G, n_groups, rule):
    n, A = states.shape[0], len(actions)
    x = np.tile(states, (n_groups, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    eps = x.shape[0]
    ret, disc, g = np.zeros(eps), np.zeros(eps), np.ones(eps)
    steps, terminal, ties = np.zeros(eps, np.int32), np.zeros(eps, np.int32), np.zeros(eps, np.int32)
    agreement = np.zeros(eps, np.int64)
    active = np.ones(eps, bool)
    while active.any():
        cols = np.zeros((eps, 2 + 2 * A))
        for k in range(n_groups):
            # the query is the cross product: row s of group k's answer is episode (k, s)
            cols[k * n:(k + 1) * n] = r.query_ensemble_raw(obs[k * n:(k + 1) * n], G, replicas=(k * G, G))[0]
        votes = cols[:, 2 + A:]
        score = votes if rule == "vote" else cols[:, 2:2 + A]
        mai = score.argmax(axis=1)                                           # the first maximum
        man = (score == score.max(axis=1, keepdims=True)).sum(axis=1)
        nx, nobs, rew, term = runner.env_step(cfg, x, actions[mai])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        ties += active & (man > 1)
        agreement += np.where(active, votes[np.arange(eps), mai].astype(np.int64), 0)
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_groups, n)
    return dict(ret=ret.reshape(shape), disc=disc.reshape(shape), steps=steps.reshape(shape), terminal=terminal.reshape(shape),
                ties=ties.reshape(shape), agreement=agreement.reshape(shape), final_state=x.reshape(shape + (3,)))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    G = args[3] if len(args) > 3 else 64
    n_groups = n // G
    n_comp = min(args[4] if len(args) > 4 else n_groups, n_groups)
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)    # time 0: full episodes
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    legs = ["fused vote", "fused mean", "composed vote", "composed mean", "members"]
    reps = {"fused vote": 10, "fused mean": 10, "composed vote": 1, "composed mean": 1, "members": 10}
    res = {leg: [] for leg in legs}
    out, ep_steps, episodes = {}, {}, {}

    def call(leg):
        kind, _, rule = leg.partition(" ")
        if kind == "fused":
            return r.evaluate_ensemble(states, G, rule)._asdict()
        if kind == "composed":
            return composed(r, cfg, states, actions, G, n_comp, rule)
        return r.evaluate(states)._asdict()

    for leg in legs:                                                         # warm-up at the timed shape: code object load, first-touch pages
        t0 = time.perf_counter()
        out[leg] = call(leg)
        ep_steps[leg] = int(np.asarray(out[leg]["steps"]).sum())
        episodes[leg] = out[leg]["steps"].size
        print(f"warm-up {leg:14s} {time.perf_counter() - t0:9.4f} s", flush=True)
    for i in range(3):
        for leg in legs:
            t0 = time.perf_counter()
            for _ in range(reps[leg]):                                       # every call ends in a device-to-host copy: synchronised
                out[leg] = call(leg)
            dt = (time.perf_counter() - t0) / reps[leg]
            res[leg].append(dt)
            print(f"run {i}  {leg:14s} {episodes[leg]:8d} episodes {dt:9.4f} s/call  {episodes[leg] / dt / 1e3:11.3f} k episodes/s"
                  f"  {ep_steps[leg] / dt / 1e6:9.3f} M episode-steps/s", flush=True)
    for rule in ("vote", "mean"):
        a, b = out["fused " + rule], out["composed " + rule]
        for name, v in b.items():
            assert np.ascontiguousarray(a[name][:n_comp]).tobytes() == np.ascontiguousarray(v.astype(a[name].dtype)).tobytes(), f"{rule}: the two legs differ in {name}"
    print(f"legs (a) and (b) agree bit for bit under both rules on the {n_comp} groups both ran (member_ties: (a) only)")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        members = 1 if leg == "members" else G
        print(f"{leg:14s} median {med[leg]:.4f} s/call  min {min(v):.4f}  max {max(v):.4f}  {ep_steps[leg] / med[leg] / 1e6:10.3f} M episode-steps/s"
              f"  {ep_steps[leg] * members / med[leg] / 1e6:10.3f} M member-steps/s")
    for rule in ("vote", "mean"):
        f, c = ep_steps["fused " + rule] / med["fused " + rule], ep_steps["composed " + rule] / med["composed " + rule]
        print(f"{rule}: fused / composed (episode-steps/s at the medians): {f / c:.1f}x;  fused member-steps/s / grlx_evaluate's: "
              f"{f * G / (ep_steps['members'] / med['members']):.2f}x")
    v = out["fused vote"]
    print(f"vote: ties at {100.0 * v['ties'].sum() / v['steps'].sum():.2f} % of the steps, agreement {100.0 * v['agreement'].sum() / (v['steps'].sum() * G):.2f} %,"
          f" member ties at {100.0 * v['member_ties'].sum() / (v['steps'].sum() * G):.2f} % of the member-steps")
    r.close()


if __name__ == "__main__":
    main()
