#!/usr/bin/env python3
"""fqi_evaluate_ensemble_throughput.py [replicas [group-size [starts-per-side [batches]]]] -- what an ensemble evaluation of the batch
path costs: seconds per call and member-steps/s (one member-step = one member's A forward passes at one step of one (group, start
state) episode) of
(a) grlx_fqi_evaluate_ensemble: all groups x all start states, whole episodes, in one call (fqi_evaluate_ensemble_kernel<20, false>), host
    arrays in and out, under each rule,
(b) the path there was before: per control step one grlx_fqi_query per group (a query takes the cross product replicas x observations,
    and every group is at observations of its own), findmax, the votes and the serial sums over the members in numpy, and one
    grlx_env_step over all episodes; its first observation comes from the device's own fmod (grlx_math), and
(c) grlx_fqi_evaluate on the same replicas and start states, for the rate per member and step of the single policy's kernel,
on 64 replicas of the reference's pendulum-fqi-ann.yaml (hidden = 20) in 4 groups of 16 after two batches, from a 16 x 16 grid of start
states at time 0 (1024 episodes of 100 steps) by default.  Three runs of each leg, alternated in one process on one context after a
warm-up call of each; medians.  (a) and (b) are compared bit for bit in all eight outputs, under both rules.  Run it under a time limit
of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner

VOTE, MEAN = "vote", "mean"


def composed(r, ecfg, gamma_tau, states, actions, groups, G, rule):
    n, A = states.shape[0], len(actions)
    x = np.tile(states, (groups, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    pairs = x.shape[0]
    ret, disc, g = np.zeros(pairs), np.zeros(pairs), np.ones(pairs)
    steps, terminal, ties = np.zeros(pairs, np.int32), np.zeros(pairs, np.int32), np.zeros(pairs, np.int32)
    mties, agree = np.zeros(pairs, np.int64), np.zeros(pairs, np.int64)
    active = np.ones(pairs, bool)
    rows = np.arange(pairs)
    while active.any():
        votes, sumq, mt = np.zeros((pairs, A), np.int64), np.zeros((pairs, A)), np.zeros(pairs, np.int64)
        for k in range(groups):
            q = r.query(obs[k * n:(k + 1) * n], replicas=(k * G, G))           # [member][start][action]
            sl = slice(k * n, (k + 1) * n)
            for m in range(G):                                                 # ascending, one accumulator per action
                sumq[sl] = sumq[sl] + q[m]
                votes[sl][rows[:n], np.argmax(q[m], axis=1)] += 1              # the first maximum; votes[sl] is a view
                mt[sl] += (q[m] == q[m].max(axis=1, keepdims=True)).sum(axis=1) > 1
        score = votes.astype(np.float64) if rule == VOTE else sumq
        mai = np.argmax(score, axis=1)                                         # the first maximum
        n_max = (score == score.max(axis=1, keepdims=True)).sum(axis=1)
        nx, nobs, rew, term = runner.env_step(ecfg, x, actions[mai])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * gamma_tau, g)
        steps += active
        ties += active & (n_max > 1)
        mties += np.where(active, mt, 0)
        agree += np.where(active, votes[rows, mai], 0)
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (groups, n)
    return grl_amd.EnsembleEvaluation(ret.reshape(shape), disc.reshape(shape), steps.reshape(shape), terminal.reshape(shape), ties.reshape(shape),
                                      mties.reshape(shape), agree.reshape(shape), x.reshape(shape + (3,)))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 64
    G = args[1] if len(args) > 1 else 16
    side = args[2] if len(args) > 2 else 16
    batches = args[3] if len(args) > 3 else 2
    groups = n // G
    cfg = grl_amd.pendulum_fqi_config(n, max_batches=batches)
    r = grl_amd.FqiRunner(cfg, np.arange(1, n + 1))
    for _ in range(batches):
        r.run_batch()
    r.sync()
    ecfg = grl_amd.pendulum_sarsa_config(1, control_step=cfg.control_step, integration_steps=cfg.integration_steps, timeout=cfg.timeout)
    gamma_tau = float(cfg.gamma) ** float(cfg.control_step)
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)    # time 0: full episodes
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    legs = [("fused", VOTE), ("fused", MEAN), ("composed", VOTE), ("composed", MEAN), ("single", None)]
    res = {leg: [] for leg in legs}
    out, member_steps = {}, {}

    def call(leg):
        kind, rule = leg
        if kind == "fused":
            return r.evaluate_ensemble(states, G, rule=rule)
        if kind == "composed":
            return composed(r, ecfg, gamma_tau, states, actions, groups, G, rule)
        return r.evaluate(states)

    for leg in legs:                                                         # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = call(leg)
        member_steps[leg] = int(np.asarray(out[leg].steps).sum()) * (1 if leg[0] == "single" else G)
    reps = {"fused": 100, "composed": 1, "single": 100}                      # calls per timed window
    for i in range(3):
        for leg in legs:
            t0 = time.perf_counter()
            for _ in range(reps[leg[0]]):                                    # every call ends in a device-to-host copy: synchronised
                out[leg] = call(leg)
            dt = (time.perf_counter() - t0) / reps[leg[0]]
            res[leg].append(dt)
            print(f"{n} replicas in {groups} groups of {G} x {states.shape[0]} starts  run {i}  {leg[0]:9s} {str(leg[1]):5s} {dt:9.5f} s/call"
                  f"  {member_steps[leg] / dt / 1e6:9.3f} M member-steps/s", flush=True)
    for rule in (VOTE, MEAN):
        same = True
        for name, a, b in zip(grl_amd.EnsembleEvaluation._fields, out[("fused", rule)], out[("composed", rule)]):
            if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(np.asarray(b).astype(a.dtype)).tobytes():
                same = False
                print(f"rule {rule}: fused and composed DIFFER in {name}")
        e = out[("fused", rule)]
        print(f"rule {rule}: fused and composed agree bit for bit in all eight outputs: {same}; ties in {int((e.ties > 0).sum())} of {e.ties.size} episodes,"
              f" agreement {e.agreement.sum() / (e.steps.sum() * G):.3f}, mean return {e.ret.mean():.1f}")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    rate = {leg: member_steps[leg] / med[leg] for leg in legs}
    for leg, v in res.items():
        print(f"{leg[0]:9s} {str(leg[1]):5s} median {med[leg]:.5f} s/call  {rate[leg] / 1e6:.3f} M member-steps/s  min {min(v):.5f} s  max {max(v):.5f} s")
    for rule in (VOTE, MEAN):
        print(f"rule {rule}: fused / composed (member-steps/s at the medians): {rate[('fused', rule)] / rate[('composed', rule)]:.1f}x;"
              f" fused / single policy per member-step: {rate[('fused', rule)] / rate[('single', None)]:.2f}x")
    print(f"mean return of the single policies: {out[('single', None)].ret.mean():.1f}")
    r.close()


if __name__ == "__main__":
    main()
