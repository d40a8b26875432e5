#!/usr/bin/env python3
"""fqi_evaluate_ensemble_sampled_throughput.py [hidden [replicas]] -- what a sampled ensemble evaluation of the batch path costs beside the
greedy one: seconds per call of
(a) grlx_fqi_evaluate_ensemble under `vote` (one lane per episode walks its group's members),
(b) grlx_fqi_evaluate_ensemble_sampled under majority / greedy members and under rank / softmax members (a row of 16 lanes per episode),
on `replicas` (64) initial networks of the reference's pendulum-fqi-ann.yaml in groups of 4, 16 and 64, from 256 and from 4096 start states at
time 0 (100-step episodes whatever the policy: the pendulum only times out),
(c) the composed path on ONE group of 16 x 256 start states: per control step one grlx_fqi_query, the members' distributions, the scores, the
    combined softmax (the device's pexp through grlx_math) and the draw in numpy, one grlx_env_step -- compared with (b) on the same group
    and streams bit for bit in all ten outputs (an assertion), and
(d) grlx_fqi_evaluate and grlx_fqi_evaluate_sampled (epsilon = 0.1) on 16 replicas x 256 start states.
One process, one context; a warm-up call of every leg at its shape, then three windows of `REPS` calls per leg (a composed leg: one),
alternated; medians.  Every call ends in a device-to-host copy, so a window is synchronised.  Run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner
from tools.evaluate_ensemble_sampled_throughput import act      # the step of include/grlx.h in numpy, q[episode][member][action]

REPS = 50
SETTINGS = {"majority / greedy": ("majority", 1.0, "greedy", None), "rank / softmax": ("rank", 16.0, "softmax", 1e-6)}


def composed(r, ecfg, gamma_tau, states, actions, G, rank, tau, tau_m, streams):
    """one group, the replicas 0 ... G - 1: SampledEnsembleEvaluation [1][n]"""
    x = states.copy()
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    obs = np.stack([np.where(a < 0, a + 2 * np.pi, a), x[:, 1]], axis=1)
    eps = x.shape[0]
    rng = streams.reshape(-1).copy()
    ret, disc, g = np.zeros(eps), np.zeros(eps), np.ones(eps)
    steps, terminal, ties, explored = (np.zeros(eps, np.int32) for _ in range(4))
    member_ties, agreement = np.zeros(eps, np.int64), np.zeros(eps, np.int64)
    active = np.ones(eps, bool)
    while active.any():
        q = r.query(obs, replicas=(0, G)).transpose(1, 0, 2)                   # [member][start][action] -> [start][member][action]
        idx, tie, off, agree, mties = act(q, rank, tau, tau_m, rng, active)
        nx, nobs, rew, term = runner.env_step(ecfg, x, actions[idx])
        ret, disc, g = np.where(active, ret + rew, ret), np.where(active, disc + g * rew, disc), np.where(active, g * gamma_tau, g)
        steps += active
        ties += active & tie
        explored += active & off
        member_ties += np.where(active, mties, 0)
        agreement += np.where(active, agree, 0)
        terminal = np.where(active, term, terminal)
        x, obs = np.where(active[:, None], nx, x), np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    return grl_amd.SampledEnsembleEvaluation(*(v.reshape(1, eps) for v in (ret, disc, steps, terminal, ties, member_ties, agreement, explored)),
                                             x.reshape(1, eps, 3), rng.reshape(1, eps))


def main():
    hidden = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    cfg = grl_amd.pendulum_fqi_config(n, max_batches=1, hidden=hidden)
    r = grl_amd.FqiRunner(cfg, np.arange(1, n + 1))
    ecfg = grl_amd.pendulum_sarsa_config(1, control_step=cfg.control_step, integration_steps=cfg.integration_steps, timeout=cfg.timeout)
    gamma_tau = float(cfg.gamma) ** float(cfg.control_step)
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    legs, pairs = {}, []
    for side in (16, 64):
        grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
        states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)
        for G in (4, 16, 64):
            tag = f"{n // G:2d} groups of {G:2d} x {states.shape[0]:4d} starts"
            legs[f"{tag}  greedy vote"] = lambda s=states, G=G: r.evaluate_ensemble(s, G, rule="vote")
            for name, (strategy, tau, member, param) in SETTINGS.items():
                legs[f"{tag}  sampled {name}"] = lambda s=states, G=G, a=(strategy, float(G) if strategy == "rank" else tau, member, param): \
                    r.evaluate_ensemble_sampled(s, G, *a)
        if side == 16:
            words = grl_amd.episode_stream_words(5, 1, states.shape[0])
            for name, (strategy, tau, member, param) in SETTINGS.items():
                fused, comp = f" 1 group  of 16 x  256 starts  sampled {name}, streams given", f" 1 group  of 16 x  256 starts  composed {name}"
                legs[fused] = lambda s=states, a=(strategy, tau, member, param): r.evaluate_ensemble_sampled(s, 16, *a, streams=words, replicas=(0, 16))
                legs[comp] = lambda s=states, a=(strategy == "rank", tau, param): composed(r, ecfg, gamma_tau, s, actions, 16, *a, words)
                pairs.append((fused, comp))
            streams = grl_amd.episode_streams(1, 16, states.shape[0])
            legs["16 replicas x  256 starts  evaluate"] = lambda s=states: r.evaluate(s, replicas=(0, 16))
            legs["16 replicas x  256 starts  evaluate_sampled, epsilon 0.1"] = lambda s=states, st=streams: r.evaluate_sampled(s, "epsilon", 0.1, st, (0, 16))
    res, out = {k: [] for k in legs}, {}
    for k, call in legs.items():
        out[k] = call()                                                     # warm-up at the timed shape
        assert (out[k].steps == 100).all(), k
    for fused, comp in pairs:
        for name, a, b in zip(grl_amd.SampledEnsembleEvaluation._fields, out[fused], out[comp]):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(np.asarray(b).astype(a.dtype)).tobytes(), f"{comp}: {name} differs from the call's"
        print(f"{comp.strip()}: bit for bit the call's ten outputs; explored {int(out[fused].explored.sum())} of {int(out[fused].steps.sum())} steps", flush=True)
    for i in range(3):
        for k, call in legs.items():
            reps = 1 if "composed" in k else REPS
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            res[k].append((time.perf_counter() - t0) / reps)
    for k, v in res.items():
        print(f"hidden {hidden}  {k:62s} median {sorted(v)[1] * 1e3:8.3f} ms/call  min {min(v) * 1e3:8.3f}  max {max(v) * 1e3:8.3f}", flush=True)
    r.close()


if __name__ == "__main__":
    main()
