#!/usr/bin/env python3
"""evaluate_actor_ensemble_throughput.py [replicas [starts [trials [group-size [composed-groups]]]]] -- what an evaluation of an ensemble of
actors costs: seconds per call, episode-steps/s (one environment step of one (group, start state) episode) and member-steps/s
(episode-steps x group size: the actor probes of one member at one step) of
(a) grlx_evaluate_actor_ensemble under its four rules (mean; binning, 64 bins; data_center, half the group kept; density, r = 0.05): all
    groups x all start states, whole episodes, one call each (actor_ensemble_kernel<cart-pole, false>), host arrays in and out,
(b) the path it replaces, composed from the entry points there were: per control step one grlx_query_state of the actor's table per group
    (a query takes the cross product members x observations, and every episode is at an observation of its own), the clip and the rule
    in numpy -- serial over the members, vectorised over the episodes, the exponentials through grlx_math --, and one grlx_env_step over
    all episodes; on the first `composed-groups` groups only (2 by default), compared with (a) bit for bit on those groups,
(c) grlx_evaluate on the same replicas and start states: the yardstick per member-step (the ensemble does the same probes and 1 / group
    size of the environment steps),
on 16384 cart-pole actor-critic replicas (BASELINE configuration 3) after 20 trials in groups of 64, from 16 start states at time 0, by
default.  Three runs of each leg (a run: ten calls; a composed leg: one), alternated in one process on one context after a warm-up call
of each; the clock stops after the device-to-host copy.  Also printed per fused leg: the device time of its launches
(grlx_read_kernel_timing, in a pass of its own after the timed runs).  Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner
from tests import configs, oracle_binding as ob, policy_evaluate_ref as ev


def serial_sum(a, take):
    """per episode the sum of a[:, i] over the members with take[:, i], ascending, starting from the first one taken and not from 0.0"""
    s, started = np.zeros(a.shape[0]), np.zeros(a.shape[0], bool)
    for i in range(a.shape[1]):
        s = np.where(take[:, i], np.where(started, s + a[:, i], a[:, i]), s)
        started |= take[:, i]
    return s


def combine(a, rule, bins, r, lo, hi):
    """(action, tie?, kept) per episode of the members' actions a[episode][member]: include/grlx.h's serial loops, vectorised over episodes"""
    eps, G = a.shape
    everyone = np.ones(a.shape, bool)
    if rule == "mean":
        return serial_sum(a, everyone) / float(G), np.zeros(eps, bool), np.full(eps, G)
    if rule == "binning":
        b = np.minimum(np.floor((float(bins) * (a - lo)) / (hi - lo)).astype(np.int64), bins - 1)
        count = (b[:, :, None] == b[:, None, :]).sum(axis=2)
        most = count.max(axis=1)
        take = count == most[:, None]
        s = np.zeros(eps)
        for i in range(G):
            s = np.where(take[:, i], s + a[:, i], s)
        n = take.sum(axis=1)
        return s / n, n // most > 1, n
    if rule == "data_center":
        alive, tie = everyone.copy(), np.zeros(eps, bool)
        mean = serial_sum(a, alive) / alive.sum(axis=1)
        for _ in range(max(G - bins, 0)):
            d = np.where(alive, (a - mean[:, None]) * (a - mean[:, None]), -1.0)
            far = d.max(axis=1)
            tie |= (d == far[:, None]).sum(axis=1) > 1
            alive[np.arange(eps), d.argmax(axis=1)] = False             # the first of the greatest
            mean = serial_sum(a, alive) / alive.sum(axis=1)
        return mean, tie, alive.sum(axis=1)
    n = -1 + 2 * ((a - lo) / (hi - lo))
    d = n[:, :, None] - n[:, None, :]
    e = runner.device_math(runner.MATH_EXP, ((-1 * (d * d)) / (r * r)).reshape(-1)).reshape(eps, G, G)
    rho = np.zeros((eps, G))
    for j in range(G):
        rho += e[:, :, j]
    best = rho.max(axis=1)
    return a[np.arange(eps), rho.argmax(axis=1)], (rho == best[:, None]).sum(axis=1) > 1, np.ones(eps, np.int64)


def composed(r, cfg, spec, states, G, n_groups, rule, bins, rad):
    n = states.shape[0]
    x = np.tile(states, (n_groups, 1))
    obs = np.tile(np.array([ev.observe(spec, s)[0] for s in states]), (n_groups, 1))
    eps = x.shape[0]
    ret, disc, g, spread = np.zeros(eps), np.zeros(eps), np.ones(eps), np.zeros(eps)
    steps, terminal, ties = (np.zeros(eps, np.int32) for _ in range(3))
    kept = np.zeros(eps, np.int64)
    active = np.ones(eps, bool)
    while active.any():
        a = np.zeros((eps, G))
        for k in range(n_groups):
            # the query is the cross product: column s of group k's answer is episode (k, s)
            a[k * n:(k + 1) * n] = r.query_state(obs[k * n:(k + 1) * n], 1, replicas=(k * G, G)).T
        a = np.minimum(np.maximum(a, cfg.action_min), cfg.action_max)
        action, tie, k_step = combine(a, rule, bins, rad, cfg.action_min, cfg.action_max)
        nx, nobs, rew, term = runner.env_step(cfg, x, action)
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        ties += active & tie
        kept += np.where(active, k_step, 0)
        spread = np.where(active, spread + (a.max(axis=1) - a.min(axis=1)), spread)
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_groups, n)
    return grl_amd.ActorEnsembleEvaluation(ret.reshape(shape), disc.reshape(shape), steps.reshape(shape), terminal.reshape(shape), ties.reshape(shape),
                                           kept.reshape(shape), spread.reshape(shape), x.reshape(shape + (states.shape[1],)))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 16384
    starts = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 20
    G = args[3] if len(args) > 3 else 64
    n_comp = min(args[4] if len(args) > 4 else 2, n // G)
    cfg, spec = configs.cart_pole_ac(grl_amd, n, max_rows=trials // 10 + 2)
    spec.math = ob.MATH_PORTABLE
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    # the cart at rest in the middle, the pole from hanging to nearly upright, time 0: full episodes
    states = np.array([[0.0, np.pi * (1 - i / starts), 0.0, 0.0, 0.0] for i in range(starts)])
    rules = {"mean": (10, 0.001), "binning": (64, 0.001), "data_center": (max(G // 2, 1), 0.001), "density": (10, 0.05)}
    calls = {"members": lambda: r.evaluate(states)}
    for rule, (bins, rad) in rules.items():
        calls["fused " + rule] = lambda rule=rule, bins=bins, rad=rad: r.evaluate_actor_ensemble(states, G, rule, bins, rad)
        if n_comp > 0:
            calls["composed " + rule] = lambda rule=rule, bins=bins, rad=rad: composed(r, cfg, spec, states, G, n_comp, rule, bins, rad)
    out, ep_steps, res = {}, {}, {leg: [] for leg in calls}
    for leg in calls:                                                        # warm-up at the timed shape: code object load, first-touch pages
        t0 = time.perf_counter()
        out[leg] = calls[leg]()
        ep_steps[leg] = int(np.asarray(out[leg].steps).sum())
        print(f"warm-up {leg:20s} {time.perf_counter() - t0:9.4f} s", flush=True)
    for i in range(3):
        for leg in calls:
            reps = 1 if leg.startswith("composed") else 10
            t0 = time.perf_counter()
            for _ in range(reps):                                            # every call ends in a device-to-host copy: synchronised
                out[leg] = calls[leg]()
            dt = (time.perf_counter() - t0) / reps
            res[leg].append(dt)
            print(f"run {i}  {leg:20s} {out[leg].steps.size:8d} episodes {dt:9.4f} s/call  {ep_steps[leg] / dt / 1e6:9.3f} M episode-steps/s", flush=True)
    for rule in rules:
        if n_comp > 0:
            for name, a, b in zip(grl_amd.ActorEnsembleEvaluation._fields, out["fused " + rule], out["composed " + rule]):
                assert np.ascontiguousarray(a[:n_comp]).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"{rule}: the two legs differ in {name}"
    if n_comp > 0:
        print(f"the fused and the composed legs agree bit for bit under all four rules on the {n_comp} groups both ran")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        members = 1 if leg == "members" else G
        print(f"{leg:20s} median {med[leg]:.4f} s/call  min {min(v):.4f}  max {max(v):.4f}  {ep_steps[leg] / med[leg] / 1e6:10.3f} M episode-steps/s"
              f"  {ep_steps[leg] * members / med[leg] / 1e6:10.3f} M member-steps/s")
    for rule in rules:
        f = ep_steps["fused " + rule] / med["fused " + rule]
        line = f"{rule}: fused member-steps/s / grlx_evaluate's: {f * G / (ep_steps['members'] / med['members']):.2f}x"
        if n_comp > 0:
            line += f";  fused / composed (episode-steps/s at the medians): {f / (ep_steps['composed ' + rule] / med['composed ' + rule]):.1f}x"
        v = out["fused " + rule]
        print(line + f";  ties at {100.0 * v.ties.sum() / v.steps.sum():.2f} % of the steps, kept {v.kept.sum() / v.steps.sum():.2f} members per step, "
              f"spread {v.spread.sum() / v.steps.sum():.3f} per step")
    ms, chunks = C.c_double(0), C.c_int(0)
    for leg in calls:
        if leg.startswith("composed"):
            continue
        r.lib.grlx_read_kernel_timing(1, None, None)
        for _ in range(3):
            calls[leg]()
        r.lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks))
        print(f"{leg:20s} device time of the launches: {ms.value / 3:.3f} ms per call ({chunks.value // 3} chunk(s)); {ep_steps[leg] / (ms.value / 3) / 1e3:.3f} M episode-steps/s")
    r.close()


if __name__ == "__main__":
    main()
