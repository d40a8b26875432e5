#!/usr/bin/env python3
"""evaluate_noisy_throughput.py [replicas [starts [trials [composed-replicas]]]] -- what a noisy evaluation of the actor-critic costs:
seconds per call, episodes/s and pair-steps/s (one pair-step = one environment step of one (replica, start state) pair) of
(a) grlx_evaluate_noisy at sigma = 5, theta = 1 and (b) at sigma = 0 (no draw: the noise-free actor through the noisy kernel), both on the
    streams of grlx_episode_stream_words, all replicas x all start states, whole episodes, one call each (evaluate_noisy_kernel<cart-pole>),
(c) grlx_evaluate at the same shape (evaluate_ac_kernel<cart-pole>; with GRLX_LIB naming the parent commit's library this leg alone runs:
    the parent's figure, taken in a process of its own on the same box), and
(d) the path (a) replaces, composed from the entry points there were: per control step one grlx_query_state of the actor's table per
    replica, the two draws and Box-Muller in numpy over the oracle's portable log and cos (the 48-bit generator in numpy's uint64), the
    clip, one grlx_env_step over all pairs, the sums in numpy -- on the first `composed-replicas` replicas only (8 by default), compared
    with (a) bit for bit on those replicas, streams, noise and clipped included,
on 16384 cart-pole actor-critic replicas (BASELINE configuration 3) after 20 trials from 16 start states at time 0 (262144 episodes to the
timeout) by default.  Three runs of each leg (a run: ten calls; the composed leg: one), alternated in one process on one context after a
warm-up call of each; the clock stops after the device-to-host copy.  Also printed per fused leg: the device time of its launches
(grlx_read_kernel_timing, in a pass of its own after the timed runs).  Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner
from tests import configs, oracle_binding as ob, policy_evaluate_ref as ev

A48, C48, MASK = np.uint64(0x5DEECE66D), np.uint64(0xB), np.uint64((1 << 48) - 1)


def lcg(x):
    return (A48 * x + C48) & MASK          # uint64 arithmetic wraps modulo 2^64: the low 48 bits are exact


def composed(r, cfg, spec, states, n_rep, sigma, theta, streams):
    L = ob.load()
    plog, pcos = np.vectorize(lambda v: float(L.orc_plog(float(v)))), np.vectorize(lambda v: float(L.orc_pcos(float(v))))
    n = states.shape[0]
    x = np.tile(states, (n_rep, 1))
    obs = np.tile(np.array([ev.observe(spec, s)[0] for s in states]), (n_rep, 1))
    pairs = x.shape[0]
    TL, noise = streams[:n_rep].reshape(-1).copy(), np.zeros(pairs)
    ret, disc, g = np.zeros(pairs), np.zeros(pairs), np.ones(pairs)
    steps, terminal, clipped = (np.zeros(pairs, np.int32) for _ in range(3))
    active = np.ones(pairs, bool)
    while active.any():
        u = np.zeros(pairs)
        for k in range(n_rep):
            u[k * n:(k + 1) * n] = r.query_state(obs[k * n:(k + 1) * n], 1, replicas=(k, 1))[0]
        noise = np.where(active & (x[:, -1] == 0), 0.0, noise)
        out = u
        if sigma != 0:
            T1 = lcg(TL)
            T2 = lcg(T1)
            U1, U2 = T1.astype(np.float64) * 2.0 ** -48, T2.astype(np.float64) * 2.0 ** -48
            with np.errstate(invalid="ignore"):
                nrm = np.sqrt(-2 * plog(U1)) * pcos(2 * np.pi * U2) * sigma + 0.
            moved = (1 - theta) * noise + nrm
            noise = np.where(active, moved, noise)
            TL = np.where(active, T2, TL)
            out = u + noise
        clipped += active & ((out < cfg.action_min) | (out > cfg.action_max))
        action = np.minimum(np.maximum(out, cfg.action_min), cfg.action_max)
        nx, nobs, rew, term = runner.env_step(cfg, x, action)
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_rep, n)
    return grl_amd.NoisyEvaluation(ret.reshape(shape), disc.reshape(shape), steps.reshape(shape), terminal.reshape(shape), clipped.reshape(shape),
                                   x.reshape(shape + (states.shape[1],)), TL.reshape(shape), noise.reshape(shape))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 16384
    starts = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 20
    n_rep = min(args[3] if len(args) > 3 else 8, n)
    cfg, spec = configs.cart_pole_ac(grl_amd, n, max_rows=trials // 10 + 2)
    spec.math = ob.MATH_PORTABLE
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    # the cart at rest in the middle, the pole from hanging to nearly upright, time 0: full episodes
    states = np.array([[0.0, np.pi * (1 - i / starts), 0.0, 0.0, 0.0] for i in range(starts)])
    noisy = hasattr(r.lib, "grlx_evaluate_noisy")                            # GRLX_LIB may name the parent's library: leg (c) alone
    streams = grl_amd.episode_stream_words(7, n, starts) if noisy else None
    calls = {"evaluate": lambda: r.evaluate(states)}
    if noisy:
        calls["sigma 5"] = lambda: r.evaluate_noisy(states, 5.0, 1.0, streams)
        calls["sigma 0"] = lambda: r.evaluate_noisy(states, 0.0, 1.0, streams)
        if n_rep > 0:
            calls["composed"] = lambda: composed(r, cfg, spec, states, n_rep, 5.0, 1.0, streams)
    out, pair_steps, res = {}, {}, {leg: [] for leg in calls}
    for leg in calls:                                                        # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = calls[leg]()
        pair_steps[leg] = int(np.asarray(out[leg].steps).sum())
    for i in range(3):
        for leg in calls:
            reps = 1 if leg == "composed" else 10
            t0 = time.perf_counter()
            for _ in range(reps):                                            # every call ends in a device-to-host copy: synchronised
                out[leg] = calls[leg]()
            dt = (time.perf_counter() - t0) / reps
            res[leg].append(dt)
            nr = n_rep if leg == "composed" else n
            print(f"{nr} replicas x {starts} starts  run {i}  {leg:9s} {dt:9.4f} s/call  {nr * starts / dt / 1e3:11.3f} k episodes/s"
                  f"  {pair_steps[leg] / dt / 1e6:9.3f} M pair-steps/s", flush=True)
    if "composed" in calls:
        for name, a, b in zip(grl_amd.NoisyEvaluation._fields, out["sigma 5"], out["composed"]):
            assert np.ascontiguousarray(a[:n_rep]).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"the composed leg differs in {name}"
        print(f"sigma 5 and the composed leg agree bit for bit on the {n_rep} replicas both ran (clipped there: {int(out['composed'].clipped.sum())} steps)")
    if noisy:
        e, z = out["evaluate"], out["sigma 0"]
        same = all(np.array_equal(getattr(e, f), getattr(z, f)) for f in ("ret", "disc", "steps", "terminal", "final_state"))
        print(f"sigma 0 equals grlx_evaluate: {same}; clipped at sigma 5: {int(out['sigma 5'].clipped.sum())} of {pair_steps['sigma 5']} steps")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        print(f"{leg:9s} median {med[leg]:.4f} s/call  {pair_steps[leg] / med[leg] / 1e6:.3f} M pair-steps/s  min {min(v):.4f} s  max {max(v):.4f} s")
    if noisy:
        for leg in ("sigma 5", "sigma 0"):
            print(f"{leg} / evaluate (s/call at the medians): {med[leg] / med['evaluate']:.3f}")
        if "composed" in calls:
            print(f"sigma 5 / composed (pair-steps/s at the medians): {pair_steps['sigma 5'] / med['sigma 5'] / (pair_steps['composed'] / med['composed']):.1f}x")
    ms, chunks = C.c_double(0), C.c_int(0)
    for leg in calls:
        if leg == "composed":
            continue
        r.lib.grlx_read_kernel_timing(1, None, None)
        for _ in range(3):
            calls[leg]()
        r.lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks))
        print(f"{leg:9s} device time of the launches: {ms.value / 3:.3f} ms per call ({chunks.value // 3} chunk(s)); {pair_steps[leg] / (ms.value / 3) / 1e3:.3f} M pair-steps/s")
    r.close()


if __name__ == "__main__":
    main()
