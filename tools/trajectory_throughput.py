#!/usr/bin/env python3
"""trajectory_throughput.py [replicas [starts-per-side [trials [composed-replicas [max-steps]]]]] -- what keeping every step of a greedy
evaluation costs, on pendulum SARSA replicas after `trials` trials from a grid of start states at time 0 (4096 replicas x 16 x 16 starts,
100 trials, max_steps 100 by default: 1 M episodes, about 9 GB of records), in one process on one context:
(a) grlx_evaluate_trajectory against grlx_evaluate(max_steps): seconds per call, host arrays in and out, alternating, median of five;
(b) the same two with the kernels timed alone: events around the launches of every chunk (grlx_read_kernel_timing; a trajectory chunk is
    the zero fill of its records and trajectory_q_kernel<pendulum, 3>), summed over a call's chunks, median of five; once under the
    default staging bound and once under a bound that holds the whole call in one chunk;
(c) `composed-replicas` (8) replicas x the same starts against the path composed from grlx_query_q and grlx_env_step per control step,
    which is the other way to get an episode's steps; the composed path's per-step values must equal the records bit for bit.
Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import capi, runner


def composed(r, cfg, states, actions, n_rep, max_steps, words):
    """the records, and evaluate's sums, from one grlx_query_q per replica and one grlx_env_step over all pairs per control step"""
    n = states.shape[0]
    x = np.tile(states, (n_rep, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    pairs = x.shape[0]
    records = np.zeros((pairs, max_steps, words))
    ret, steps = np.zeros(pairs), np.zeros(pairs, np.int32)
    active = np.ones(pairs, bool)
    for t in range(max_steps):
        if not active.any():
            break
        value, greedy, n_max = np.zeros(pairs), np.zeros(pairs, np.int64), np.zeros(pairs, np.int64)
        for k in range(n_rep):
            _, vk, gk, mk = r.query_q(obs[k * n:(k + 1) * n], replicas=(k, 1))
            value[k * n:(k + 1) * n], greedy[k * n:(k + 1) * n], n_max[k * n:(k + 1) * n] = vk[0], gk[0], mk[0]
        nx, nobs, rew, term = runner.env_step(cfg, x, actions[greedy])
        rec = np.concatenate([np.stack([actions[greedy], rew, value, greedy.astype(np.float64), n_max.astype(np.float64), term.astype(np.float64)], axis=1),
                              obs, nx], axis=1)
        records[active, t] = rec[active]
        ret = np.where(active, ret + rew, ret)
        steps += active
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    return records.reshape(n_rep, n, max_steps, words), ret.reshape(n_rep, n), steps.reshape(n_rep, n)


def median(v):
    return sorted(v)[len(v) // 2]


def kernel_ms(lib, call):
    """(milliseconds of the call's kernels by events, chunks)"""
    ms, chunks = C.c_double(0), C.c_int(0)
    capi.check(lib.grlx_read_kernel_timing(1, None, None))
    call()
    capi.check(lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks)))
    return ms.value, chunks.value


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    n_rep = min(args[3] if len(args) > 3 else 8, n)
    max_steps = args[4] if len(args) > 4 else 100
    runs = 5
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    lib = r.lib
    r.run(trials); r.sync()
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.ascontiguousarray(np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1))    # time 0: full episodes
    ns = states.shape[0]
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    words = r.trajectory_record_words()

    # the timed calls write into arrays allocated once: the first touch of 9 GB of host pages is not what is measured
    P = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
    ret, disc, fin = np.zeros((n, ns)), np.zeros((n, ns)), np.zeros((n, ns, 3))
    steps, term, ties = np.zeros((n, ns), np.int32), np.zeros((n, ns), np.int32), np.zeros((n, ns), np.int32)
    records = np.zeros((n, ns, max_steps, words))
    sums = lambda: (P(ret), P(disc), P(steps, C.c_int32), P(term, C.c_int32), P(ties, C.c_int32), P(fin))
    legs = {"evaluate": lambda: capi.check(lib.grlx_evaluate(r._ctx, 0, n, P(states), ns, max_steps, *sums())),
            "trajectory": lambda: capi.check(lib.grlx_evaluate_trajectory(r._ctx, 0, n, P(states), ns, max_steps, *sums(), P(records)))}
    print(f"{n} replicas x {ns} starts, max_steps {max_steps}, record of {words} doubles: {records.nbytes / 1e9:.3f} GB of records per call", flush=True)
    for leg in legs:                                                         # warm-up at the timed shape
        legs[leg]()
    pair_steps = int(steps.sum())
    want = (ret.copy(), steps.copy())
    assert 1 <= steps.min() and steps.max() <= max_steps

    # (a) seconds per call
    wall = {leg: [] for leg in legs}
    for i in range(runs):
        for leg in legs:
            t0 = time.perf_counter()
            legs[leg]()
            wall[leg].append(time.perf_counter() - t0)
            print(f"(a) run {i}  {leg:10s} {wall[leg][-1]:9.4f} s/call", flush=True)
    for leg in legs:
        m = median(wall[leg])
        print(f"(a) {leg:10s} median {m:.4f} s/call  {pair_steps / m / 1e6:9.3f} M pair-steps/s  min {min(wall[leg]):.4f}  max {max(wall[leg]):.4f}"
              + (f"  {records.nbytes / m / 1e9:.2f} GB/s of records to the host" if leg == "trajectory" else ""), flush=True)
    print(f"(a) trajectory / evaluate (s/call at the medians): {median(wall['trajectory']) / median(wall['evaluate']):.1f}x", flush=True)

    # (b) the kernels alone
    pair_sums = lambda: records.view(np.uint64).reshape(n * ns, -1).sum(axis=1, dtype=np.uint64)       # one word sum per episode
    chunked_sums = pair_sums()                                               # of the calls above: chunks of a few start states, small offsets
    for bound, name in ((0, "default staging bound"), (records.nbytes + (1 << 30), "one chunk")):
        capi.check(lib.grlx_set_query_chunk_bytes(bound))
        dev = {leg: [] for leg in legs}
        chunks = {}
        for i in range(runs):
            for leg in legs:
                ms, chunks[leg] = kernel_ms(lib, legs[leg])
                dev[leg].append(ms)
        capi.check(lib.grlx_set_query_chunk_bytes(0))
        for leg in legs:
            m = median(dev[leg])
            print(f"(b) {name}: {leg:10s} kernels median {m:9.3f} ms in {chunks[leg]} chunk(s)  {pair_steps / m / 1e6:9.3f} G pair-steps/s"
                  f"  min {min(dev[leg]):.3f}  max {max(dev[leg]):.3f}", flush=True)
        extra = median(dev["trajectory"]) - median(dev["evaluate"])
        written = pair_steps * words * 8
        print(f"(b) {name}: trajectory - evaluate = {extra:.3f} ms for {written / 1e9:.3f} GB of records written and {records.nbytes / 1e9:.3f} GB zero-filled"
              f" ({written / extra / 1e6:.1f} GB/s over the records written; ratio {median(dev['trajectory']) / median(dev['evaluate']):.2f}x)", flush=True)
    assert ret.tobytes() == want[0].tobytes() and steps.tobytes() == want[1].tobytes()
    # the last call was one chunk: record offsets up to the whole array's size on the device, against the chunked calls' words
    assert np.array_equal(pair_sums(), chunked_sums), "the one-chunk call's records differ from the chunked call's"
    taken = (np.arange(max_steps) < steps[:, :, None])
    assert not records[~taken].any() and np.array_equal(records[..., -3:][np.arange(n)[:, None], np.arange(ns)[None, :], steps - 1], fin)
    print(f"(b) the records of the one-chunk call equal the chunked call's (a word sum per episode, {n * ns} episodes); zeros behind every end; last state = final_state", flush=True)

    # (c) against the composed path, on the first n_rep replicas
    fused = r.evaluate_trajectory(states, max_steps, replicas=(0, n_rep))
    comp = composed(r, cfg, states, actions, n_rep, max_steps, words)
    assert fused.records.tobytes() == comp[0].tobytes(), "the composed path's per-step values differ from the records"
    assert fused.records.tobytes() == records[:n_rep].tobytes() and fused.ret.tobytes() == comp[1].tobytes() and (fused.steps == comp[2]).all()
    print(f"(c) the composed path's per-step values equal the records bit for bit ({int(fused.steps.sum())} records of {n_rep} replicas)", flush=True)
    res = {"trajectory": [], "composed": []}
    small = int(fused.steps.sum())
    for i in range(runs):
        for leg in res:
            t0 = time.perf_counter()
            if leg == "trajectory":
                r.evaluate_trajectory(states, max_steps, replicas=(0, n_rep))
            else:
                composed(r, cfg, states, actions, n_rep, max_steps, words)
            res[leg].append(time.perf_counter() - t0)
    for leg in res:
        m = median(res[leg])
        print(f"(c) {n_rep} replicas x {ns} starts  {leg:10s} median {m:.4f} s/call  {small / m / 1e6:9.3f} M pair-steps/s  min {min(res[leg]):.4f}  max {max(res[leg]):.4f}", flush=True)
    print(f"(c) trajectory / composed (pair-steps/s at the medians): {median(res['composed']) / median(res['trajectory']):.1f}x")
    r.close()


if __name__ == "__main__":
    main()
