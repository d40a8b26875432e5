#!/usr/bin/env python3
"""Where the cycles of the environment server go (stats build: GRLX_EXTRA_FLAGS=-DGRLX_ENV_SERVER_STATS, library named by GRLX_LIB;
run with GRLX_ENV_SERVER=1): env_server_stats.py [replicas] [trials <= 32, one launch] [warm-up launches, default 1]
The stamped launch is the one after the warm-up launches: with 11 trials and 5 warm-up launches it covers trials 56-66, the regime
bench.py times (few slot creations); with one warm-up launch most passes still create a slot somewhere in the wave."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import capi
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
trials = int(sys.argv[2]) if len(sys.argv) > 2 else 32
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 1
cfg = grl_amd.pendulum_sarsa_config(n)
r = grl_amd.Runner(cfg, np.arange(1, n + 1))
for _ in range(warm):
    r.run(trials); r.sync()      # warm tables
l0, t0 = r.step_counts()
r.run(trials); r.sync()
l1, t1 = r.step_counts()
lib = r.lib
lib.grlx_env_server_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
mail = np.zeros((n, 128), dtype=np.uint64)
capi.check(lib.grlx_env_server_debug(r._ctx, mail.ctypes.data_as(C.c_void_p), mail.nbytes))
st = mail[:, 16:32].astype(np.float64)
steps = (l1 - l0) + (t1 - t0)
print(f"{n} replicas, {trials} trials after {warm} warm-up launch(es): {steps} env-steps, {steps / n:.0f} per replica")
print(f"server : kernel {st[:,0].mean():.0f} cycles, busy (command seen -> candidates stored) {st[:,1].mean():.0f} = {st[:,1].sum()/st[:,0].sum():.2f}, "
      f"{st[:,2].mean():.0f} commands, {st[:,1].sum()/max(st[:,2].sum(),1):.0f} cycles per command, {st[:,3].mean():.0f} idle polls, "
      f"{st[:,10].mean():.0f} batches of which {st[:,9].mean():.0f} without all four replicas of the wave")
print(f"rollout: kernel {st[:,4].mean():.0f} cycles, waiting for candidates {st[:,5].mean():.0f} = {st[:,5].sum()/st[:,4].sum():.2f}, "
      f"{st[:,6].mean():.0f} fetches, {st[:,5].sum()/max(st[:,6].sum(),1):.0f} cycles per fetch, {st[:,7].sum()/max(st[:,6].sum(),1):.2f} extra polls per fetch, "
      f"{int(st[:,8].sum())} of {n} replicas still served at the end")
print(f"cycles per pass (rollout kernel / fetches): {st[:,4].sum()/max(st[:,6].sum(),1):.0f}   (s_memtime ticks = shader cycles)")
ph = mail[:, 112:120].astype(np.float64)      # EnvMail::pad1[0..7], byte 896: the rollout wave's stamps
# (the loop of the specialised kernels is rotated, SPEC::kEarlyTake: there "taking the server's answer" is the vote at the sampler, the
#  command and, after the tail, the handing round; the load of the fifteen units is issued under "inserts + LDS writes"; the bucket loads
#  are issued at the top of a pass, straight after the previous pass's tail, and waited for under "table lookup")
names = ["loop/bookkeeping (held eviction)", "environment step: taking the server's answer (vote, command, handing round)", "tile hashing",
         "inserts + LDS writes (+ load of the 15 candidate units)", "LDS sums + sampler", "TD update + trace (+ target)", "wait for previous stores",
         "table lookup (loads)"]
tot = ph.sum()
if tot > 0:
    print("rollout wave, share of the stamped cycles per phase (%.0f cycles per pass):" % (tot / max(st[:, 6].sum(), 1)))
    for k, nm in enumerate(names):
        print(f"  {nm:80s} {ph[:, k].sum() / tot:6.3f}   {ph[:, k].sum() / max(st[:, 6].sum(), 1):8.0f} cycles per pass")
r.close()
