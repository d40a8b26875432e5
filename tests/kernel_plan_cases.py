"""Which kernel runs: one table of cases shared by tests/test_kernel_plan.py (grlx_kernel_plan, no device),
tests/test_gpu_kernel_plan.py (what a context launches) and tests/test_gpu_kernel_plan_parity.py (what that launch computes, against the
oracle built from the same case: build_pair).  The expected values are literals: they state what the launch ladders chose
before the kernel table replaced them (profiles/kernel_plan_ab.md has the kernel traces of both builds).

A case: (id, builder, n_replicas, config overrides, flags, simds, gpu, (replicas per wave, rollout row, server row, variant)).
  flags  the PLAN_* bits of grlx_kernel_plan; on the GPU: grlx_set_diag, grlx_set_replica_params, GRLX_ENV_SERVER, GRLX_ENV_SERVER_WALKER
  simds  the device size the plan is asked for (1: the automatic layout's thresholds at tiny sizes)
  gpu    the case is also launched (layout forced through the config, at most 37 replicas, the runtime's own answer to "fits")
"""
from grl_amd import capi

GENERIC, SPECIALISED, IN_PLACE = 1, 2, 3
STAMPS1, STAMPS2, SWEEP, OFF, WALKER, FITS, NOFIT = (capi.PLAN_STAMPS_IN_PLACE, capi.PLAN_STAMPS_DEFERRED, capi.PLAN_SWEEP, capi.PLAN_SERVER_OFF,
                                                     capi.PLAN_WALKER_SERVER, capi.PLAN_FITS_YES, capi.PLAN_FITS_NO)
TAPS = dict(tap_replica=0, tap_capacity=64)
TAPDEF = dict(tap_replica=0, tap_capacity=64, tap_deferred=1)
SARSA, Q, ES, ADV = capi.AGENT_SARSA, capi.AGENT_Q, capi.AGENT_EXPECTED_SARSA, capi.AGENT_ADVANTAGE


BUILDERS = {"pendulum": "pendulum", "acrobot": "acrobot", "walker": "compass_walker", "cart_pole_q": "cart_pole_q", "cart_pole_ac": "cart_pole_ac",
            "pendulum_ac": "pendulum_ac", "pendulum_qv": "pendulum_qv", "acrobot_qv": "acrobot_qv"}      # case builder -> tests/configs.py
# Every override key of a case is in exactly one of these lists; build_pair refuses any other, so a case cannot run against an oracle
# that silently lacks one of its overrides.
RESULT_KEYS = ["agent", "alpha", "gamma", "epsilon", "timeout", "sigma", "kappa", "trace", "action_steps", "target_interval", "target_tau",
               "safe"]                                        # they change results: the oracle's spec gets them too
KERNEL_KEYS = ["replicas_per_wave", "force_generic", "wave_limit", "tap_replica", "tap_capacity", "tap_deferred",
               "table_log2_capacity"]                         # they only choose a kernel or size its buffers: the spec never sees them


def build_pair(grlx, builder, n, over):
    """(grlx_config, oracle spec) of a case, the overrides applied to both halves (`safe` is the projector's in the config).
    grlx = None: the oracle half only (a cart-pole spec then has the task's penalties off instead of its config's: tests/configs.py)."""
    from tests import configs
    unknown = [k for k in over if k not in RESULT_KEYS and k not in KERNEL_KEYS]
    if unknown:
        raise KeyError(f"override keys {unknown} are neither in RESULT_KEYS nor in KERNEL_KEYS (tests/kernel_plan_cases.py)")
    over = dict(over)
    safe = over.pop("safe", 0)
    cfg, spec = getattr(configs, BUILDERS[builder])(grlx, n, **over)
    if cfg is not None:
        cfg.projector.safe = safe
    spec.safe = safe
    for k in RESULT_KEYS:
        if k in over:
            setattr(spec, k, over[k])
    return cfg, spec


def build(grlx, builder, n, over):
    """The grlx_config of a case."""
    return build_pair(grlx, builder, n, over)[0]


def open_runner(grlx, monkeypatch, case, cfg):
    """What a launched case does before its first run: the environment-server switches of its flags, the context with seeds 1..n, the
    per-replica alphas of a sweep case, the stamps of a stamped one.  Returns (runner, alpha of every replica or None)."""
    import numpy as np
    n, flags = case[2], case[4]
    monkeypatch.setenv("GRLX_ENV_SERVER", "0" if flags & OFF else "1")
    monkeypatch.setenv("GRLX_ENV_SERVER_WALKER", "1" if flags & WALKER else "0")
    r = grlx.Runner(cfg, np.arange(1, n + 1))
    alphas = None
    try:
        if flags & SWEEP:
            alphas = [0.1 + 0.01 * k for k in range(n)]
            r.set_replica_params(alpha=alphas)
        if flags & (STAMPS1 | STAMPS2):
            r.set_diag(2 if flags & STAMPS2 else 1)
    except Exception:
        r.close()
        raise
    return r, alphas


CASES = [
    # ---- the pendulum: served pair -> specialised 4 -> generic 4, from both sides of every step
    ("pend-sarsa-served", "pendulum", 5, dict(replicas_per_wave=4), 0, 1024, True,
     (4, "rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_SARSA>>", SPECIALISED)),
    ("pend-q-served", "pendulum", 5, dict(replicas_per_wave=4, agent=Q), 0, 1024, True,
     (4, "rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_Q>>", "env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_Q>>", SPECIALISED)),
    ("pend-es-served", "pendulum", 5, dict(replicas_per_wave=4, agent=ES), 0, 1024, True,
     (4, "rollout_served_kernel<3, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>", "env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>", SPECIALISED)),
    ("pend-served-force-generic", "pendulum", 5, dict(replicas_per_wave=4, force_generic=1), 0, 1024, True,
     (4, "rollout_served_kernel<3, SpecNone>", "env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecNone>", GENERIC)),
    ("pend-served-alpha-perturbed", "pendulum", 5, dict(replicas_per_wave=4, alpha=0.25), 0, 1024, True,
     (4, "rollout_served_kernel<3, SpecNone>", "env_server_kernel<GRLX_ENV_PENDULUM, 3, SpecNone>", GENERIC)),
    ("pend-sarsa-unserved", "pendulum", 5, dict(replicas_per_wave=4), OFF, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("pend-q-unserved", "pendulum", 5, dict(replicas_per_wave=4, agent=Q), OFF, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_Q>>", "", SPECIALISED)),
    ("pend-es-unserved", "pendulum", 5, dict(replicas_per_wave=4, agent=ES), OFF, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_EXPECTED_SARSA>>", "", SPECIALISED)),
    ("pend-unserved-force-generic", "pendulum", 5, dict(replicas_per_wave=4, force_generic=1), OFF, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecNone>", "", GENERIC)),
    ("pend-unserved-timeout-perturbed", "pendulum", 5, dict(replicas_per_wave=4, timeout=2.5), OFF, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecNone>", "", GENERIC)),
    ("pend5-4", "pendulum", 5, dict(replicas_per_wave=4, action_steps=5), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 5, false, SpecNone>", "", GENERIC)),
    ("pend5-8", "pendulum", 9, dict(replicas_per_wave=8, action_steps=5), 0, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 5, 2, SpecNone>", "", GENERIC)),
    ("pend-sarsa-8", "pendulum", 9, dict(replicas_per_wave=8), 0, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("pend-q-8", "pendulum", 9, dict(replicas_per_wave=8, agent=Q), 0, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_Q>>", "", SPECIALISED)),
    ("pend-es-8-has-no-specialised", "pendulum", 9, dict(replicas_per_wave=8, agent=ES), 0, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecNone>", "", GENERIC)),
    ("pend-8-force-generic", "pendulum", 9, dict(replicas_per_wave=8, force_generic=1), 0, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecNone>", "", GENERIC)),
    # ---- records: stamped deferred -> tapped deferred -> in place; taps always run four replicas per wave
    ("pend-taps", "pendulum", 5, dict(replicas_per_wave=8, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("pend-tapdef", "pendulum", 5, dict(replicas_per_wave=4, **TAPDEF), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecNone, true, false, true>", "", GENERIC)),
    ("pend5-tapdef", "pendulum", 5, dict(replicas_per_wave=4, action_steps=5, **TAPDEF), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 5, false, SpecNone, true, false, true>", "", GENERIC)),
    ("acrobot-tapdef", "acrobot", 5, dict(replicas_per_wave=4, **TAPDEF), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecNone, true, false, true>", "", GENERIC)),
    ("pend5-taps", "pendulum", 5, dict(replicas_per_wave=4, action_steps=5, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 5, true, SpecNone>", "", IN_PLACE)),
    ("pend-stamps-in-place", "pendulum", 5, dict(replicas_per_wave=4), STAMPS1, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("pend-stamps-in-place-layout-8", "pendulum", 9, dict(replicas_per_wave=8), STAMPS1, 1024, True,
     (8, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("pend-stamps-deferred", "pendulum", 5, dict(replicas_per_wave=4), STAMPS2, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone, true>", "", GENERIC)),
    ("pend-stamps-deferred-with-taps-falls-through", "pendulum", 5, dict(replicas_per_wave=4, **TAPS), STAMPS2, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("acrobot-stamps-deferred-falls-through", "acrobot", 5, dict(replicas_per_wave=4), STAMPS2, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone>", "", IN_PLACE)),
    ("acrobot-taps", "acrobot", 5, dict(replicas_per_wave=4, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone>", "", IN_PLACE)),
    ("cart-pole-q-taps", "cart_pole_q", 5, dict(replicas_per_wave=4, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_CART_POLE, 3, true, SpecNone>", "", IN_PLACE)),
    ("walker-taps", "walker", 5, dict(replicas_per_wave=4, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, true, SpecNone>", "", IN_PLACE)),
    # ---- advantage learning: its own rows, after the stamped deferred one
    ("pend-advantage", "pendulum", 5, dict(replicas_per_wave=4, agent=ADV, kappa=0.5), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone, false, true>", "", IN_PLACE)),
    ("acrobot-advantage", "acrobot", 5, dict(replicas_per_wave=4, agent=ADV, kappa=0.5), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone, false, true>", "", IN_PLACE)),
    ("pend-advantage-taps", "pendulum", 5, dict(replicas_per_wave=4, agent=ADV, kappa=0.5, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone, false, true>", "", IN_PLACE)),
    # ---- sweep rows: a sweep context, and a TD context without a trace
    ("pend-sweep-4", "pendulum", 5, dict(replicas_per_wave=4), SWEEP, 1024, True, (4, "rollout_sweep_kernel<GRLX_ENV_PENDULUM, 3>", "", GENERIC)),
    ("pend-sweep-8", "pendulum", 9, dict(replicas_per_wave=8), SWEEP, 1024, True, (8, "rollout_wide_sweep_kernel<GRLX_ENV_PENDULUM, 3>", "", GENERIC)),
    ("pend5-sweep-4", "pendulum", 5, dict(replicas_per_wave=4, action_steps=5), SWEEP, 1024, True, (4, "rollout_sweep_kernel<GRLX_ENV_PENDULUM, 5>", "", GENERIC)),
    ("pend5-sweep-8", "pendulum", 9, dict(replicas_per_wave=8, action_steps=5), SWEEP, 1024, True, (8, "rollout_wide_sweep_kernel<GRLX_ENV_PENDULUM, 5>", "", GENERIC)),
    ("acrobot-sweep-4", "acrobot", 5, dict(replicas_per_wave=4), SWEEP, 1024, True, (4, "rollout_sweep_kernel<GRLX_ENV_ACROBOT, 3>", "", GENERIC)),
    ("acrobot-sweep-8", "acrobot", 9, dict(replicas_per_wave=8), SWEEP, 1024, True, (8, "rollout_wide_sweep_kernel<GRLX_ENV_ACROBOT, 3>", "", GENERIC)),
    ("cart-pole-q-sweep-4", "cart_pole_q", 5, dict(replicas_per_wave=4), SWEEP, 1024, True, (4, "rollout_sweep_kernel<GRLX_ENV_CART_POLE, 3>", "", GENERIC)),
    ("cart-pole-q-sweep-8", "cart_pole_q", 9, dict(replicas_per_wave=8), SWEEP, 1024, True, (8, "rollout_wide_sweep_kernel<GRLX_ENV_CART_POLE, 3>", "", GENERIC)),
    ("walker-sweep-4", "walker", 5, dict(replicas_per_wave=4), SWEEP, 1024, True, (4, "rollout_sweep_kernel<GRLX_ENV_COMPASS_WALKER, 3>", "", GENERIC)),
    ("walker-sweep-8", "walker", 9, dict(replicas_per_wave=8), SWEEP, 1024, True, (8, "rollout_wide_sweep_kernel<GRLX_ENV_COMPASS_WALKER, 3>", "", GENERIC)),
    ("pend-no-trace-runs-sweep-row", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_NONE), 0, 1024, True,
     (4, "rollout_sweep_kernel<GRLX_ENV_PENDULUM, 3>", "", GENERIC)),
    ("pend-no-trace-taps-in-place", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_NONE, **TAPS), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("acrobot-no-trace-16-capped-to-8", "acrobot", 17, dict(replicas_per_wave=16, trace=capi.TRACE_NONE), 0, 1024, True,
     (8, "rollout_wide_sweep_kernel<GRLX_ENV_ACROBOT, 3>", "", GENERIC)),
    ("walker-sweep-32-falls-to-8", "walker", 33, dict(replicas_per_wave=0), SWEEP, 1, False, (8, "rollout_wide_sweep_kernel<GRLX_ENV_COMPASS_WALKER, 3>", "", GENERIC)),
    # ---- the acrobot: wide served -> 16 -> 8 -> specialised 4 -> generic 4
    ("acrobot-4", "acrobot", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecAcrobotQ>", "", SPECIALISED)),
    ("acrobot-4-force-generic", "acrobot", 5, dict(replicas_per_wave=4, force_generic=1), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecNone>", "", GENERIC)),
    ("acrobot-4-sarsa-is-not-the-q-constants", "acrobot", 5, dict(replicas_per_wave=4, agent=SARSA), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, false, SpecNone>", "", GENERIC)),
    ("acrobot-8-served", "acrobot", 9, dict(replicas_per_wave=8), FITS, 1024, True,
     (8, "rollout_wide_served_kernel<GRLX_ENV_ACROBOT, SpecAcrobotQ>", "env_server_acrobot_pinned_kernel<SpecAcrobotQ>", SPECIALISED)),
    ("acrobot-8-served-force-generic", "acrobot", 9, dict(replicas_per_wave=8, force_generic=1), FITS, 1024, True,
     (8, "rollout_wide_served_kernel<GRLX_ENV_ACROBOT, SpecNone>", "env_server_acrobot_kernel<SpecNone>", GENERIC)),
    ("acrobot-8-served-gamma-perturbed", "acrobot", 9, dict(replicas_per_wave=8, gamma=0.96), FITS, 1024, True,
     (8, "rollout_wide_served_kernel<GRLX_ENV_ACROBOT, SpecNone>", "env_server_acrobot_kernel<SpecNone>", GENERIC)),
    ("acrobot-8-does-not-fit", "acrobot", 9, dict(replicas_per_wave=8), NOFIT, 1024, False,
     (8, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecAcrobotQ>", "", SPECIALISED)),
    ("acrobot-8-server-off", "acrobot", 9, dict(replicas_per_wave=8), OFF | FITS, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecAcrobotQ>", "", SPECIALISED)),
    ("acrobot-8-server-off-force-generic", "acrobot", 9, dict(replicas_per_wave=8, force_generic=1), OFF, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecNone>", "", GENERIC)),
    ("acrobot-16", "acrobot", 17, dict(replicas_per_wave=16), FITS, 1024, True, (16, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecAcrobotQ>", "", SPECIALISED)),
    ("acrobot-16-force-generic", "acrobot", 17, dict(replicas_per_wave=16, force_generic=1), FITS, 1024, True,
     (16, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecNone>", "", GENERIC)),
    # ---- the compass walker: its server is opt-in; 32 -> 16 -> 8 -> 4
    ("walker-4", "walker", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-4-force-generic", "walker", 5, dict(replicas_per_wave=4, force_generic=1), 0, 1024, True,
     (4, "rollout_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, SpecNone>", "", GENERIC)),
    ("walker-8-server-not-opted-in", "walker", 9, dict(replicas_per_wave=8), FITS, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-8-force-generic", "walker", 9, dict(replicas_per_wave=8, force_generic=1), FITS, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecNone>", "", GENERIC)),
    ("walker-8-served", "walker", 9, dict(replicas_per_wave=8), WALKER | FITS, 1024, True,
     (8, "rollout_wide_served_kernel<GRLX_ENV_COMPASS_WALKER, SpecWalkerQ>", "env_server_walker_kernel<SpecWalkerQ>", SPECIALISED)),
    # (the generic walker pair needs 384 + 160 registers: on the device it does not fit and runs unserved)
    ("walker-8-served-gamma-perturbed", "walker", 9, dict(replicas_per_wave=8, gamma=0.96), WALKER | FITS, 1024, False,
     (8, "rollout_wide_served_kernel<GRLX_ENV_COMPASS_WALKER, SpecNone>", "env_server_walker_kernel<SpecNone>", GENERIC)),
    ("walker-8-opted-in-generic-does-not-fit", "walker", 9, dict(replicas_per_wave=8, gamma=0.96), WALKER | NOFIT, 1024, False,
     (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecNone>", "", GENERIC)),
    ("walker-8-opted-in-does-not-fit", "walker", 9, dict(replicas_per_wave=8), WALKER | NOFIT, 1024, False,
     (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-8-opted-in-server-off", "walker", 9, dict(replicas_per_wave=8), WALKER | FITS | OFF, 1024, True,
     (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-16", "walker", 17, dict(replicas_per_wave=16), WALKER | FITS, 1024, True, (16, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-16-force-generic", "walker", 17, dict(replicas_per_wave=16, force_generic=1), 0, 1024, True,
     (16, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecNone>", "", GENERIC)),
    ("walker-32", "walker", 37, dict(replicas_per_wave=32), 0, 1024, True, (32, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 8, SpecWalkerQ>", "", SPECIALISED)),
    ("walker-32-force-generic", "walker", 37, dict(replicas_per_wave=32, force_generic=1), 0, 1024, True,
     (32, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 8, SpecNone>", "", GENERIC)),
    # ---- the discretised cart-pole: generic rows only
    ("cart-pole-q-4", "cart_pole_q", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_kernel<GRLX_ENV_CART_POLE, 3, false, SpecNone>", "", GENERIC)),
    ("cart-pole-q-8", "cart_pole_q", 9, dict(replicas_per_wave=8), 0, 1024, True, (8, "rollout_wide_kernel<GRLX_ENV_CART_POLE, 3, 2, SpecNone>", "", GENERIC)),
    # ---- actor-critic
    ("ac-4", "cart_pole_ac", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecCartPoleAc, true>", "", SPECIALISED)),
    ("ac-4-force-generic", "cart_pole_ac", 5, dict(replicas_per_wave=4, force_generic=1), 0, 1024, True,
     (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, true>", "", GENERIC)),
    ("ac-4-sigma-perturbed", "cart_pole_ac", 5, dict(replicas_per_wave=4, sigma=4.0), 0, 1024, True,
     (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, true>", "", GENERIC)),
    ("ac-taps", "cart_pole_ac", 9, dict(replicas_per_wave=8, **TAPS), 0, 1024, True, (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, false>", "", IN_PLACE)),
    ("ac-no-trace-in-place", "cart_pole_ac", 17, dict(replicas_per_wave=16, trace=capi.TRACE_NONE), 0, 1024, True,
     (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, false>", "", IN_PLACE)),
    ("ac-8", "cart_pole_ac", 9, dict(replicas_per_wave=8), 0, 1024, True, (8, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecCartPoleAc>", "", SPECIALISED)),
    ("ac-8-force-generic", "cart_pole_ac", 9, dict(replicas_per_wave=8, force_generic=1), 0, 1024, True,
     (8, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecNone>", "", GENERIC)),
    ("ac-12", "cart_pole_ac", 13, dict(replicas_per_wave=12), 0, 1024, True, (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecCartPoleAc>", "", SPECIALISED)),
    ("ac-12-force-generic", "cart_pole_ac", 13, dict(replicas_per_wave=12, force_generic=1), 0, 1024, True,
     (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecNone>", "", GENERIC)),
    ("ac-16", "cart_pole_ac", 17, dict(replicas_per_wave=16), 0, 1024, True, (16, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 4, SpecCartPoleAc>", "", SPECIALISED)),
    ("ac-16-force-generic", "cart_pole_ac", 17, dict(replicas_per_wave=16, force_generic=1), 0, 1024, True,
     (16, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 4, SpecNone>", "", GENERIC)),
    # the 12-slot kernel's waves own at most 64 replicas each: beyond, the 8-slot kernel runs and the context goes on reporting 12
    ("ac-12-one-wave-owns-64", "cart_pole_ac", 64, dict(replicas_per_wave=12, wave_limit=1), 0, 1024, False,
     (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecCartPoleAc>", "", SPECIALISED)),
    ("ac-12-one-wave-cannot-own-65", "cart_pole_ac", 65, dict(replicas_per_wave=12, wave_limit=1), 0, 1024, False,
     (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecCartPoleAc>", "", SPECIALISED)),
    ("pend-ac-4", "pendulum_ac", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_ac_kernel<GRLX_ENV_PENDULUM, SpecNone, true>", "", GENERIC)),
    ("pend-ac-taps", "pendulum_ac", 5, dict(replicas_per_wave=4, **TAPS), 0, 1024, True, (4, "rollout_ac_kernel<GRLX_ENV_PENDULUM, SpecNone, false>", "", IN_PLACE)),
    ("pend-ac-8", "pendulum_ac", 9, dict(replicas_per_wave=8), 0, 1024, True, (8, "rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 2, SpecNone>", "", GENERIC)),
    ("pend-ac-12", "pendulum_ac", 13, dict(replicas_per_wave=12), 0, 1024, True, (12, "rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 3, SpecNone>", "", GENERIC)),
    ("pend-ac-16", "pendulum_ac", 17, dict(replicas_per_wave=16), 0, 1024, True, (16, "rollout_ac_wide_kernel<GRLX_ENV_PENDULUM, 4, SpecNone>", "", GENERIC)),
    # ---- QV, accumulating trace, target network / claim table: four replicas per wave whatever the layout
    ("pend-qv", "pendulum_qv", 5, dict(replicas_per_wave=8), 0, 1024, True, (4, "rollout_qv_kernel<GRLX_ENV_PENDULUM, 3>", "", IN_PLACE)),
    ("acrobot-qv", "acrobot_qv", 5, dict(replicas_per_wave=4), 0, 1024, True, (4, "rollout_qv_kernel<GRLX_ENV_ACROBOT, 3>", "", IN_PLACE)),
    ("pend-acc-sarsa", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING), 0, 1024, True,
     (4, "rollout_acc_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumAcc<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("pend-acc-q", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING, agent=Q), 0, 1024, True,
     (4, "rollout_acc_kernel<GRLX_ENV_PENDULUM, 3, SpecPendulumAcc<GRLX_AGENT_Q>>", "", SPECIALISED)),
    ("pend-acc-es-has-no-specialised", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING, agent=ES), 0, 1024, True,
     (4, "rollout_acc_kernel<GRLX_ENV_PENDULUM, 3>", "", IN_PLACE)),
    ("pend-acc-taps", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING, **TAPS), 0, 1024, True,
     (4, "rollout_acc_kernel<GRLX_ENV_PENDULUM, 3>", "", IN_PLACE)),
    ("pend-acc-epsilon-perturbed", "pendulum", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING, epsilon=0.1), 0, 1024, True,
     (4, "rollout_acc_kernel<GRLX_ENV_PENDULUM, 3>", "", IN_PLACE)),
    ("acrobot-acc", "acrobot", 5, dict(replicas_per_wave=4, trace=capi.TRACE_ACCUMULATING), 0, 1024, True, (4, "rollout_acc_kernel<GRLX_ENV_ACROBOT, 3>", "", IN_PLACE)),
    ("pend-target", "pendulum", 5, dict(replicas_per_wave=4, target_interval=5, target_tau=0.5), 0, 1024, True,
     (4, "rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, true, false>", "", IN_PLACE)),
    ("pend-safe", "pendulum", 5, dict(replicas_per_wave=4, safe=1), 0, 1024, True, (4, "rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, false, true>", "", IN_PLACE)),
    ("pend-target-safe", "pendulum", 5, dict(replicas_per_wave=4, target_interval=5, target_tau=0.5, safe=2), 0, 1024, True,
     (4, "rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, true, true>", "", IN_PLACE)),
    ("acrobot-target", "acrobot", 5, dict(replicas_per_wave=8, target_interval=5, target_tau=0.5), 0, 1024, True,
     (4, "rollout_tgt_kernel<GRLX_ENV_ACROBOT, 3, true, false>", "", IN_PLACE)),
    ("acrobot-safe", "acrobot", 5, dict(replicas_per_wave=4, safe=1), 0, 1024, True, (4, "rollout_tgt_kernel<GRLX_ENV_ACROBOT, 3, false, true>", "", IN_PLACE)),
    ("cart-pole-q-target", "cart_pole_q", 5, dict(replicas_per_wave=4, target_interval=5, target_tau=0.5), 0, 1024, True,
     (4, "rollout_tgt_kernel<GRLX_ENV_CART_POLE, 3, true, false>", "", IN_PLACE)),
    ("cart-pole-q-safe", "cart_pole_q", 5, dict(replicas_per_wave=4, safe=1), 0, 1024, True, (4, "rollout_tgt_kernel<GRLX_ENV_CART_POLE, 3, false, true>", "", IN_PLACE)),
    ("walker-target", "walker", 5, dict(replicas_per_wave=4, target_interval=5, target_tau=0.5), 0, 1024, True,
     (4, "rollout_tgt_kernel<GRLX_ENV_COMPASS_WALKER, 3, true, false>", "", IN_PLACE)),
    ("walker-safe", "walker", 5, dict(replicas_per_wave=4, safe=1), 0, 1024, True, (4, "rollout_tgt_kernel<GRLX_ENV_COMPASS_WALKER, 3, false, true>", "", IN_PLACE)),
    # ---- the automatic layout (replicas_per_wave = 0) at its thresholds, on a device of ONE SIMD
    ("auto-4-replicas-one-wave", "pendulum", 4, dict(), OFF, 1, False, (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, false, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("auto-5-replicas-step-to-8", "pendulum", 5, dict(), OFF, 1, False, (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("auto-5-replicas-taps-stay-4", "pendulum", 5, dict(**TAPS), OFF, 1, False, (4, "rollout_kernel<GRLX_ENV_PENDULUM, 3, true, SpecNone>", "", IN_PLACE)),
    ("auto-ac-8", "cart_pole_ac", 8, dict(), 0, 1, False, (8, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecCartPoleAc>", "", SPECIALISED)),
    ("auto-ac-9", "cart_pole_ac", 9, dict(), 0, 1, False, (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecCartPoleAc>", "", SPECIALISED)),
    ("auto-ac-14", "cart_pole_ac", 14, dict(), 0, 1, False, (12, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 3, SpecCartPoleAc>", "", SPECIALISED)),
    ("auto-ac-15", "cart_pole_ac", 15, dict(), 0, 1, False, (16, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 4, SpecCartPoleAc>", "", SPECIALISED)),
    ("auto-ac-15-wave-limit-set-stays-8", "cart_pole_ac", 15, dict(wave_limit=1), 0, 1, False, (8, "rollout_ac_wide_kernel<GRLX_ENV_CART_POLE, 2, SpecCartPoleAc>", "", SPECIALISED)),
    ("auto-ac-15-no-trace-capped-to-4", "cart_pole_ac", 15, dict(trace=capi.TRACE_NONE), 0, 1, False, (4, "rollout_ac_kernel<GRLX_ENV_CART_POLE, SpecNone, false>", "", IN_PLACE)),
    ("auto-acrobot-14", "acrobot", 14, dict(), OFF, 1, False, (8, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 2, SpecAcrobotQ>", "", SPECIALISED)),
    ("auto-acrobot-15", "acrobot", 15, dict(), OFF, 1, False, (16, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecAcrobotQ>", "", SPECIALISED)),
    ("auto-acrobot-30-has-no-32", "acrobot", 30, dict(), OFF, 1, False, (16, "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecAcrobotQ>", "", SPECIALISED)),
    ("auto-acrobot-15-no-trace-capped-to-8", "acrobot", 15, dict(trace=capi.TRACE_NONE), OFF, 1, False, (8, "rollout_wide_sweep_kernel<GRLX_ENV_ACROBOT, 3>", "", GENERIC)),
    ("auto-acrobot-15-taps-stay-4", "acrobot", 15, dict(**TAPS), OFF, 1, False, (4, "rollout_kernel<GRLX_ENV_ACROBOT, 3, true, SpecNone>", "", IN_PLACE)),
    ("auto-pendulum-15-stays-8", "pendulum", 15, dict(), OFF, 1, False, (8, "rollout_wide_kernel<GRLX_ENV_PENDULUM, 3, 2, SpecPendulumTcA<GRLX_AGENT_SARSA>>", "", SPECIALISED)),
    ("auto-walker-14", "walker", 14, dict(), OFF, 1, False, (8, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 2, SpecWalkerQ>", "", SPECIALISED)),
    ("auto-walker-15", "walker", 15, dict(), OFF, 1, False, (16, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecWalkerQ>", "", SPECIALISED)),
    ("auto-walker-29", "walker", 29, dict(), OFF, 1, False, (16, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 4, SpecWalkerQ>", "", SPECIALISED)),
    ("auto-walker-30", "walker", 30, dict(), OFF, 1, False, (32, "rollout_wide_kernel<GRLX_ENV_COMPASS_WALKER, 3, 8, SpecWalkerQ>", "", SPECIALISED)),
    ("auto-target-network-stays-4", "pendulum", 30, dict(target_interval=5, target_tau=0.5), OFF, 1, False, (4, "rollout_tgt_kernel<GRLX_ENV_PENDULUM, 3, true, false>", "", IN_PLACE)),
]

# the cases a device launches: tests/test_gpu_kernel_plan.py (which row ran) and tests/test_gpu_kernel_plan_parity.py (with the oracle's bits)
LAUNCHED = [c for c in CASES if c[6]]

# the grid of the two 12-slot cases (one wave each) is asserted too
GRIDS = {"ac-12-one-wave-owns-64": 1, "ac-12-one-wave-cannot-own-65": 1, "ac-12": 2, "pend-sarsa-served": 2, "walker-32": 2, "acrobot-8-served": 2}
