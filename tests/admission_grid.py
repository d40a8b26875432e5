"""What grlx_create says to a grid of configurations: the (code, message) of every refusal, GRLX_ERR_NO_DEVICE for what it admits.

The listing of tests/data/kernel_admission.txt was written by this module against the build BEFORE the admission checks moved to the kernel
table (`GRLX_LIB=<that libgrlx.so> python -m tests.admission_grid > tests/data/kernel_admission.txt`, on a box without a GPU);
tests/test_kernel_admission.py compares the current library with it line by line.  Messages are numbered in order of first appearance
(the `M<k> <code> <message>` lines at the top); a grid line holds the message numbers of one (environment, agent, trace)."""
import ctypes as C
import itertools

from grl_amd import capi

ENVS = (capi.ENV_PENDULUM, capi.ENV_CART_POLE, capi.ENV_ACROBOT, capi.ENV_COMPASS_WALKER, capi.ENV_CART_POLE_BALANCING, capi.ENV_EXTERNAL)
AGENTS = (capi.AGENT_SARSA, capi.AGENT_Q, capi.AGENT_AC, capi.AGENT_EXPECTED_SARSA, capi.AGENT_ADVANTAGE, capi.AGENT_QV)
TRACES = (capi.TRACE_NONE, capi.TRACE_REPLACING, capi.TRACE_ACCUMULATING)
ACTIONS = (1, 3, 4, 5)
SAFE = (0, 1, 2)
TARGET = (0, 5)
LAYOUTS = (0, 4, 8, 12, 16, 32, 7)
OBS_DIMS = {capi.ENV_PENDULUM: 2, capi.ENV_CART_POLE: 4, capi.ENV_ACROBOT: 4, capi.ENV_COMPASS_WALKER: 5, capi.ENV_CART_POLE_BALANCING: 4,
            capi.ENV_EXTERNAL: 2}
STEP = {capi.ENV_PENDULUM: (0.03, 5, 2.99), capi.ENV_CART_POLE: (0.05, 5, 9.99), capi.ENV_ACROBOT: (0.05, 5, 20.0),
        capi.ENV_COMPASS_WALKER: (0.2, 20, 100.0), capi.ENV_CART_POLE_BALANCING: (0.05, 5, 9.99), capi.ENV_EXTERNAL: (0.03, 5, 2.99)}


ADMITTED = (capi.ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback")


def config(lib, env, agent, trace, actions, safe, target, layout, tap_deferred=0, taps=0, test_trials=0):
    """A configuration that is valid but for the fields under test: tile codings of the right width for the environment and the agent."""
    cfg = capi.Config()
    lib.grlx_config_pendulum_sarsa(C.byref(cfg))
    cfg.n_replicas, cfg.env, cfg.agent, cfg.trace = 5, env, agent, trace
    cfg.control_step, cfg.integration_steps, cfg.timeout = STEP[env]
    cfg.action_steps, cfg.replicas_per_wave, cfg.target_interval, cfg.target_tau = actions, layout, target, 0.5
    cfg.kappa, cfg.beta, cfg.actor_alpha, cfg.sigma, cfg.theta, cfg.ac_decay_rate = 0.5, 0.1, 0.01, 5.0, 1.0, 1.0
    d = OBS_DIMS[env]
    wide = d if agent == capi.AGENT_AC else d + 1
    for ts, dims in ((cfg.projector, wide), (cfg.actor_projector, d)):
        ts.tilings, ts.memory, ts.dims, ts.safe = 16, 8388608, dims, 0
        for i in range(capi.MAX_DIMS):
            ts.resolution[i], ts.wrapping[i] = (1.0 if i < dims else 0.0), 0.0
    cfg.projector.safe = safe
    cfg.actor_representation = cfg.representation
    cfg.tap_deferred, cfg.test_trials = tap_deferred, test_trials
    cfg.table_log2_capacity = 8         # (where there is a GPU the admitted contexts are created: small ones)
    if taps:
        cfg.tap_replica, cfg.tap_capacity = 0, 64
    return cfg


def listing(lib):
    """The lines of the listing for the library `lib` (a ctypes handle of libgrlx.so)."""
    lib.grlx_create.restype, lib.grlx_last_error.restype, lib.grlx_destroy.argtypes = C.c_int, C.c_char_p, [C.c_void_p]
    seeds = (C.c_int64 * 8)(*range(1, 9))
    numbers, head, body = {}, [], []

    def ask(cfg):
        ctx = C.c_void_p()
        code = lib.grlx_create(C.byref(cfg), seeds, C.byref(ctx))
        key = (code, lib.grlx_last_error().decode())
        if code == capi.OK:       # a box with a GPU: admitted is admitted
            lib.grlx_destroy(ctx)
            key = ADMITTED
        if key not in numbers:
            numbers[key] = len(numbers)
            head.append("M%d %d %s" % (numbers[key], key[0], key[1]))
        return "0123456789abcdefghijklmnopqrstuvwxyz"[numbers[key]]

    # one line per (environment, agent, trace); per number of actions a group: safe x target blocks of one character per forced layout
    # (the message number in base 36), then -- where the rest of the configuration is plain -- a block of tap_deferred /
    # tap_deferred + taps / taps + test_trials 3 / test_trials 3
    for env, agent, trace in itertools.product(ENVS, AGENTS, TRACES):
        groups = []
        for actions in ACTIONS:
            blocks = ["".join(ask(config(lib, env, agent, trace, actions, safe, target, layout)) for layout in LAYOUTS)
                      for safe, target in itertools.product(SAFE, TARGET)]
            blocks.append("".join(ask(config(lib, env, agent, trace, actions, 0, 0, 0, **kw)) for kw in (
                dict(tap_deferred=1), dict(tap_deferred=1, taps=1), dict(taps=1, test_trials=3), dict(test_trials=3))))
            groups.append("%d: %s" % (actions, " ".join(blocks)))
        body.append("env %d agent %d trace %d actions %s" % (env, agent, trace, " | ".join(groups)))
    return head + body


if __name__ == "__main__":
    print("\n".join(listing(C.CDLL(capi.lib_path()))))
