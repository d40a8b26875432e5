"""Thin Python host over the C ABI: one `Runner` = one grlx context = the
replicas of one GPU.  All computation happens in the HIP kernels behind
include/grlx.h; this file only marshals arguments."""
import collections
import ctypes as C
import math

import numpy as np

from . import capi


def pendulum_sarsa_config(n_replicas=1, **overrides) -> capi.Config:
    """Config of the reference's tests/pendulum-sarsa-tc.yaml (cfg/pendulum/sarsa_tc.yaml semantics)."""
    lib = capi.load()
    cfg = capi.Config()
    lib.grlx_config_pendulum_sarsa(C.byref(cfg))
    cfg.n_replicas = n_replicas
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def cart_pole_ac_config(n_replicas=1, **overrides) -> capi.Config:
    """Config of the reference's cfg/cart_pole/ac_tc.yaml (actor-critic over two tile-coded tables)."""
    lib = capi.load()
    cfg = capi.Config()
    lib.grlx_config_cart_pole_ac(C.byref(cfg))
    cfg.n_replicas = n_replicas
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def _set_tile(ts, tilings, memory, resolution, wrapping):
    ts.tilings, ts.memory, ts.dims = tilings, memory, len(resolution)
    for i in range(capi.MAX_DIMS):
        ts.resolution[i] = resolution[i] if i < len(resolution) else 0.0
        ts.wrapping[i] = wrapping[i] if i < len(wrapping) else 0.0


def acrobot_q_config(n_replicas=1, agent=capi.AGENT_Q, **overrides) -> capi.Config:
    """dynamics/acrobot + task/acrobot/balancing (acrobot.cpp) under the TD agent block of the reference's
    cfg/pendulum/q_tc.yaml -- the reference ships no TD yaml for the acrobot: 3 torques
    over [-1, 1], control step 0.05 s, tile resolution [0.05, 0.05, 0.2, 0.4 | 1.0]."""
    cfg = pendulum_sarsa_config(n_replicas, agent=agent, **overrides)
    cfg.env = capi.ENV_ACROBOT
    cfg.control_step, cfg.integration_steps, cfg.timeout = 0.05, 5, 20.0
    cfg.action_min, cfg.action_max, cfg.action_steps = -1.0, 1.0, 3
    _set_tile(cfg.projector, 16, 8388608, [0.05, 0.05, 0.2, 0.4, 1.0], [0] * 5)
    return cfg


def compass_walker_q_config(n_replicas=1, agent=capi.AGENT_Q, **overrides) -> capi.Config:
    """The reference's cfg/compass_walker/qlearning_walk.yaml: model/compass_walker + task/compass_walker/walk,
    Q-learning over a 6-input tile coding, 3 hip torques over [-1.2, 1.2], control step 0.2 s (20 sub-steps)."""
    cfg = pendulum_sarsa_config(n_replicas, agent=agent, **overrides)
    cfg.env = capi.ENV_COMPASS_WALKER
    cfg.control_step, cfg.integration_steps, cfg.timeout = 0.2, 20, 100.0
    cfg.slope_angle, cfg.initial_state_variation, cfg.negative_reward = 0.004, 0.2, -100.0
    cfg.action_min, cfg.action_max, cfg.action_steps = -1.2, 1.2, 3
    _set_tile(cfg.projector, 16, 8388608, [0.0838, 0.1047, 0.1111, 0.2222, 10, 1.2], [0] * 6)
    return cfg


def sweep_grid(repetitions, **axes):
    """The replicas of a grid sweep: the Cartesian product of the axes in the order given, the last axis fastest, every point
    repeated `repetitions` times -- replica i = point * repetitions + k.  Returns {axis: [value of replica i]} (plain lists,
    ready for Runner.set_replica_params); `grlxd -p` lays its clones out in the same order."""
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("repetitions must be >= 1")
    names = list(axes)
    values = [list(axes[n]) for n in names]
    if not names or any(len(v) == 0 for v in values):
        raise ValueError("every axis needs at least one value")
    points = 1
    for v in values:
        points *= len(v)
    out = {n: [] for n in names}
    for point in range(points):
        rest = point
        at = [0] * len(names)
        for a in range(len(names) - 1, -1, -1):
            at[a] = rest % len(values[a])
            rest //= len(values[a])
        for a, n in enumerate(names):
            out[n].extend([float(values[a][at[a]])] * repetitions)
    return out


def snapshot_info(src) -> capi.SnapshotInfo:
    """grlx_snapshot_info of a snapshot file (a path) or of its bytes: the header's fields and the grlx_config; needs no device."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytes(src)
    else:
        with open(src, "rb") as f:
            data = f.read()
    info = capi.SnapshotInfo()
    capi.check(capi.load().grlx_snapshot_info(data, len(data), C.byref(info)))
    return info


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


# ---- what the evaluation calls of Runner and FqiRunner share
def _state_rows(states, dims):
    states = np.ascontiguousarray(states, dtype=np.float64)
    if states.ndim != 2 or states.shape[1] != dims:
        raise ValueError(f"expected states of shape (n, {dims}), got {states.shape}")
    return states


_RULES = {"vote": capi.ENSEMBLE_VOTE, "mean": capi.ENSEMBLE_MEAN_Q, "mean_q": capi.ENSEMBLE_MEAN_Q}


def _rule(rule):
    return _RULES[rule] if isinstance(rule, str) else int(rule)


_ENSEMBLE_FIELDS = "ret disc steps terminal ties member_ties agreement final_state"
_SAMPLED_FIELDS = "ret disc steps terminal ties explored final_state streams"
_NOISY_FIELDS = "ret disc steps terminal clipped final_state streams noise"
_ACTOR_ENSEMBLE_FIELDS = "ret disc steps terminal ties kept spread final_state"
_ACTOR_RULES = {"mean": capi.ACTOR_ENSEMBLE_MEAN, "binning": capi.ACTOR_ENSEMBLE_BINNING, "data_center": capi.ACTOR_ENSEMBLE_DATA_CENTER,
                "density": capi.ACTOR_ENSEMBLE_DENSITY}
_BASE_OUTPUTS = {"ret": np.float64, "disc": np.float64, "steps": np.int32, "terminal": np.int32, "ties": np.int32}
_CTYPES = {np.float64: C.c_double, np.int32: C.c_int32, np.int64: C.c_int64, np.uint64: C.c_uint64}


def _episode_outputs(rows, n, state_dims, fields, records=None, **extra):
    """The zeroed output arrays of an evaluation call for `rows` replicas or groups and n start states, in the order of `fields` -- the
    order of the C call's output pointers and of the result tuple: ret, disc, steps, terminal, ties [rows][n], final_state
    [rows][n][state_dims], and the variant's own fields, extra[name] = an int32, int64, uint64 or float64 dtype or (dtype, width) for
    [rows][n][width].  records = (max_steps, words): a last array [rows][n][max_steps][words].  Returns (arrays, their pointers)."""
    arrays = []
    for name in fields.split():
        dtype = (np.float64, state_dims) if name == "final_state" else extra.get(name) or _BASE_OUTPUTS[name]
        dtype, tail = dtype if isinstance(dtype, tuple) else (dtype, None)
        arrays.append(np.zeros((rows, n) if tail is None else (rows, n, tail), dtype))
    if records is not None:
        arrays.append(np.zeros((rows, n, max(records[0], 0), records[1]), np.float64))
    return arrays, [_ptr(a, _CTYPES[a.dtype.type]) for a in arrays]


class Runner:
    """N independent-seed replicas of one experiment graph on the current GPU
    (the reference's experiment/multi clones, base/src/experiments/multi.cpp:44-75)."""

    def __init__(self, cfg: capi.Config, seeds):
        self.lib = capi.load()
        self.cfg = cfg
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        if seeds.shape != (cfg.n_replicas,):
            raise ValueError("need one seed per replica")
        self.seeds = seeds
        self._ctx = C.c_void_p()
        capi.check(self.lib.grlx_create(C.byref(cfg), _ptr(seeds, C.c_int64), C.byref(self._ctx)))
        if cfg.env == capi.ENV_EXTERNAL:        # the caller's environment: the agent's observation = the projector's input (minus the action)
            self.state_dims, self.obs_dims = 0, cfg.projector.dims - (0 if cfg.agent == capi.AGENT_AC else 1)
        else:
            sd, od = C.c_int(), C.c_int()
            capi.check(self.lib.grlx_env_dims(cfg.env, C.byref(sd), C.byref(od)))
            self.state_dims, self.obs_dims = sd.value, od.value

    # ---- exact resume: the whole context as one byte string (include/grlx.h: grlx_snapshot_*) ----
    def snapshot_size(self) -> int:
        n = C.c_uint64(0)
        capi.check(self.lib.grlx_snapshot_size(self._ctx, C.byref(n)))
        return n.value

    def _snapshot_view(self, cap=None) -> memoryview:
        cap = self.snapshot_size() if cap is None else int(cap)
        buf = (C.c_ubyte * max(cap, 1))()
        n = C.c_uint64(0)
        capi.check(self.lib.grlx_snapshot_save(self._ctx, buf, cap, C.byref(n)))
        return memoryview(buf)[: n.value]

    def snapshot(self, cap: int = None) -> bytes:
        """The context's snapshot (waits for what is in flight; the context is left as it was).  cap: the buffer handed to the
        library, by default exactly grlx_snapshot_size."""
        return bytes(self._snapshot_view(cap))

    def load_snapshot(self, data: bytes):
        """Continue from a snapshot: allowed before the first launch of the context; a refusal leaves the context as it was."""
        data = bytes(data)
        capi.check(self.lib.grlx_snapshot_load(self._ctx, data, len(data)))

    def save_state(self, path):
        with open(path, "wb") as f:
            f.write(self._snapshot_view())          # straight from the buffer the library filled: one copy of a snapshot in memory

    def load_state(self, path):
        with open(path, "rb") as f:
            self.load_snapshot(f.read())

    @classmethod
    def from_state(cls, path, **layout):
        """A context continued from the snapshot in `path`: the configuration is the snapshot's, with `layout` overriding the fields results
        do not depend on (replicas_per_wave, wave_limit, force_generic, table_log2_capacity, table_log2_max).  The seeds given to grlx_create
        do not matter: every state is overwritten by the load."""
        info = snapshot_info(path)
        cfg = capi.Config.from_buffer_copy(info.config)
        allowed = ("replicas_per_wave", "wave_limit", "force_generic", "table_log2_capacity", "table_log2_max")
        for k, v in layout.items():
            if k not in allowed:
                raise ValueError(f"{k} is not a layout field: a continued context keeps the snapshot's {k}")
            setattr(cfg, k, v)
        r = cls(cfg, np.zeros(cfg.n_replicas, np.int64))
        try:
            r.load_state(path)
        except Exception:
            r.close()
            raise
        return r

    def close(self):
        if self._ctx:
            self.lib.grlx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # OnlineLearningExperiment::run for n_trials further trials (async on `stream`)
    def run(self, n_trials: int, stream: int = 0):
        capi.check(self.lib.grlx_run(self._ctx, int(n_trials), C.c_void_p(stream)))

    def run_steps(self, max_trials: int, steps: int, stream: int = 0):
        """The trial loop with both bounds (online_learning.cpp:154): at most max_trials further trials per replica, none started once
        the replica's learning steps of the run have reached `steps`."""
        capi.check(self.lib.grlx_run_steps(self._ctx, int(max_trials), int(steps), C.c_void_p(stream)))

    def sync(self, stream: int = 0):
        capi.check(self.lib.grlx_sync(self._ctx, C.c_void_p(stream)))

    def replica_rows(self, replica: int) -> int:
        return capi.check(self.lib.grlx_replica_rows(self._ctx, int(replica)))

    def set_diag(self, enable: bool = True):
        capi.check(self.lib.grlx_set_diag(self._ctx, int(enable)))

    def read_diag(self):
        waves = (self.cfg.n_replicas + 3) // 4
        out = np.zeros((waves, 8), np.uint64)
        n = C.c_int()
        capi.check(self.lib.grlx_read_diag(self._ctx, _ptr(out, C.c_uint64), waves, C.byref(n)))
        return out[: n.value]

    def n_rows(self) -> int:
        return capi.check(self.lib.grlx_rows(self._ctx))

    def rows(self, replica: int, first: int = 0, count: int = None):
        if count is None:
            count = self.replica_rows(replica) - first
        trial = np.zeros(count, np.int64)
        steps = np.zeros(count, np.int64)
        reward = np.zeros(count, np.float64)
        capi.check(self.lib.grlx_read_rows(self._ctx, replica, first, count, _ptr(trial, C.c_int64),
                                           _ptr(steps, C.c_int64), _ptr(reward, C.c_double)))
        return trial, steps, reward

    def last_kernel(self) -> int:
        """capi GRLX_KERNEL_*: 1 generic, 2 specialised (compile-time instantiation), 3 diagnostic in-place."""
        return self.lib.grlx_last_kernel(self._ctx)

    def last_kernel_name(self) -> str:
        """The row of the kernel table the context launched last, as spelled there ("" before the first launch) -- diagnostic export."""
        return self.lib.grlx_last_kernel_name(self._ctx).decode()

    def env_server_counts(self):
        """(replicas served by the environment server to the end of the last launch that had it, replicas that fell back to integrating
        themselves); (0, 0) when no launch of this context had it -- diagnostic export, not part of include/grlx.h"""
        a, b = C.c_int(0), C.c_int(0)
        capi.check(self.lib.grlx_env_server_counts(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def uniform_pass_counts(self):
        """Per replica, the passes its wave took in the wave-uniform loop of rollout_served_kernel in the last launch that had the
        environment server (zeros when none had it) -- diagnostic export, not part of include/grlx.h"""
        out = np.zeros(self.cfg.n_replicas, dtype=np.uint64)
        capi.check(self.lib.grlx_uniform_pass_counts(self._ctx, _ptr(out, C.c_ulonglong), out.size))
        return out

    def env_server_flags(self):
        """Per replica, what env_server_counts sums: 1 served by the environment server to the end of the last launch that had it, 2 fell
        back to integrating itself (zeros when no launch had it) -- diagnostic export, not part of include/grlx.h"""
        out = np.zeros(self.cfg.n_replicas, dtype=np.int32)
        capi.check(self.lib.grlx_env_server_flags(self._ctx, _ptr(out, C.c_int32), out.size))
        return out

    def replicas_per_wave(self) -> int:
        """4: one replica per 16 lanes; 8: two sub-batches per wave sharing the environment phase (wide kernels); 12 / 16: three / four
        sub-batches (actor-critic only; 12 rotates the wave's own replicas through its slots trial by trial)."""
        return self.lib.grlx_replicas_per_wave(self._ctx)

    def row_times(self, replica: int, first: int = 0, count: int = None):
        """Episode time of each row's trial (column 4, online_learning.cpp:243): steps under discrete_time."""
        if count is None:
            count = self.n_rows() - first
        out = np.zeros(count, np.float64)
        capi.check(self.lib.grlx_read_row_times(self._ctx, replica, first, count, _ptr(out, C.c_double)))
        return out

    def curve_stats(self, out_dev_ptr: int, first: int, count: int, stream: int = 0):
        capi.check(self.lib.grlx_curve_stats(self._ctx, first, count, C.c_void_p(out_dev_ptr), C.c_void_p(stream)))

    def curve_stats_grouped(self, out_dev_ptr: int, first: int, count: int, group_size: int, stream: int = 0):
        """grlx_curve_stats per group of `group_size` consecutive replicas (the repetitions of one sweep point):
        device buffer out[count][n_replicas // group_size][3]."""
        capi.check(self.lib.grlx_curve_stats_grouped(self._ctx, first, count, int(group_size), C.c_void_p(out_dev_ptr), C.c_void_p(stream)))

    # ---- hyper-parameter sweep: alpha / gamma / lambda / epsilon per replica (include/grlx.h) ----
    def set_replica_params(self, alpha=None, gamma=None, lambda_=None, epsilon=None):
        """One value per replica for each parameter given (see sweep_grid); the others keep the configuration's value.
        Only before the first run of the context; makes it a sweep context.

        grlx_set_replica_params takes one parameter per call and validates it against the other three as they stand, so a grid
        whose final (gamma, lambda) pairs are all valid could be refused on the way there (gamma = 0.99 beside the
        configuration's lambda = 0.65, though its own lambda is 0.4).  With both given, lambda therefore first goes to
        min(current, new) per replica -- a shorter trace is always valid -- then gamma, then lambda: every valid grid is
        accepted in any order of values.  A refusal leaves all four parameters as they were before the call."""
        given = {}
        for name, values in (("alpha", alpha), ("gamma", gamma), ("lambda_", lambda_), ("epsilon", epsilon)):
            if values is None:
                continue
            v = np.ascontiguousarray(values, dtype=np.float64)
            if v.shape != (self.cfg.n_replicas,):
                raise ValueError("need one value per replica")
            given[name] = v
        if not given:
            return
        before = self.replica_params()
        applied = []
        try:
            for name in ("alpha", "epsilon"):
                if name in given:
                    self._set_param(name, given[name])
                    applied.append(name)
            if "gamma" in given and "lambda_" in given:
                applied += ["gamma", "lambda_"]
                self._set_gamma_lambda(before["lambda_"], given["gamma"], given["lambda_"])
            else:
                for name in ("gamma", "lambda_"):
                    if name in given:
                        self._set_param(name, given[name])
            # (a single gamma or lambda_ that is refused was not applied)
        except capi.GrlxError:
            if "gamma" in applied:
                self._set_gamma_lambda(self.replica_params()["lambda_"], before["gamma"], before["lambda_"])
            for name in applied:
                if name in ("alpha", "epsilon"):
                    self._set_param(name, before[name])
            raise

    _PARAMS = {"alpha": capi.PARAM_ALPHA, "gamma": capi.PARAM_GAMMA, "lambda_": capi.PARAM_LAMBDA, "epsilon": capi.PARAM_EPSILON}

    def _set_param(self, name, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        capi.check(self.lib.grlx_set_replica_params(self._ctx, self._PARAMS[name], _ptr(v, C.c_double)))

    def _set_gamma_lambda(self, lambda_now, gamma, lambda_):
        self._set_param("lambda_", np.minimum(lambda_now, lambda_))      # (a NaN stays a NaN and is refused here, by name)
        self._set_param("gamma", gamma)
        self._set_param("lambda_", lambda_)

    def replica_params(self):
        """dict(alpha, gamma, lambda_, epsilon) of float64[n_replicas]: what every replica runs with."""
        out = {}
        for name, param in (("alpha", capi.PARAM_ALPHA), ("gamma", capi.PARAM_GAMMA), ("lambda_", capi.PARAM_LAMBDA), ("epsilon", capi.PARAM_EPSILON)):
            v = np.zeros(self.cfg.n_replicas, np.float64)
            capi.check(self.lib.grlx_get_replica_params(self._ctx, param, _ptr(v, C.c_double)))
            out[name] = v
        return out

    def step_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        capi.check(self.lib.grlx_step_counts(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def env_state(self, replica: int):
        st = np.zeros(capi.MAX_STATE, np.float64)
        capi.check(self.lib.grlx_get_env_state(self._ctx, replica, _ptr(st, C.c_double)))
        return st[: self.state_dims]

    def rng(self, replica: int):
        out = np.zeros(4, np.uint64)
        capi.check(self.lib.grlx_get_rng(self._ctx, replica, _ptr(out, C.c_uint64)))
        return out

    def weights(self, replica: int, slots, table: int = 0):
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(slots.size, np.float64)
        capi.check(self.lib.grlx_get_weights(self._ctx, table, replica, _ptr(slots, C.c_uint32), slots.size, _ptr(out, C.c_double)))
        return out

    def target_weights(self, replica: int, slots):
        """Values of the Q table's target network (representation `interval` / `tau`) and the synchronisations so far."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(slots.size, np.float64)
        n = C.c_uint32()
        capi.check(self.lib.grlx_get_target_weights(self._ctx, replica, _ptr(slots, C.c_uint32), slots.size, _ptr(out, C.c_double), C.byref(n)))
        return out, n.value

    def export_weights(self, replica: int, table: int = 0):
        """Dense double[memory] parameter vector, as grl's .dat files hold it (representation.h:201-229)."""
        t = self.cfg.actor_projector if table == 1 else self.cfg.projector
        out = np.zeros(t.memory, np.float64)
        capi.check(self.lib.grlx_export_weights(self._ctx, table, replica, _ptr(out, C.c_double)))
        return out

    def load_weights(self, dense, table: int = 0, first_replica: int = 0, n_replicas=None):
        """ParameterizedRepresentation {action: load} (representation.h:231-263): every weight of `table`
        of the given replicas becomes dense[slot]; nothing else of the experiment changes."""
        dense = np.ascontiguousarray(dense, dtype=np.float64)
        if n_replicas is None:
            n_replicas = self.cfg.n_replicas - first_replica
        capi.check(self.lib.grlx_load_weights(self._ctx, table, first_replica, n_replicas, _ptr(dense, C.c_double), dense.size))

    def table_load(self, replica: int, table: int = 0) -> int:
        n = C.c_uint32()
        capi.check(self.lib.grlx_table_load(self._ctx, table, replica, C.byref(n)))
        return n.value

    def table_capacity(self) -> int:
        """log2 of the entries per replica and table (the sparse tables grow between launches)."""
        n = C.c_uint32(0)
        capi.check(self.lib.grlx_table_capacity(self._ctx, C.byref(n)))
        return int(n.value)

    def reset_run(self):
        """Experiment::reset() between two runs (online_learning.cpp:307-308): see grlx_reset_run."""
        capi.check(self.lib.grlx_reset_run(self._ctx))

    def grow_tables(self, new_log2: int):
        capi.check(self.lib.grlx_grow_tables(self._ctx, new_log2))

    def taps(self):
        cap = max(int(self.cfg.tap_capacity), 1)
        buf = (capi.Tap * cap)()
        n = C.c_int()
        capi.check(self.lib.grlx_read_taps(self._ctx, buf, cap, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    # ---- the per-step plug-in interfaces: one call of the reference's interface for every replica (include/grlx.h) ----
    def _active(self, active):
        if active is None:
            return None, None
        a = np.ascontiguousarray(active, dtype=np.int32)
        if a.shape != (self.cfg.n_replicas,):
            raise ValueError("active: one entry per replica")
        return a, _ptr(a, C.c_int32)

    def _rows(self, x, cols=None):
        shape = (self.cfg.n_replicas,) if cols is None else (self.cfg.n_replicas, cols)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != shape:
            raise ValueError(f"expected an array of shape {shape}, got {x.shape}")
        return x

    def env_start(self, test: int, active=None, obs=None):
        """Environment::start (environment.h:48) for the replicas: first observations [n_replicas][obs_dims]."""
        obs = np.zeros((self.cfg.n_replicas, self.obs_dims), np.float64) if obs is None else self._rows(obs, self.obs_dims)
        keep, ap = self._active(active)
        capi.check(self.lib.grlx_env_start(self._ctx, int(test), ap, _ptr(obs, C.c_double)))
        return obs

    def env_advance(self, action, active=None, obs=None, reward=None, terminal=None):
        """Environment::step (environment.h:49-51) on the replicas' model states: (obs, reward, terminal); tau = 1."""
        n = self.cfg.n_replicas
        action = self._rows(action)
        obs = np.zeros((n, self.obs_dims), np.float64) if obs is None else self._rows(obs, self.obs_dims)
        reward = np.zeros(n, np.float64) if reward is None else self._rows(reward)
        terminal = np.zeros(n, np.int32) if terminal is None else np.ascontiguousarray(terminal, dtype=np.int32)
        keep, ap = self._active(active)
        capi.check(self.lib.grlx_env_advance(self._ctx, ap, _ptr(action, C.c_double), _ptr(obs, C.c_double), _ptr(reward, C.c_double), _ptr(terminal, C.c_int32)))
        return obs, reward, terminal

    def agent_start(self, test: int, obs, active=None, action=None):
        """Agent::start (agent.h:44-47): test = 0 the learning agent, 1 the test agent; returns the actions [n_replicas]."""
        obs = self._rows(obs, np.asarray(obs).shape[-1])
        action = np.zeros(self.cfg.n_replicas, np.float64) if action is None else self._rows(action)
        keep, ap = self._active(active)
        capi.check(self.lib.grlx_agent_start(self._ctx, int(test), ap, _ptr(obs, C.c_double), _ptr(action, C.c_double)))
        return action

    def agent_step(self, test: int, obs, reward, terminal=None, active=None, action=None, tau: float = 1.0):
        """Agent::step (agent.h:49-52); replicas whose `terminal` entry is 2 get Agent::end instead and keep their `action` row."""
        obs = self._rows(obs, np.asarray(obs).shape[-1])
        reward = self._rows(reward)
        action = np.zeros(self.cfg.n_replicas, np.float64) if action is None else self._rows(action)
        tp = None
        if terminal is not None:
            terminal = np.ascontiguousarray(terminal, dtype=np.int32)
            tp = _ptr(terminal, C.c_int32)
        keep, ap = self._active(active)
        capi.check(self.lib.grlx_agent_step(self._ctx, int(test), ap, float(tau), _ptr(obs, C.c_double), _ptr(reward, C.c_double), tp, _ptr(action, C.c_double)))
        return action

    def agent_end(self, test: int, obs, reward, active=None, tau: float = 1.0):
        """Agent::end (agent.h:54-56): the transition into an absorbing state."""
        obs = self._rows(obs, np.asarray(obs).shape[-1])
        reward = self._rows(reward)
        keep, ap = self._active(active)
        capi.check(self.lib.grlx_agent_end(self._ctx, int(test), ap, float(tau), _ptr(obs, C.c_double), _ptr(reward, C.c_double)))

    # Representation::read / write / update (batched rows, applied in order)
    def read(self, replica, idx, table: int = 0):
        replica = np.ascontiguousarray(replica, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        out = np.zeros(replica.size, np.float64)
        capi.check(self.lib.grlx_read(self._ctx, table, _ptr(replica, C.c_int32), _ptr(idx, C.c_uint32), replica.size, _ptr(out, C.c_double)))
        return out

    def write(self, replica, idx, target, alpha: float, table: int = 0):
        replica = np.ascontiguousarray(replica, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        target = np.ascontiguousarray(target, dtype=np.float64)
        capi.check(self.lib.grlx_write(self._ctx, table, _ptr(replica, C.c_int32), _ptr(idx, C.c_uint32), replica.size, _ptr(target, C.c_double), float(alpha)))

    def update(self, replica, idx, delta, table: int = 0):
        replica = np.ascontiguousarray(replica, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        delta = np.ascontiguousarray(delta, dtype=np.float64)
        capi.check(self.lib.grlx_update(self._ctx, table, _ptr(replica, C.c_int32), _ptr(idx, C.c_uint32), replica.size, _ptr(delta, C.c_double)))

    # ---- policy queries: the read side of the policies at observations of the caller's choice (include/grlx.h: grlx_query_*).
    # A query changes nothing in the context.  replicas: None = all, else a range(first, end) or a (first, count) pair.
    def _replica_range(self, replicas):
        if replicas is None:
            return 0, self.cfg.n_replicas
        if isinstance(replicas, range):
            if replicas.step != 1:
                raise ValueError("replicas: a contiguous range")
            return replicas.start, len(replicas)
        first, count = replicas
        return int(first), int(count)

    def _obs_rows(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != self.obs_dims:
            raise ValueError(f"expected observations of shape (n, {self.obs_dims}), got {obs.shape}")
        return obs

    def query_q(self, obs, replicas=None):
        """(q[replica][obs][action], value[replica][obs], greedy, n_max) of the Q agents: QPolicy::values, QPolicy::value under the greedy
        sampler, and GreedySampler::findmax's first maximum and number of maxima (a tie is reported, not broken)."""
        obs = self._obs_rows(obs)
        first, count = self._replica_range(replicas)
        n, na = obs.shape[0], max(int(self.cfg.action_steps), 0)
        q = np.zeros((count, n, na), np.float64)
        value = np.zeros((count, n), np.float64)
        greedy = np.zeros((count, n), np.int32)
        n_max = np.zeros((count, n), np.int32)
        capi.check(self.lib.grlx_query_q(self._ctx, first, count, _ptr(obs, C.c_double), n, _ptr(q, C.c_double), _ptr(value, C.c_double),
                                         _ptr(greedy, C.c_int32), _ptr(n_max, C.c_int32)))
        return q, value, greedy, n_max

    def query_state(self, obs, table, replicas=None):
        """out[replica][obs]: the read of a table over the observation alone -- actor-critic: 0 the critic's V(s), 1 ActionPolicy::read;
        QV: 1 = V(s)."""
        obs = self._obs_rows(obs)
        first, count = self._replica_range(replicas)
        out = np.zeros((count, obs.shape[0]), np.float64)
        capi.check(self.lib.grlx_query_state(self._ctx, int(table), first, count, _ptr(obs, C.c_double), obs.shape[0], _ptr(out, C.c_double)))
        return out

    def policy_action(self, obs, replicas=None):
        """The greedy action [replica][obs]: the discretizer's action at `greedy` for the Q agents (the first maximum: ties are not
        broken), the actor's read clipped to the action range for the actor-critic."""
        if self.cfg.agent == capi.AGENT_AC:
            return np.minimum(np.maximum(self.query_state(obs, 1, replicas), self.cfg.action_min), self.cfg.action_max)
        greedy = self.query_q(obs, replicas)[2]
        # UniformDiscretizer::configure (uniform.cpp:60-95), as grlx_create builds the action list
        delta = (self.cfg.action_max - self.cfg.action_min) / (float(self.cfg.action_steps) - 1) if self.cfg.action_steps != 1 else 0.0
        if math.isnan(delta):
            delta = 0.0
        actions = np.array([self.cfg.action_min + delta * k for k in range(self.cfg.action_steps)], np.float64)
        return actions[greedy]

    def query_ensemble_raw(self, obs, group_size=None, replicas=None):
        """grlx_query_ensemble as it is: out[group][obs][2 + 2A] = {sum value, sum value^2, sum q[0..A), votes[0..A)}, every sum over the
        group's replicas in ascending order."""
        obs = self._obs_rows(obs)
        first, count = self._replica_range(replicas)
        group_size = count if group_size is None else int(group_size)
        groups = count // group_size if group_size > 0 else 0
        out = np.zeros((groups, obs.shape[0], 2 + 2 * int(self.cfg.action_steps)), np.float64)
        capi.check(self.lib.grlx_query_ensemble(self._ctx, first, count, group_size, _ptr(obs, C.c_double), obs.shape[0], _ptr(out, C.c_double)))
        return out

    def query_ensemble(self, obs, group_size=None, replicas=None):
        """Ensemble statistics per group of `group_size` consecutive replicas (default: one group of all) and observation."""
        first, count = self._replica_range(replicas)
        group_size = count if group_size is None else int(group_size)
        return EnsembleResult(self.query_ensemble_raw(obs, group_size, replicas), group_size, int(self.cfg.action_steps))

    def evaluate(self, states, replicas=None, max_steps=0):
        """One greedy episode of the test agent per (replica, start state) pair, on the device, from states[n][state_dims] (the MODEL's
        state, time included: what get_env_state and the taps give) to its end or to max_steps (0 = GRLX_MAX_EPISODE_STEPS):
        Evaluation(ret, disc, steps, terminal, ties, final_state), each [replica][start] (final_state: [replica][start][state_dims]).
        terminal: 1 timed out, 2 absorbing, 0 cut at max_steps, 3 left the portable math's domain.  ties: steps at which the Q agents'
        maximum was not unique (the first maximum acts; no random draw).  The context is not changed (include/grlx.h: grlx_evaluate)."""
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        n = states.shape[0]
        out, ptrs = _episode_outputs(count, n, self.state_dims, "ret disc steps terminal ties final_state")
        capi.check(self.lib.grlx_evaluate(self._ctx, first, count, _ptr(states, C.c_double), n, int(max_steps), *ptrs))
        return Evaluation(*out)

    def evaluate_ensemble(self, states, group_size, rule="vote", replicas=None, max_steps=0):
        """One greedy episode per (group of `group_size` consecutive replicas, start state) pair, on the device: at every step the
        members' first maxima are counted and their Q-values summed in ascending replica order, and the episode takes the first maximum
        of the votes (rule "vote") or of the summed Q (rule "mean").  EnsembleEvaluation(ret, disc, steps, terminal, ties, member_ties,
        agreement, final_state), each [group][start]: ties = steps at which the combined score had more than one maximum, member_ties =
        member-steps at which a member's own maximum was not unique, agreement = member-steps whose own first maximum was the action
        taken.  disc uses the gamma of a group's first replica.  The context is not changed (include/grlx.h: grlx_evaluate_ensemble)."""
        rule = _rule(rule)
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        group_size = int(group_size)
        groups = count // group_size if group_size > 0 else 0
        n = states.shape[0]
        out, ptrs = _episode_outputs(groups, n, self.state_dims, _ENSEMBLE_FIELDS, member_ties=np.int64, agreement=np.int64)
        capi.check(self.lib.grlx_evaluate_ensemble(self._ctx, first, count, group_size, rule, _ptr(states, C.c_double), n, int(max_steps), *ptrs))
        return EnsembleEvaluation(*out)

    def trajectory_record_words(self, ensemble=False):
        """R, the doubles of one trajectory record of this context (grlx_trajectory_record_words)"""
        return capi.check(self.lib.grlx_trajectory_record_words(self._ctx, 1 if ensemble else 0))

    def evaluate_trajectory(self, states, max_steps, replicas=None):
        """Runner.evaluate with every step of every episode: Trajectory(ret, disc, steps, terminal, ties, final_state, records),
        records[replica][start][max_steps][R] with one record per step taken and zeros behind an episode's end.  The views .action,
        .reward, .value, .action_index, .n_max, .code, .obs and .state cut the records by name; .episode(k, s) gives the records of one
        episode.  max_steps sizes the records, so it has no default (include/grlx.h: grlx_evaluate_trajectory)."""
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        n, max_steps = states.shape[0], int(max_steps)
        out, ptrs = _episode_outputs(count, n, self.state_dims, "ret disc steps terminal ties final_state",
                                     records=(max_steps, self.trajectory_record_words(False)))
        capi.check(self.lib.grlx_evaluate_trajectory(self._ctx, first, count, _ptr(states, C.c_double), n, max_steps, *ptrs))
        return Trajectory(*out)

    def evaluate_trajectory_stream(self, states, max_steps, sink, replicas=None) -> int:
        """Runner.evaluate_trajectory's result chunk by chunk: sink(chunk) is called once per chunk of consecutive start states, in ascending
        order, with a TrajectoryChunk(first_start, ret, disc, steps, terminal, ties, final_state, records) of READ-ONLY views into the
        library's staging memory -- [replica][start of the chunk]..., records [replica][start][max_steps][R], the views .action, .reward, ...
        of a Trajectory -- while the next chunk is computed and copied.  The views are valid only inside the call of the sink: copy what
        is to be kept.  A truthy return of the sink stops the stream (GrlxError with ERR_STOPPED; an int's value is in the message); an
        exception raised in the sink stops it too and is raised again once the library has returned.  No other method of this Runner may
        be called from inside the sink (ERR_INVALID, "a streamed call is in progress").  Returns the number of chunks delivered
        (include/grlx.h: grlx_evaluate_trajectory_stream)."""
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        delivered, raised = [0], []

        def view(ptr, *shape):
            a = np.ctypeslib.as_array(ptr, shape=shape)
            a.flags.writeable = False
            return a

        def on_chunk(_user, cp):
            try:
                c = cp.contents
                rows, n = c.rows, c.n_starts
                chunk = TrajectoryChunk(c.first_start, view(c.ret, rows, n), view(c.disc, rows, n), view(c.steps, rows, n), view(c.terminal, rows, n),
                                        view(c.ties, rows, n), view(c.final_state, rows, n, c.state_dims),
                                        view(c.records, rows, n, c.max_steps, c.record_words))
                delivered[0] += 1
                stop = sink(chunk)
                if not stop:
                    return 0
                return stop if type(stop) is int and -2**31 <= stop < 2**31 else 1
            except BaseException as ex:              # a callback must not raise into the library: stop the stream, raise after it has returned
                raised.append(ex)
                return 1

        cb = capi.TRAJECTORY_SINK(on_chunk) if sink is not None else capi.TRAJECTORY_SINK()
        rc = self.lib.grlx_evaluate_trajectory_stream(self._ctx, first, count, _ptr(states, C.c_double), states.shape[0], int(max_steps), cb, None)
        if raised:
            raise raised[0]
        capi.check(rc)
        return delivered[0]

    def evaluate_ensemble_trajectory(self, states, group_size, max_steps, rule="vote", replicas=None):
        """Runner.evaluate_ensemble with every step of every episode: EnsembleTrajectory(..., records), records[group][start][max_steps][R];
        beside Trajectory's views .step_agreement (votes[mai] of the step) and .step_member_ties (members with a tie at the step), and
        .value is the combined score of the action taken (include/grlx.h: grlx_evaluate_ensemble_trajectory)."""
        rule = _rule(rule)
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        group_size, max_steps = int(group_size), int(max_steps)
        groups = count // group_size if group_size > 0 else 0
        n = states.shape[0]
        out, ptrs = _episode_outputs(groups, n, self.state_dims, _ENSEMBLE_FIELDS, member_ties=np.int64, agreement=np.int64,
                                     records=(max_steps, self.trajectory_record_words(True)))
        capi.check(self.lib.grlx_evaluate_ensemble_trajectory(self._ctx, first, count, group_size, rule, _ptr(states, C.c_double), n, max_steps, *ptrs))
        return EnsembleTrajectory(*out)

    # ---- sampled evaluation: the same episodes acted by the reference's samplers on streams the episodes carry (grlx_evaluate_sampled)
    def _sampled_args(self, states, sampler, epsilon, streams, replicas):
        samplers = {"greedy": capi.SAMPLER_GREEDY, "epsilon": capi.SAMPLER_EPSILON_GREEDY, "epsilon_greedy": capi.SAMPLER_EPSILON_GREEDY}
        sampler = samplers[sampler] if isinstance(sampler, str) else int(sampler)
        if isinstance(epsilon, str):
            if epsilon != "own":
                raise ValueError('epsilon: a number in [0, 1] or "own"')
            epsilon = capi.EPSILON_OWN
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        n = states.shape[0]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
            if streams.shape != (count, n, 2):
                raise ValueError(f"expected streams of shape ({count}, {n}, 2), got {streams.shape}")
        return states, sampler, float(epsilon), streams, first, count, n

    def evaluate_sampled(self, states, sampler="epsilon", epsilon="own", streams=None, replicas=None, max_steps=0):
        """Runner.evaluate's episodes acted by a sampler of the reference: "greedy" (the first maximum, a tie broken by a draw) or
        "epsilon" (epsilon-greedy; epsilon a number in [0, 1] for every replica, or "own": the replica's decayed epsilon as it stands).
        streams[replica][start][2]: the rand48 states every episode starts from -- [..][0] the sampler's stream (the epsilon draw),
        [..][1] the global stream (the random action, the tie break); None = copies of the replica's own two streams (see episode_streams).
        SampledEvaluation(ret, disc, steps, terminal, ties, explored, final_state, streams): ties = tie breaks drawn, explored = random
        actions taken, streams = both states after the last step.  The context is not changed (include/grlx.h: grlx_evaluate_sampled)."""
        states, sampler, epsilon, streams, first, count, n = self._sampled_args(states, sampler, epsilon, streams, replicas)
        out, ptrs = _episode_outputs(count, n, self.state_dims, _SAMPLED_FIELDS, explored=np.int32, streams=(np.uint64, 2))
        capi.check(self.lib.grlx_evaluate_sampled(self._ctx, first, count, _ptr(states, C.c_double), n, int(max_steps), sampler, epsilon,
                                                  None if streams is None else _ptr(streams, C.c_uint64), *ptrs))
        return SampledEvaluation(*out)

    def sampled_trajectory_record_words(self):
        """R of evaluate_sampled_trajectory's records: trajectory_record_words() + 1 (grlx_sampled_trajectory_record_words)"""
        return capi.check(self.lib.grlx_sampled_trajectory_record_words(self._ctx))

    def evaluate_sampled_trajectory(self, states, max_steps, sampler="epsilon", epsilon="own", streams=None, replicas=None):
        """Runner.evaluate_sampled with every step of every episode: SampledTrajectory(..., records), records[replica][start][max_steps][R]
        with Trajectory's views -- .action_index the index that acted, .n_max the number of maxima, .value Q of the action taken -- and
        .explored, 1.0 where the action was the random draw; the per-episode count is the field n_explored (include/grlx.h:
        grlx_evaluate_sampled_trajectory)."""
        states, sampler, epsilon, streams, first, count, n = self._sampled_args(states, sampler, epsilon, streams, replicas)
        max_steps = int(max_steps)
        out, ptrs = _episode_outputs(count, n, self.state_dims, _SAMPLED_FIELDS, explored=np.int32, streams=(np.uint64, 2),
                                     records=(max_steps, self.sampled_trajectory_record_words()))
        capi.check(self.lib.grlx_evaluate_sampled_trajectory(self._ctx, first, count, _ptr(states, C.c_double), n, max_steps, sampler, epsilon,
                                                             None if streams is None else _ptr(streams, C.c_uint64), *ptrs))
        return SampledTrajectory(*out)

    # ---- noisy evaluation: the actor-critic's episodes under its exploration, on a stream and a noise state the episodes carry (grlx_evaluate_noisy)
    def _noisy_args(self, states, sigma, theta, streams, noise, replicas):
        if isinstance(sigma, str):
            if sigma != "own":
                raise ValueError('sigma: a number >= 0 or "own"')
            sigma = capi.SIGMA_OWN
        if isinstance(theta, str):
            if theta != "own":
                raise ValueError('theta: a number in [0, 1] or "own"')
            theta = capi.THETA_OWN
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        n = states.shape[0]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
            if streams.shape != (count, n):
                raise ValueError(f"expected streams of shape ({count}, {n}), got {streams.shape}")
        if noise is not None:
            noise = np.ascontiguousarray(noise, dtype=np.float64)
            if noise.shape != (count, n):
                raise ValueError(f"expected noise of shape ({count}, {n}), got {noise.shape}")
        return states, float(sigma), float(theta), streams, noise, first, count, n

    def evaluate_noisy(self, states, sigma="own", theta="own", streams=None, noise=None, replicas=None, max_steps=0):
        """Runner.evaluate's episodes of the actor-critic acted by the policy that collects its data: the actor's read plus Gaussian /
        Ornstein-Uhlenbeck noise, clipped to the action range.  sigma: a number >= 0 for every replica, or "own": the replica's decayed
        sigma as it stands; theta: a number in [0, 1] (1 = independent Gaussian noise), or "own": the configuration's.
        streams[replica][start]: the rand48 state every episode draws from, None = a copy of the replica's thread-local stream (see
        episode_stream_words); noise[replica][start]: the noise state every episode starts on, None = 0.
        NoisyEvaluation(ret, disc, steps, terminal, clipped, final_state, streams, noise): clipped = steps whose noisy action lay outside
        the action range, streams / noise = both states after the last step.  The context is not changed (include/grlx.h:
        grlx_evaluate_noisy)."""
        states, sigma, theta, streams, noise, first, count, n = self._noisy_args(states, sigma, theta, streams, noise, replicas)
        out, ptrs = _episode_outputs(count, n, self.state_dims, _NOISY_FIELDS, clipped=np.int32, streams=np.uint64, noise=np.float64)
        capi.check(self.lib.grlx_evaluate_noisy(self._ctx, first, count, _ptr(states, C.c_double), n, int(max_steps), sigma, theta,
                                                None if streams is None else _ptr(streams, C.c_uint64),
                                                None if noise is None else _ptr(noise, C.c_double), *ptrs))
        return NoisyEvaluation(*out)

    def noisy_trajectory_record_words(self):
        """R of evaluate_noisy_trajectory's records: trajectory_record_words() + 2 (grlx_noisy_trajectory_record_words)"""
        return capi.check(self.lib.grlx_noisy_trajectory_record_words(self._ctx))

    def evaluate_noisy_trajectory(self, states, max_steps, sigma="own", theta="own", streams=None, noise=None, replicas=None):
        """Runner.evaluate_noisy with every step of every episode: NoisyTrajectory(..., records), records[replica][start][max_steps][R]
        with Trajectory's views -- .action the action that acted (noisy, clipped), .value the actor's read before noise and clip -- and
        .noise (the noise state after the step) and .clipped (1.0 where the step clipped); the per-episode count is the field n_clipped
        (include/grlx.h: grlx_evaluate_noisy_trajectory)."""
        states, sigma, theta, streams, noise, first, count, n = self._noisy_args(states, sigma, theta, streams, noise, replicas)
        max_steps = int(max_steps)
        out, ptrs = _episode_outputs(count, n, self.state_dims, _NOISY_FIELDS, clipped=np.int32, streams=np.uint64, noise=np.float64,
                                     records=(max_steps, self.noisy_trajectory_record_words()))
        capi.check(self.lib.grlx_evaluate_noisy_trajectory(self._ctx, first, count, _ptr(states, C.c_double), n, max_steps, sigma, theta,
                                                           None if streams is None else _ptr(streams, C.c_uint64),
                                                           None if noise is None else _ptr(noise, C.c_double), *ptrs))
        return NoisyTrajectory(*out)

    # ---- actor-critic ensembles: episodes on the members' combined action (grlx_evaluate_actor_ensemble)
    def _actor_ensemble_args(self, states, group_size, rule, bins, r, replicas):
        if isinstance(rule, str):
            if rule not in _ACTOR_RULES:
                raise ValueError(f"rule {rule!r}: one of {sorted(_ACTOR_RULES)}")
            rule = _ACTOR_RULES[rule]
        states = _state_rows(states, self.state_dims)
        first, count = self._replica_range(replicas)
        group_size = int(group_size)
        groups = count // group_size if group_size > 0 else 0
        return states, first, count, group_size, groups, int(rule), int(bins), float(r)

    def evaluate_actor_ensemble(self, states, group_size, rule="mean", bins=10, r=0.001, replicas=None, max_steps=0):
        """One episode per (group of `group_size` consecutive actor-critic replicas, start state) pair, on the device: at every step the
        members' noise-free actions (each what Runner.evaluate would act on for that replica) are combined in ascending replica order by
        mapping/policy/multi's rule "mean", "binning" (`bins` bins, 1 ... 64), "data_center" (`bins` = the members kept) or "density"
        (radius `r`), and the episode acts on the result.  ActorEnsembleEvaluation(ret, disc, steps, terminal, ties, kept, spread,
        final_state), each [group][start]: ties = steps at which the rule's selection tied (the first candidate acts; no random draw), kept
        = member-steps that entered the action taken, spread = the steps' max - min over the members, added up.  The defaults are the
        reference's; at its r = 0.001 nearly every density is exactly 1, so nearly every step ties and the group's first member acts.
        group_size 1 is Runner.evaluate.  The context is not changed (include/grlx.h: grlx_evaluate_actor_ensemble)."""
        states, first, count, group_size, groups, rule, bins, r = self._actor_ensemble_args(states, group_size, rule, bins, r, replicas)
        n = states.shape[0]
        out, ptrs = _episode_outputs(groups, n, self.state_dims, _ACTOR_ENSEMBLE_FIELDS, kept=np.int64, spread=np.float64)
        capi.check(self.lib.grlx_evaluate_actor_ensemble(self._ctx, first, count, group_size, rule, bins, r, _ptr(states, C.c_double), n, int(max_steps),
                                                         *ptrs))
        return ActorEnsembleEvaluation(*out)

    def actor_ensemble_trajectory_record_words(self):
        """R of evaluate_actor_ensemble_trajectory's records: trajectory_record_words() + 2 (grlx_actor_ensemble_trajectory_record_words)"""
        return capi.check(self.lib.grlx_actor_ensemble_trajectory_record_words(self._ctx))

    def evaluate_actor_ensemble_trajectory(self, states, group_size, max_steps, rule="mean", bins=10, r=0.001, replicas=None):
        """Runner.evaluate_actor_ensemble with every step of every episode: ActorEnsembleTrajectory(..., records),
        records[group][start][max_steps][R] with Trajectory's views -- .action the combined action, .value the members' arithmetic mean under
        every rule, .action_index the selected member ("density"), the winning bin ("binning") or -1, .n_max the tied candidates -- and
        .kept and .spread, per step; the per-episode sums are the fields n_kept and total_spread
        (include/grlx.h: grlx_evaluate_actor_ensemble_trajectory)."""
        states, first, count, group_size, groups, rule, bins, r = self._actor_ensemble_args(states, group_size, rule, bins, r, replicas)
        n, max_steps = states.shape[0], int(max_steps)
        out, ptrs = _episode_outputs(groups, n, self.state_dims, _ACTOR_ENSEMBLE_FIELDS, kept=np.int64, spread=np.float64,
                                     records=(max_steps, self.actor_ensemble_trajectory_record_words()))
        capi.check(self.lib.grlx_evaluate_actor_ensemble_trajectory(self._ctx, first, count, group_size, rule, bins, r, _ptr(states, C.c_double), n,
                                                                    max_steps, *ptrs))
        return ActorEnsembleTrajectory(*out)


Evaluation = collections.namedtuple("Evaluation", "ret disc steps terminal ties final_state")
EnsembleEvaluation = collections.namedtuple("EnsembleEvaluation", "ret disc steps terminal ties member_ties agreement final_state")


class _RecordViews:
    """Read-only views by name into records[..., max_steps, R] (include/grlx.h: GRLX_TRAJ_*).  `_OBS`: the word at which the observation
    starts; the model state follows it and has final_state's width."""
    __slots__ = ()
    _OBS = capi.TRAJ_OBS

    def _cut(self, lo, hi=None):
        view = self.records[..., lo] if hi is None else self.records[..., lo:hi]
        view.flags.writeable = False
        return view

    action = property(lambda self: self._cut(capi.TRAJ_ACTION))
    reward = property(lambda self: self._cut(capi.TRAJ_REWARD))
    value = property(lambda self: self._cut(capi.TRAJ_VALUE))
    action_index = property(lambda self: self._cut(capi.TRAJ_ACTION_INDEX))
    n_max = property(lambda self: self._cut(capi.TRAJ_N_MAX))
    code = property(lambda self: self._cut(capi.TRAJ_TERMINAL))
    obs = property(lambda self: self._cut(self._OBS, self.records.shape[-1] - self.final_state.shape[-1]))
    state = property(lambda self: self._cut(self.records.shape[-1] - self.final_state.shape[-1], self.records.shape[-1]))

    def episode(self, k, s):
        """the records of the steps pair (k, s) took: [steps[k, s]][R]"""
        view = self.records[k, s, :int(self.steps[k, s])]
        view.flags.writeable = False
        return view


class Trajectory(_RecordViews, collections.namedtuple("Trajectory", "ret disc steps terminal ties final_state records")):
    """What Runner.evaluate_trajectory returns: Evaluation's fields and records[replica][start][max_steps][R]."""
    __slots__ = ()


class TrajectoryChunk(_RecordViews, collections.namedtuple("TrajectoryChunk", "first_start ret disc steps terminal ties final_state records")):
    """What the sink of Runner.evaluate_trajectory_stream is handed: the start states first_start ... first_start + ret.shape[1] - 1 of the
    call, Trajectory's fields for them as read-only views that are valid only inside the sink."""
    __slots__ = ()


class EnsembleTrajectory(_RecordViews, collections.namedtuple("EnsembleTrajectory",
                                                              "ret disc steps terminal ties member_ties agreement final_state records")):
    """What Runner.evaluate_ensemble_trajectory returns: EnsembleEvaluation's fields and records[group][start][max_steps][R]."""
    __slots__ = ()
    _OBS = capi.TRAJ_ENS_OBS
    step_agreement = property(lambda self: self._cut(capi.TRAJ_ENS_AGREEMENT))
    step_member_ties = property(lambda self: self._cut(capi.TRAJ_ENS_MEMBER_TIES))


SampledEvaluation = collections.namedtuple("SampledEvaluation", "ret disc steps terminal ties explored final_state streams")


class SampledTrajectory(_RecordViews, collections.namedtuple("SampledTrajectory",
                                                             "ret disc steps terminal ties n_explored final_state streams records")):
    """What Runner.evaluate_sampled_trajectory returns: SampledEvaluation's fields and records[replica][start][max_steps][R], whose last word
    (after the model state) says whether the step's action was the random draw: the view .explored, per step.  The per-episode count that
    SampledEvaluation calls explored is the field n_explored here."""
    __slots__ = ()
    obs = property(lambda self: self._cut(self._OBS, self.records.shape[-1] - 1 - self.final_state.shape[-1]))
    state = property(lambda self: self._cut(self.records.shape[-1] - 1 - self.final_state.shape[-1], self.records.shape[-1] - 1))
    explored = property(lambda self: self._cut(self.records.shape[-1] - 1))


def episode_streams(seed: int, n_replicas: int, n_starts: int, first_pair: int = 0):
    """streams[n_replicas][n_starts][2] for Runner.evaluate_sampled from one seed (grlx_episode_streams; host only): stream k =
    2 * (first_pair + replica * n_starts + start) + which is srand48(seed) advanced by k * 2^20 draws, so no two episodes share a draw."""
    out = np.zeros((int(n_replicas), int(n_starts), 2), np.uint64)
    capi.load().grlx_episode_streams(int(seed), int(first_pair), out.shape[0] * out.shape[1], _ptr(out, C.c_uint64))
    return out


NoisyEvaluation = collections.namedtuple("NoisyEvaluation", "ret disc steps terminal clipped final_state streams noise")


class NoisyTrajectory(_RecordViews, collections.namedtuple("NoisyTrajectory",
                                                           "ret disc steps terminal n_clipped final_state streams final_noise records")):
    """What Runner.evaluate_noisy_trajectory returns: NoisyEvaluation's fields and records[replica][start][max_steps][R], whose two last
    words (after the model state) are the noise state after the step and whether the step clipped: the views .noise and .clipped, per step.
    The per-episode count that NoisyEvaluation calls clipped is the field n_clipped here, its noise the field final_noise."""
    __slots__ = ()
    obs = property(lambda self: self._cut(self._OBS, self.records.shape[-1] - 2 - self.final_state.shape[-1]))
    state = property(lambda self: self._cut(self.records.shape[-1] - 2 - self.final_state.shape[-1], self.records.shape[-1] - 2))
    noise = property(lambda self: self._cut(self.records.shape[-1] - 2))
    clipped = property(lambda self: self._cut(self.records.shape[-1] - 1))


ActorEnsembleEvaluation = collections.namedtuple("ActorEnsembleEvaluation", _ACTOR_ENSEMBLE_FIELDS)


class ActorEnsembleTrajectory(_RecordViews, collections.namedtuple("ActorEnsembleTrajectory",
                                                                   "ret disc steps terminal ties n_kept total_spread final_state records")):
    """What Runner.evaluate_actor_ensemble_trajectory returns: ActorEnsembleEvaluation's fields and records[group][start][max_steps][R], whose
    two last words (after the model state) are the members that entered the step's action and the step's max - min over the members: the
    views .kept and .spread, per step.  The per-episode sums that ActorEnsembleEvaluation calls kept and spread are the fields n_kept and
    total_spread here."""
    __slots__ = ()
    obs = property(lambda self: self._cut(self._OBS, self.records.shape[-1] - 2 - self.final_state.shape[-1]))
    state = property(lambda self: self._cut(self.records.shape[-1] - 2 - self.final_state.shape[-1], self.records.shape[-1] - 2))
    kept = property(lambda self: self._cut(self.records.shape[-1] - 2))
    spread = property(lambda self: self._cut(self.records.shape[-1] - 1))


def episode_stream_words(seed: int, n_replicas: int, n_starts: int, first_pair: int = 0):
    """streams[n_replicas][n_starts] for Runner.evaluate_noisy from one seed (grlx_episode_stream_words; host only): the even streams
    of episode_streams, episode_streams(...)[..., 0] -- stream of pair p = srand48(seed) advanced by p * 2^21 draws."""
    out = np.zeros((int(n_replicas), int(n_starts)), np.uint64)
    capi.load().grlx_episode_stream_words(int(seed), int(first_pair), out.shape[0] * out.shape[1], _ptr(out, C.c_uint64))
    return out


class EnsembleResult:
    """What Runner.query_ensemble returns, each [group][obs] (mean_q and votes: [group][obs][action]): mean_value and var_value (n - 1;
    NaN for groups of one) of QPolicy::value over the group's replicas, mean_q, votes (replicas whose greedy action is a) and majority
    (the action with most votes, the lowest index winning a tie).  `raw` holds the sums they are formed from."""

    def __init__(self, raw, group_size, n_actions):
        n = float(group_size)
        self.raw, self.group_size = raw, group_size
        s, ss = raw[..., 0], raw[..., 1]
        self.mean_value = s / n
        with np.errstate(divide="ignore", invalid="ignore"):
            self.var_value = (ss - s * s / n) / (n - 1.0) if group_size > 1 else np.full(s.shape, np.nan)
        self.mean_q = raw[..., 2:2 + n_actions] / n
        self.votes = raw[..., 2 + n_actions:2 + 2 * n_actions].astype(np.int64)
        self.majority = np.argmax(self.votes, axis=-1)          # argmax: the first of equal counts


def observation_grid(lo, hi, points):
    """The cartesian grid over [lo[i], hi[i]] with points[i] values per dimension (end points included), row-major -- the last
    dimension fastest: float64[prod(points)][len(lo)], ready for the query calls.  Pure numpy."""
    lo, hi = np.atleast_1d(np.asarray(lo, np.float64)), np.atleast_1d(np.asarray(hi, np.float64))
    points = np.atleast_1d(np.asarray(points, np.int64))
    if not (lo.shape == hi.shape == points.shape) or lo.ndim != 1:
        raise ValueError("lo, hi and points need one entry per dimension")
    if np.any(points < 1):
        raise ValueError("points must be >= 1")
    axes = [np.linspace(lo[i], hi[i], int(points[i])) for i in range(lo.size)]
    mesh = np.meshgrid(*axes, indexing="ij")
    return np.ascontiguousarray(np.stack([m.reshape(-1) for m in mesh], axis=1))


def pendulum_fqi_config(n_replicas=1, **overrides) -> capi.FqiConfig:
    """Config of the reference's tests/pendulum-fqi-ann.yaml (experiment/batch_learning + predictor/fqi + ANN)."""
    lib = capi.load()
    cfg = capi.FqiConfig()
    lib.grlx_fqi_config_pendulum(C.byref(cfg))
    cfg.n_replicas = n_replicas
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


class FqiRunner:
    """N independent-seed replicas of the batch-learning experiment (fitted Q-iteration over a 3-H-1 network) on the
    current GPU: include/grlx.h, grlx_fqi_*."""

    def __init__(self, cfg: capi.FqiConfig, seeds):
        self.lib = capi.load()
        self.cfg = cfg
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        if seeds.shape != (cfg.n_replicas,):
            raise ValueError("need one seed per replica")
        self._ctx = C.c_void_p()
        capi.check(self.lib.grlx_fqi_create(C.byref(cfg), _ptr(seeds, C.c_int64), C.byref(self._ctx)))
        self.n_params = 4 * cfg.hidden + cfg.hidden + 1

    def close(self):
        if self._ctx:
            self.lib.grlx_fqi_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_batch(self, stream: int = 0):
        capi.check(self.lib.grlx_fqi_run_batch(self._ctx, C.c_void_p(stream)))

    def sync(self, stream: int = 0):
        capi.check(self.lib.grlx_fqi_sync(self._ctx, C.c_void_p(stream)))

    def rows(self, replica: int, count: int):
        b = np.zeros(count, np.int64); t = np.zeros(count, np.int64); rew = np.zeros(count, np.float64)
        capi.check(self.lib.grlx_fqi_read_rows(self._ctx, replica, 0, count, _ptr(b, C.c_int64), _ptr(t, C.c_int64), _ptr(rew, C.c_double)))
        return b, t, rew

    def params(self, replica: int):
        out = np.zeros(self.n_params, np.float64)
        capi.check(self.lib.grlx_fqi_get_params(self._ctx, replica, _ptr(out, C.c_double), out.size))
        return out

    def transitions(self, replica: int, first: int, count: int):
        inp = np.zeros((count, 3), np.float64); nobs = np.zeros((count, 2), np.float64)
        rew = np.zeros(count, np.float64); tgt = np.zeros(count, np.float64)
        capi.check(self.lib.grlx_fqi_get_transitions(self._ctx, replica, first, count, _ptr(inp, C.c_double), _ptr(nobs, C.c_double),
                                                     _ptr(rew, C.c_double), _ptr(tgt, C.c_double)))
        return inp, nobs, rew, tgt

    def query(self, obs, replicas=None):
        """q[replica][obs][action]: the batch path's Q(s, a_k) on every replica's current parameters (grlx_fqi_query); replicas: None =
        all, else a range(first, end) or a (first, count) pair.  Changes nothing in the context."""
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != 2:
            raise ValueError(f"expected observations of shape (n, 2), got {obs.shape}")
        first, count = self._replica_range(replicas)
        q = np.zeros((count, obs.shape[0], self.cfg.action_steps), np.float64)
        capi.check(self.lib.grlx_fqi_query(self._ctx, first, count, _ptr(obs, C.c_double), obs.shape[0], _ptr(q, C.c_double)))
        return q

    def _replica_range(self, replicas):
        if replicas is None:
            return 0, self.cfg.n_replicas
        if isinstance(replicas, range):
            return replicas.start, len(replicas)
        first, count = (int(x) for x in replicas)
        return first, count

    STATE_DIMS = 3          # the pendulum's model state: angle, velocity, time

    def evaluate(self, states, replicas=None, max_steps=0):
        """One greedy episode of the fitted policy per (replica, start state) pair, on the device, from states[n][3] (the pendulum's
        MODEL state: angle, velocity, time) to its end or to max_steps (0 = GRLX_MAX_EPISODE_STEPS): Evaluation(ret, disc, steps,
        terminal, ties, final_state), each [replica][start].  The first maximum of Q(obs, .) acts; ties counts the steps at which it was
        not unique (no random draw).  terminal: 1 timed out, 0 cut at max_steps, 3 left the portable math's domain.  disc discounts by
        gamma ** control_step per step.  The context is not changed (include/grlx.h: grlx_fqi_evaluate)."""
        states = _state_rows(states, self.STATE_DIMS)
        first, count = self._replica_range(replicas)
        n = states.shape[0]
        out, ptrs = _episode_outputs(count, n, self.STATE_DIMS, "ret disc steps terminal ties final_state")
        capi.check(self.lib.grlx_fqi_evaluate(self._ctx, first, count, _ptr(states, C.c_double), n, int(max_steps), *ptrs))
        return Evaluation(*out)

    def trajectory_record_words(self):
        """R = 11, the doubles of one trajectory record (grlx_fqi_trajectory_record_words)"""
        return capi.check(self.lib.grlx_fqi_trajectory_record_words(self._ctx))

    def evaluate_trajectory(self, states, max_steps, replicas=None):
        """FqiRunner.evaluate with every step of every episode: Trajectory(ret, disc, steps, terminal, ties, final_state, records),
        records[replica][start][max_steps][11] with one record per step taken and zeros behind an episode's end; the views and
        .episode(k, s) are Runner.evaluate_trajectory's (include/grlx.h: grlx_fqi_evaluate_trajectory)."""
        states = _state_rows(states, self.STATE_DIMS)
        first, count = self._replica_range(replicas)
        n, max_steps = states.shape[0], int(max_steps)
        out, ptrs = _episode_outputs(count, n, self.STATE_DIMS, "ret disc steps terminal ties final_state",
                                     records=(max_steps, self.trajectory_record_words()))
        capi.check(self.lib.grlx_fqi_evaluate_trajectory(self._ctx, first, count, _ptr(states, C.c_double), n, max_steps, *ptrs))
        return Trajectory(*out)

    # ---- the ensemble over groups of `group_size` consecutive replicas (bagged FQI): Runner's calls of the same names restated
    def _groups(self, replicas, group_size):
        first, count = self._replica_range(replicas)
        group_size = max(count, 1) if group_size is None else int(group_size)      # an empty range is GRLX_OK with nothing written
        return first, count, group_size, (count // group_size if group_size > 0 else 0)

    def query_ensemble_raw(self, obs, group_size=None, replicas=None):
        """grlx_fqi_query_ensemble as it is: out[group][obs][2 + 2A] = {sum value, sum value^2, sum q[0..A), votes[0..A)}, every sum over
        the group's replicas in ascending order (Runner.query_ensemble_raw's columns)."""
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != 2:
            raise ValueError(f"expected observations of shape (n, 2), got {obs.shape}")
        first, count, group_size, groups = self._groups(replicas, group_size)
        out = np.zeros((groups, obs.shape[0], 2 + 2 * int(self.cfg.action_steps)), np.float64)
        capi.check(self.lib.grlx_fqi_query_ensemble(self._ctx, first, count, group_size, _ptr(obs, C.c_double), obs.shape[0], _ptr(out, C.c_double)))
        return out

    def query_ensemble(self, obs, group_size=None, replicas=None):
        """Ensemble statistics per group of `group_size` consecutive replicas (default: one group of all) and observation."""
        group_size = self._groups(replicas, group_size)[2]
        return EnsembleResult(self.query_ensemble_raw(obs, group_size, replicas), group_size, int(self.cfg.action_steps))

    def evaluate_ensemble(self, states, group_size, rule="vote", replicas=None, max_steps=0):
        """One greedy episode per (group of `group_size` consecutive replicas, start state) pair, on the device: at every step the
        members' first maxima are counted and their Q-values summed in ascending replica order, and the episode takes the first maximum
        of the votes (rule "vote") or of the summed Q (rule "mean").  EnsembleEvaluation(ret, disc, steps, terminal, ties, member_ties,
        agreement, final_state), each [group][start], as Runner.evaluate_ensemble defines them; the episode is FqiRunner.evaluate's.
        The context is not changed (include/grlx.h: grlx_fqi_evaluate_ensemble)."""
        rule = _rule(rule)
        states = _state_rows(states, self.STATE_DIMS)
        first, count, group_size, groups = self._groups(replicas, group_size)
        n = states.shape[0]
        out, ptrs = _episode_outputs(groups, n, self.STATE_DIMS, _ENSEMBLE_FIELDS, member_ties=np.int64, agreement=np.int64)
        capi.check(self.lib.grlx_fqi_evaluate_ensemble(self._ctx, first, count, group_size, rule, _ptr(states, C.c_double), n, int(max_steps), *ptrs))
        return EnsembleEvaluation(*out)

    def ensemble_trajectory_record_words(self):
        """R = 13, the doubles of one record of the ensemble's trajectory (grlx_fqi_ensemble_trajectory_record_words)"""
        return capi.check(self.lib.grlx_fqi_ensemble_trajectory_record_words(self._ctx))

    def evaluate_ensemble_trajectory(self, states, group_size, max_steps, rule="vote", replicas=None):
        """FqiRunner.evaluate_ensemble with every step of every episode: EnsembleTrajectory(..., records), records[group][start][max_steps]
        [13]; the views, .step_agreement, .step_member_ties and .episode(k, s) are Runner.evaluate_ensemble_trajectory's
        (include/grlx.h: grlx_fqi_evaluate_ensemble_trajectory)."""
        rule = _rule(rule)
        states = _state_rows(states, self.STATE_DIMS)
        first, count, group_size, groups = self._groups(replicas, group_size)
        n, max_steps = states.shape[0], int(max_steps)
        out, ptrs = _episode_outputs(groups, n, self.STATE_DIMS, _ENSEMBLE_FIELDS, member_ties=np.int64, agreement=np.int64,
                                     records=(max_steps, self.ensemble_trajectory_record_words()))
        capi.check(self.lib.grlx_fqi_evaluate_ensemble_trajectory(self._ctx, first, count, group_size, rule, _ptr(states, C.c_double), n, max_steps, *ptrs))
        return EnsembleTrajectory(*out)

    def info(self, replica: int):
        n = C.c_int64(); md = C.c_double(); it = C.c_int32(); err = C.c_double(); rng = (C.c_uint64 * 2)()
        capi.check(self.lib.grlx_fqi_info(self._ctx, replica, C.byref(n), C.byref(md), C.byref(it), C.byref(err), rng))
        return dict(n=n.value, maxdelta=md.value, iterations=it.value, error=err.value, rng=[rng[0], rng[1]])


# ---- stateless batched operators --------------------------------------------
def project(spec: capi.TileSpec, x):
    """Projector::project (TileCodingProjector::_project) for a batch of inputs."""
    lib = capi.load()
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, spec.dims)
    out = np.zeros((x.shape[0], spec.tilings), np.uint32)
    capi.check(lib.grlx_project(C.byref(spec), _ptr(x, C.c_double), x.shape[0], _ptr(out, C.c_uint32)))
    return out


def env_step(cfg: capi.Config, state, action):
    """Environment::step (ModeledEnvironment::step) for a batch of (state, action)."""
    lib = capi.load()
    sd, od = C.c_int(), C.c_int()
    capi.check(lib.grlx_env_dims(cfg.env, C.byref(sd), C.byref(od)))
    state = np.array(state, dtype=np.float64).reshape(-1, sd.value)
    action = np.ascontiguousarray(action, dtype=np.float64).reshape(-1)
    n = state.shape[0]
    obs = np.zeros((n, od.value), np.float64)
    reward = np.zeros(n, np.float64)
    terminal = np.zeros(n, np.int32)
    capi.check(lib.grlx_env_step(C.byref(cfg), _ptr(state, C.c_double), _ptr(action, C.c_double), n,
                                 _ptr(obs, C.c_double), _ptr(reward, C.c_double), _ptr(terminal, C.c_int32)))
    return state, obs, reward, terminal


MATH_SIN, MATH_COS, MATH_LOG, MATH_FMOD, MATH_SQRT, MATH_DIV6 = 0, 1, 2, 3, 4, 5
MATH_SIN_SMALL, MATH_COS_SMALL, MATH_SINCOS_SMALL = 6, 7, 8                 # psin_s, pcos_s, psincos_s (sine + cosine)
# the unchecked forms the rollout kernels and the environment servers call (|x| < 2^20, else GRLX_ERR_INVALID), and pexp
MATH_SIN_PINNED, MATH_SIN_SERVER, MATH_COS_PINNED, MATH_SINCOS_PINNED, MATH_EXP = 9, 10, 11, 12, 13


def device_math(op: int, x, y=None):
    lib = capi.load()
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    out = np.zeros_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        yp = _ptr(y, C.c_double)
    capi.check(lib.grlx_math(op, _ptr(x, C.c_double), yp, x.size, _ptr(out, C.c_double)))
    return out


def rand48_at(seed: int, skip):
    lib = capi.load()
    skip = np.ascontiguousarray(skip, dtype=np.uint64).reshape(-1)
    out = np.zeros(skip.size, np.float64)
    capi.check(lib.grlx_rand48_at(int(seed), _ptr(skip, C.c_uint64), skip.size, _ptr(out, C.c_double)))
    return out


def format_row(trial: int, steps: int, reward: float) -> str:
    """One row in the layout of the reference's golden files (three setw(15)
    columns, default ostream precision; tests/template/pendulum-sarsa-tc-0.txt)."""
    return "%15d%15d%15s\n" % (trial, steps, "%g" % reward) if not math.isnan(reward) else "%15d%15d%15s\n" % (trial, steps, "nan")
