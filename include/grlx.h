/* grlx.h -- C ABI of the MI355X-native runner for grl's online-learning hot path.
 *
 * This is the drop-in boundary: plain C, POD structs, caller-allocated buffers,
 * `int` status returns (0 = GRLX_OK, negative = error; grlx_last_error() has the
 * text), no exceptions, no torch/Eigen types.  One context owns the replicas of
 * one GPU; a context is not thread-safe.  Every entry point names the reference
 * interface it replaces (paths relative to the wcaarls/grl checkout); the
 * reference-side binding a grl maintainer would add is shown in INTEGRATION.md.
 *
 * There is NO CPU fallback: every compute entry point runs HIP kernels on the
 * current device and returns GRLX_ERR_NO_DEVICE when there is none.
 */
#ifndef GRLX_H_
#define GRLX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): grlx_config grew test_trials / reserved0 in round 3 and the per-step entry points were added; a binding compiled against
 * version 1's header must not drive this library (grlx_create would read past the end of its struct). */
#define GRLX_ABI_VERSION 2

enum {
  GRLX_OK = 0,
  GRLX_ERR_INVALID = -1,       /* bad argument / unsupported configuration (grl: bad_param)   */
  GRLX_ERR_NO_DEVICE = -2,     /* no HIP device: the product never computes on the CPU        */
  GRLX_ERR_HIP = -3,           /* HIP runtime error                                           */
  GRLX_ERR_TABLE_FULL = -4,    /* a replica's sparse weight table overflowed (raise capacity) */
  GRLX_ERR_DOMAIN = -5,        /* portable sin/cos argument outside |x| < 2^20                */
  GRLX_ERR_ROWS_FULL = -6,     /* more test rows than reserved at create                      */
  GRLX_ERR_OOM = -7,
  GRLX_ERR_STOPPED = -8        /* the sink of a streamed call returned nonzero (the message carries its value) */
};

/* YAML type strings of the reference these enumerators stand for */
enum { GRLX_ENV_PENDULUM = 0,        /* dynamics/pendulum + task/pendulum/swingup   (pendulum.cpp)       */
       GRLX_ENV_CART_POLE = 1,       /* dynamics/cart_pole + task/cart_pole/swingup (cart_pole.cpp)      */
       GRLX_ENV_ACROBOT = 2,         /* dynamics/acrobot + task/acrobot/balancing   (acrobot.cpp)        */
       GRLX_ENV_COMPASS_WALKER = 3,  /* sandbox/compass_walker (walk task)          (compass_walker.cpp) */
       GRLX_ENV_CART_POLE_BALANCING = 4,/* dynamics/cart_pole + task/cart_pole/balancing (cart_pole.cpp:239-320): the task of the
                                        reference's tests/cart_pole_balancing-pid.yaml; grlx_env_step only (grlx_create refuses it) */
       GRLX_ENV_EXTERNAL = 5         /* no environment in the context: it is the caller's (any grl Environment: gym, a robot, a CPU
                                        simulator).  Observation dimensions = the projector's input dimensions (minus the action's for
                                        the Q agents).  Only the per-step agent entry points (grlx_agent_start / _step / _end) and the
                                        table operators serve such a context; grlx_run, grlx_env_start and grlx_env_advance refuse it.
                                        The environment fields of grlx_config (control_step, timeout, ...) are not read. */ };
enum { GRLX_AGENT_SARSA = 0,         /* agent/td + policy/discrete/q + predictor/critic/sarsa (sarsa.cpp)     */
       GRLX_AGENT_Q = 1,             /* ... + predictor/critic/q (advantage.cpp:71-110)                       */
       GRLX_AGENT_AC = 2,            /* policy/action + predictor/ac/action + predictor/critic/td (ac.cpp)    */
       GRLX_AGENT_EXPECTED_SARSA = 3,/* ... + predictor/critic/expected_sarsa (sarsa.cpp:167-194)              */
       GRLX_AGENT_ADVANTAGE = 4,     /* ... + predictor/critic/advantage (advantage.cpp:222-268), `kappa`     */
       GRLX_AGENT_QV = 5             /* ... + predictor/critic/qv (qv.cpp:74-108): table 0 = Q, table 1 = V
                                        (v_projector / v_representation in the actor_* fields), `beta`     */ };
enum { GRLX_TRACE_NONE = 0, GRLX_TRACE_REPLACING = 1, GRLX_TRACE_ACCUMULATING = 2 };   /* trace.h:208-263 */

#define GRLX_MAX_DIMS 8
#define GRLX_MAX_STATE 12
#define GRLX_MAX_ACTIONS 8
/* An episode ends on the task's terminal state, at the latest on time > timeout; the fused kernels have no
 * other exit, so grlx_create refuses a non-finite or negative timeout and more control steps per episode
 * (timeout / control_step; twice that for the compass walker's test episodes) than this. */
#define GRLX_MAX_EPISODE_STEPS 100000

/* projector/tile_coding (tile_coding.cpp:34-80): tilings, memory, resolution, wrapping; safe = 0.
 * HARD LIMIT of the fused rollout kernels (grlx_create): tilings == 16 -- one lane per tiling, 16 lanes per replica, four (or
 * eight) replicas per 64-lane wavefront; anything else is GRLX_ERR_INVALID.  The reference takes any count (tile_coding.cpp:47);
 * the stateless operator grlx_project takes 1..32.  memory: 1 .. 2^26-1 slots. */
typedef struct {
  int32_t tilings;
  int32_t memory;
  int32_t dims;
  int32_t safe;                       /* collision detection (tile_coding.cpp:39): 0 = off; 1 = claim on write (single projections
                                         claim their slots with their hash sum, tile_coding.h:116-151) -- served by the plain kernel
                                         for SARSA / Q-learning on the pendulum and the acrobot; 2 = claim always: the policy's batch
                                         projections (tile_coding.h:67-73) claim too, one variant after the other */
  double  resolution[GRLX_MAX_DIMS];
  double  wrapping[GRLX_MAX_DIMS];
} grlx_tile_spec;

/* representation/parameterized/linear (linear.cpp:34-101) */
typedef struct {
  double  init_min, init_max;
  double  output_min, output_max;     /* +-DBL_MAX for the yaml's empty vectors */
  int32_t limit;                      /* default 1 (linear.h:46-49)             */
  int32_t reserved;
} grlx_linear_spec;

/* One fused experiment graph:
 *   experiment/online_learning { environment/modeled { model/dynamical, task },
 *                                agent/td { policy, predictor }, test_agent agent/fixed }
 * Field names follow the reference's YAML parameter names. */
typedef struct {
  uint32_t struct_size;               /* = sizeof(grlx_config), ABI check                       */
  int32_t  n_replicas;                /* independent-seed replicas on this GPU (experiment/multi analogue, multi.cpp:44-75) */
  int32_t  test_interval;             /* experiment: -1 = none                                  */
  int32_t  env;                       /* GRLX_ENV_*                                             */
  double   control_step;              /* model/dynamical                                        */
  int32_t  integration_steps;
  int32_t  discrete_time;             /* environment/modeled: must be 1                         */
  double   timeout;                   /* task                                                   */
  double   randomization;
  double   action_min, action_max;    /* discretizer/uniform over task action range             */
  int32_t  action_steps;
  int32_t  agent;                     /* GRLX_AGENT_*                                           */
  grlx_tile_spec   projector;
  grlx_linear_spec representation;
  double   epsilon, decay_rate, decay_min;    /* sampler/epsilon_greedy                         */
  double   alpha, gamma, lambda;              /* predictor                                      */
  int32_t  trace;                             /* GRLX_TRACE_*                                   */
  int32_t  tap_starts;                /* 1: taps also record the start of every trial (terminal = -1): the rows of a transition log */
  /* actor-critic only */
  grlx_tile_spec   actor_projector;
  grlx_linear_spec actor_representation;
  double   actor_alpha, sigma, theta, ac_decay_rate, ac_decay_min, ac_step_limit;
  int32_t  ac_update_method;
  /* GPU-side sizing (no reference counterpart) */
  int32_t  table_log2_capacity;       /* sparse table slots per replica = 2^this; 0 = default   */
  int32_t  max_rows;                  /* test rows reserved per replica                          */
  int32_t  tap_replica;               /* -1: off; else record per-step taps of that replica      */
  int32_t  tap_capacity;
  /* task/cart_pole/swingup (cart_pole.cpp:110-130); class defaults 1 / 0, cfg/cart_pole/ac_tc.yaml: 0 / 0 */
  int32_t  end_stop_penalty;
  int32_t  action_penalty;
  int32_t  force_generic;             /* 1: never pick a compile-time specialised kernel (tests) */
  /* model/compass_walker + task/compass_walker/walk (compass_walker.cpp:41-60, 198-249) */
  double   slope_angle;               /* default 0.004 */
  double   initial_state_variation;   /* default 0.2   */
  double   negative_reward;           /* default -100  */
  /* predictor/critic/advantage (advantage.cpp:183-213) */
  double   kappa;                     /* advantage scaling factor (cfg/pendulum/advantage_tc.yaml: 0.2) */
  /* predictor/critic/qv (qv.cpp:35-64): state-value learning rate; V's projector / representation
   * are given in actor_projector / actor_representation (the second table of the context) */
  double   beta;
  /* GPU-side layout (no reference counterpart): replicas carried by one wavefront.  0 = automatic: 4 (16 lanes per
   * replica, lane = tiling) while the batch has no more than 4 replicas per SIMD of the device, else 8 (two sub-batches
   * of four share one environment phase; grlx_rollout_wide.h).  4 / 8 force the choice (tests); the actor-critic kernel also
   * takes 12 and 16 (three / four sub-batches, the lane state of those beyond the second parked in registers; with 12 a wave
   * owns ceil(replicas / waves) replicas and rotates them through its slots trial by trial -- grlx_rollout_ac_wide.h; batches that
   * would give a wave more than 64 replicas run with 8).  Automatic for the actor-critic: 16 from 15 replicas per SIMD up, 12 for 9-14.
   * 16 also for the TD agents on the acrobot / the compass walker with three actions (round 4; automatic from 15 replicas per SIMD up),
   * 32 for the TD agents on the compass walker (eight sub-batches; automatic from 30 replicas per SIMD up).  Results are identical. */
  int32_t  replicas_per_wave;
  /* 1: the taps are recorded by the PRODUCTION ordering of the rollout kernel (TD update applied one pass later, under the
   * next step's table loads) instead of the in-place diagnostic ordering: per-step parity of the kernel that is benchmarked.
   * Built for the pendulum and the acrobot with 3 actions (SARSA / Q / Expected SARSA, replacing or no trace). */
  int32_t  tap_deferred;
  /* representation/parameterized/linear: interval, tau (ParameterizedRepresentation, representation.h:161-306): a TARGET
   * NETWORK on the Q table.  target_interval > 0: SARSA / Q-learning read their targets from a second copy of the
   * parameters (sarsa.cpp:107, advantage.cpp:88), synchronised as tau*params + (1-tau)*target (tau = 0: plain copy) every
   * target_interval LinearRepresentation::update calls (linear.cpp:267: one per write and one per trace entry).  Served by
   * its own plain kernel (pendulum / acrobot, 3 actions, replacing or no trace); 0 = none. */
  int32_t  target_interval;
  /* GPU-side layout (no reference counterpart), wide actor-critic kernel: at most this many wavefronts are launched; each
   * carries replicas_per_wave replicas at a time and takes the next unstarted replica from a device-side counter whenever
   * one of its slots has finished its trials (episodes of a learning batch are ragged: without the queue a wave idles until
   * its slowest replica is done).  0 = automatic: one wave per SIMD of the device.  Results do not depend on it (tests). */
  int32_t  wave_limit;
  /* Sparse weight tables: table_log2_capacity (above) is the INITIAL size, 2^k entries per replica and table.  Between
   * launches -- at the start of a grlx_run whose predecessor has been waited for (grlx_sync or any read-back) -- the fullest
   * table of the context is looked at, and beyond a quarter of the capacity all tables are re-hashed into larger ones
   * (results do not depend on it: positions are internal).  table_log2_max bounds the growth: 0 = up to 2^26; a value equal
   * to the initial size = fixed tables, overflow is then the sticky error GRLX_ERR_TABLE_FULL, as within one launch. */
  int32_t  table_log2_max;
  double   target_tau;
  /* experiment/online_learning:test_trials (online_learning.cpp:160-225): a test trial is `test_trials` greedy episodes, each begun with
   * environment start and agent start; reward and time keep adding up across them and the row holds their means.  0 and 1 = one episode.
   * Every kernel family has it (round 4: QV, advantage, the accumulating trace, target networks / safe too); not with taps. */
  int32_t  test_trials;
  int32_t  reserved0;
} grlx_config;

typedef struct grlx_ctx grlx_ctx;

/* per-step record of the tapped replica (debug / parity tests / transition log).  A record with
 * terminal = -1 (only with tap_starts) is the start of a trial: first observation and first action. */
typedef struct {
  int32_t  test, action_index, terminal, trace_len;
  double   obs[GRLX_MAX_DIMS];
  double   action, reward, delta;
  double   q[GRLX_MAX_ACTIONS];
  uint32_t p_idx[32];
  double   state[GRLX_MAX_STATE];     /* model state after this step (start record: the start state) */
} grlx_tap;

const char *grlx_last_error(void);
int  grlx_abi_version(void);
/* How the library was built: "device-asm+mir-exec-prologue-fix/2" when grl_amd/_build.py built it (the only supported
 * build: it passes the device code through the work-around for a register-allocation bug of ROCm 7.2's compiler,
 * DESIGN.md 4.1f), "" for a plain `hipcc -shared`, whose kernels may read stale lanes.  Bindings refuse the latter
 * (grl_amd/capi.py: load(); the reference-side addon: integration/addons/grlx). */
const char *grlx_build_pipeline(void);
int  grlx_device_count(void);

/* Fill *cfg with the values of the reference's tests/pendulum-sarsa-tc.yaml. */
void grlx_config_pendulum_sarsa(grlx_config *cfg);
/* Fill *cfg with the values of the reference's cfg/cart_pole/ac_tc.yaml (actor-critic, two tables). */
void grlx_config_cart_pole_ac(grlx_config *cfg);

/* Replaces: Configurator::instantiate of the experiment subtree (configurable.cpp:603-715)
 * for n_replicas deep clones (multi.cpp:49-59) after `srand48(seeds[r])`
 * (deployer.cpp:70-74).  RNG streams are consumed exactly in the reference's
 * YAML instantiate order; the 8,388,608-draw weight
 * initialisation (linear.cpp:110-121) is performed lazily per touched slot by
 * LCG jump-ahead and is bit-identical. */
int  grlx_create(const grlx_config *cfg, const int64_t *seeds, grlx_ctx **out);
int  grlx_destroy(grlx_ctx *ctx);

/* Replaces: OnlineLearningExperiment::run (online_learning.cpp:110-315) for every
 * replica: advance each by n_trials trials (learning and test trials both
 * count).  Asynchronous on `stream` (a hipStream_t passed as void*; NULL = default). */
int  grlx_run(grlx_ctx *ctx, int n_trials, void *stream);
/* Wait for the stream, then report sticky per-replica error flags (table full, ...). */
int  grlx_sync(grlx_ctx *ctx, void *stream);
/* Stream contract: grlx_run and grlx_curve_stats are asynchronous on the caller's stream.  Every entry point
 * that reads a context back to the host or works on its tables (grlx_rows, grlx_read_rows, grlx_read_row_times,
 * grlx_step_counts, grlx_get_*, grlx_table_load, grlx_export_weights, grlx_load_weights, grlx_read_taps,
 * grlx_read_diag, grlx_read / _write / _update) first waits for the stream of the context's last grlx_run,
 * so it never observes rollouts in flight -- also on a hipStreamNonBlocking stream. */

/* Test rows written so far (same for every replica). */
int  grlx_rows(grlx_ctx *ctx);
/* Replaces the per-replica `<output>-<run>@<i>.txt` rows (online_learning.cpp:238-262):
 * copy rows [first, first+count) of `replica` to host arrays (columns 1-3). */
int  grlx_read_rows(grlx_ctx *ctx, int replica, int first, int count,
                    int64_t *trial, int64_t *steps, double *reward);
/* column 4 of the same rows (online_learning.cpp:243 `total_time`): the sum of the tau returned by
 * Environment::step over the trial -- under discrete_time (modeled.cpp:209-212) the number of steps. */
int  grlx_read_row_times(grlx_ctx *ctx, int replica, int first, int count, double *episode_time);
/* Device-side learning-curve statistics over this GPU's replicas, written to a
 * DEVICE buffer out[count][3] = {sum reward, sum reward^2, replica count};
 * fixed reduction order (bitwise reproducible).  Input of the one RCCL
 * all-reduce of the multi-GPU path. */
int  grlx_curve_stats(grlx_ctx *ctx, int first, int count, double *out_dev, void *stream);

/* ... per group of group_size consecutive replicas: out[count][n_replicas / group_size][3], group q = the replicas
 * [q * group_size, (q + 1) * group_size) -- the repetitions of one point of a sweep.  Same fixed order (every thread strided over its
 * group, then the tree): with group_size == n_replicas the result equals grlx_curve_stats bit for bit.  n_replicas % group_size != 0
 * is GRLX_ERR_INVALID. */
int  grlx_curve_stats_grouped(grlx_ctx *ctx, int first, int count, int group_size, double *out_dev, void *stream);

/* --- hyper-parameter sweep: one context, a different configuration per replica -------------------------------------------------
 * The reference's study (bin/grlo over bin/optimize.yaml) varies predictor/alpha, predictor/gamma, predictor/lambda and
 * sampler/epsilon and runs every (point, repetition) as a process of its own; here they are the replicas of one context.
 * grlx_set_replica_params gives every replica its own value of ONE of the four (values[n_replicas]); parameters never set keep the
 * configuration's value for every replica, and grlx_get_replica_params returns what holds (before any set: the configuration's).
 * Allowed only between grlx_create and the first launch of the context (grlx_run, grlx_run_steps, a per-step call); persists
 * across grlx_reset_run.  Every replica's values are validated as grlx_create validates the shared ones (finite; with a replacing
 * trace gamma*lambda in (0,1) and its trace within the register trace's ten entries): a violation is GRLX_ERR_INVALID naming the
 * replica and the value, and nothing is applied.
 * The first set makes the context a SWEEP context.  Built for: SARSA / Q / Expected SARSA, a replacing trace or none, no target
 * network, safe = 0, no taps, no diagnostics, not GRLX_ENV_EXTERNAL, replicas_per_wave 0, 4 or 8 (the automatic choice then never
 * exceeds 8) -- otherwise GRLX_ERR_INVALID naming what is not built.  A sweep context runs the generic instantiation
 * (grlx_last_kernel: GRLX_KERNEL_GENERIC) without the environment server; grlx_agent_*, grlx_env_start / _advance and
 * grlx_set_diag(ctx, 1 | 2) return GRLX_ERR_INVALID on it, never a silent run on the shared values. */
enum { GRLX_PARAM_ALPHA = 0, GRLX_PARAM_GAMMA = 1, GRLX_PARAM_LAMBDA = 2, GRLX_PARAM_EPSILON = 3 };
int  grlx_set_replica_params(grlx_ctx *ctx, int param, const double *values /*[n_replicas]*/);
int  grlx_get_replica_params(grlx_ctx *ctx, int param, double *values /*[n_replicas]*/);

/* Which instantiation of the rollout kernel the last grlx_run launched (tests and benchmarks check that
 * the configuration they mean to measure takes the path they mean to measure). */
enum { GRLX_KERNEL_NONE = 0,          /* nothing launched yet                                                  */
       GRLX_KERNEL_GENERIC = 1,       /* parameters read at run time                                           */
       GRLX_KERNEL_SPECIALISED = 2,   /* compile-time instantiation of a reference yaml (pendulum tile-coding
                                         SARSA / Q / Expected SARSA, cart-pole actor-critic)                   */
       GRLX_KERNEL_IN_PLACE = 3       /* diagnostic instantiation: taps / stamps, TD update applied in place   */ };
int  grlx_last_kernel(grlx_ctx *ctx);
/* Replicas per wavefront of the context's rollout kernels (4 or 8): the layout chosen at create. */
int  grlx_replicas_per_wave(grlx_ctx *ctx);

/* counters: total env steps executed by all replicas since create */
int  grlx_step_counts(grlx_ctx *ctx, uint64_t *learn_steps, uint64_t *test_steps);

/* --- diagnostics: a separately compiled, stamped build of the rollout kernel
 * (s_memtime per phase).  Its run time is NOT representative; only the shares.
 * enable = 1: the instantiation that applies each TD update in place (the one
 * that also records taps); enable = 2: the production ordering (update applied
 * one pass later, under the next step's table loads; pendulum with 3 actions
 * only); 0: off. */
int  grlx_set_diag(grlx_ctx *ctx, int enable);
int  grlx_read_diag(grlx_ctx *ctx, uint64_t *out /*[waves][8] cycle sums*/, int cap_waves, int *n_waves);

/* --- state inspection (parity tests) ------------------------------------ */
int  grlx_get_env_state(grlx_ctx *ctx, int replica, double *state /*[GRLX_MAX_STATE]*/);
int  grlx_get_rng(grlx_ctx *ctx, int replica, uint64_t out[4] /* G, TL, S1, S2; a sampler stream the graph does not have (actor-critic: both) is 0 */);
/* Replaces reading LinearRepresentation::params_ (linear.cpp; .dat dump
 * representation.h:201-263): current weights of the given reference slots. */
int  grlx_get_weights(grlx_ctx *ctx, int table, int replica, const uint32_t *slots, int n, double *out);
int  grlx_table_load(grlx_ctx *ctx, int table, int replica, uint32_t *n_slots_used);
/* Current table size (log2 of the entries per replica and table), and explicit growth to 2^new_log2 (waits for the context's
 * work first; no-op if the tables are at least that large). */
int  grlx_table_capacity(grlx_ctx *ctx, uint32_t *log2_entries);
int  grlx_grow_tables(grlx_ctx *ctx, uint32_t new_log2);
/* The trial loop of OnlineLearningExperiment::run with BOTH of its bounds (online_learning.cpp:154: `(!trials_ || tt < trials_) &&
 * (!steps_ || ss < steps_)`): every replica runs at most max_trials further trials and starts none once its learning steps of the run
 * (since grlx_create / grlx_reset_run) have reached `steps` (> 0).  Replicas stop at trials of their own, so their rows are ragged:
 * grlx_replica_rows gives a replica's count, grlx_curve_stats counts per row.  One launch per call.  Every kernel family has it
 * (round 4); GRLX_ERR_INVALID with taps or diagnostics. */
int  grlx_run_steps(grlx_ctx *ctx, int max_trials, uint64_t steps, void *stream);
int  grlx_replica_rows(grlx_ctx *ctx, int replica);          /* rows replica `replica` has written (grlx_rows: replica 0) */
/* Experiment::reset() between two runs of `runs: N` (online_learning.cpp:307-308; Configurable::reset, configurable.h:770-776):
 * the representations' parameters are drawn again from the CONTINUING thread-local stream (linear.cpp:104-125), predictors clear
 * their traces (sarsa.cpp:60-66), epsilon-greedy and the action policy set decay_ = 1 (greedy.cpp:140-141, action.cpp:93-97); the
 * run's step / trial counters and rows start again; no stream is reseeded.  A target network draws again too, before its representation
 * (the walk visits the provided `target` object first: configurable.cpp:690-712, 754-757), and is synchronised from the two fresh vectors as
 * at construction; the claims of projector/tile_coding:safe are dropped (tile_coding.cpp:82-89). */
int  grlx_reset_run(grlx_ctx *ctx);
/* Replaces reading target()->params() (representation.h:266-282): the target network's current value of the given
 * reference slots of the Q table, and the number of synchronisations so far; contexts with target_interval > 0 only. */
int  grlx_get_target_weights(grlx_ctx *ctx, int replica, const uint32_t *slots, int n, double *out, uint32_t *n_syncs);
/* Replaces ParameterizedRepresentation's {action: load} (representation.h:231-263, driven by
 * experiment/online_learning:load_file, online_learning.cpp:140-150): setParams() with the raw
 * little-endian double[memory] image of a .dat file.  Every weight of `table` of the replicas
 * [first_replica, first_replica + n_replicas) becomes dense[slot]; RNG streams, environment state
 * and counters are untouched, as in the reference.  The image (count must equal the table's
 * memory, else GRLX_ERR_INVALID like the reference's "Configuration mismatch") is copied once to
 * the device and shared by those replicas; their sparse tables are cleared and re-created on
 * first touch from it.  Actor-critic contexts accept it only before the first grlx_run.  With a target network (table 0 of a context with
 * target_interval > 0) the load is followed by synchronize() as in the reference (representation.h:256-257): the target becomes
 * tau * image + (1 - tau) * target for EVERY slot -- one dense vector of `memory` doubles per replica on the device while tau != 0
 * (GRLX_ERR_OOM beyond 8 GiB of them). */
int  grlx_load_weights(grlx_ctx *ctx, int table, int first_replica, int n_replicas, const double *dense, uint64_t count);
/* Replaces ParameterizedRepresentation's {action: save} (representation.h:201-229): the DENSE
 * parameter vector double[memory] of one replica's table, little-endian as grl's .dat files hold it
 * (untouched slots carry their lazily computed initial value).  out: host buffer of `memory` doubles. */
int  grlx_export_weights(grlx_ctx *ctx, int table, int replica, double *out);

/* --- exact resume: a whole context as one byte string -------------------------------------------------------------------------
 * A snapshot holds everything a context carries from one launch to the next: the replicas' random streams, environment state,
 * exploration decay, trial / step counters, the rows written so far, the actor-critic's persisted critic trace, the occupied entries
 * of the sparse tables with their claim words and positions, the target network's values and synchronisation counts, the base of
 * the lazy initialisation, a sweep context's per-replica values -- and the grlx_config it was created with.  A context that loads
 * it and runs b trials gives the bits of the one that ran on for b trials: in another process, on another device of the same kind.
 * One self-describing little-endian byte string in the caller's host buffer (layout: grl_amd/csrc/grlx_snapshot_format.h); canonical:
 * two contexts in the same state give the same bytes.  No device pointer, nothing that lives inside one launch only.
 *
 * grlx_snapshot_size: waits for the context's work; the exact size of a snapshot taken now.
 * grlx_snapshot_save: waits likewise, writes the snapshot into buf[cap] (*written = its size; cap too small: GRLX_ERR_INVALID) and leaves
 *   the context exactly as it was.  NOT BUILT (GRLX_ERR_INVALID, "not built"): a context that holds a loaded policy (grlx_load_weights), one
 *   on which a per-step entry point has run, GRLX_ENV_EXTERNAL, taps or grlx_set_diag.
 * grlx_snapshot_load: allowed on a context that has launched nothing yet.  The context's configuration must equal the snapshot's except in
 *   replicas_per_wave, wave_limit, force_generic, table_log2_capacity, table_log2_max (layout and sizing: results do not depend on them) and
 *   the tap fields (a context with taps is refused); a difference elsewhere is GRLX_ERR_INVALID naming the field and both values.  The tables
 *   are re-allocated at the snapshot's capacity (beyond the context's table_log2_max: GRLX_ERR_INVALID; no memory: GRLX_ERR_OOM).  Everything
 *   is validated, and everything allocated, before the context is touched: a refused load leaves a context that runs as a fresh one.  After
 *   a successful load the context counts as launched (grlx_set_replica_params is refused); a snapshot of a sweep context makes it one.
 * grlx_snapshot_info: host only, needs no device: the header's fields and the configuration; `bytes` may cover the header alone. */
typedef struct {
  uint32_t format_version;
  uint32_t n_replicas, n_tables;
  uint32_t table_log2;                /* entries per replica and table = 2^this            */
  uint32_t is_sweep, has_trace, has_target, twin_tables;
  uint32_t rows;                      /* largest row count of a replica                    */
  uint32_t record_bytes;              /* one table record: 24, or 32 with a target network */
  int64_t  trials_run;
  uint64_t total_bytes, header_bytes;
  uint64_t n_records;                 /* occupied table entries, all tables and replicas   */
  uint64_t checksum;                  /* FNV-1a 64 over everything after the header        */
  uint64_t section_bytes[5];          /* states, rows, trace, sweep, records               */
  grlx_config config;
} grlx_snapshot_info_t;
int  grlx_snapshot_size(grlx_ctx *ctx, uint64_t *bytes);
int  grlx_snapshot_save(grlx_ctx *ctx, void *buf, uint64_t cap, uint64_t *written);
int  grlx_snapshot_load(grlx_ctx *ctx, const void *buf, uint64_t bytes);
int  grlx_snapshot_info(const void *buf, uint64_t bytes, grlx_snapshot_info_t *out);

int  grlx_read_taps(grlx_ctx *ctx, grlx_tap *out, int cap, int *n);

/* --- fine-grained batched operators (host pointers; each call copies in, runs a
 *     HIP kernel, copies out).  They mirror the plug-in interfaces one to one. */

/* Projector::project -> TileCodingProjector::_project (tile_coding.cpp:103-149):
 * in[n][dims] -> out[n][tilings] reference slot indices.  A coordinate that is not finite, or whose |x * tilings / resolution|
 * reaches 2^30 (the quantisation casts its floor to int), is refused with GRLX_ERR_INVALID naming row and dimension, as the
 * queries refuse it; nothing is written then. */
int  grlx_project(const grlx_tile_spec *spec, const double *in, int n, uint32_t *out);

/* Environment::step -> ModeledEnvironment::step (modeled.cpp:160-213):
 * state[n][S] updated in place; obs[n][D], reward[n], terminal[n]. */
int  grlx_env_step(const grlx_config *cfg, double *state, const double *action, int n,
                   double *obs, double *reward, int32_t *terminal);
int  grlx_env_dims(int env, int *state_dims, int *obs_dims);

/* Representation::read / write / update on a context's table
 * (linear.cpp:136-184, 186-196, 198-216): idx[n][tilings] reference slots,
 * replica[n] selects the table instance.  Rows are applied in order. */
int  grlx_read(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n, double *out);
int  grlx_write(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n,
                const double *target, double alpha);
int  grlx_update(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n,
                 const double *delta);

/* --- policy queries: what the replicas have learned at observations of the caller's choice ------------------------------------
 * The read side of the policies (the reference's value / policy field plots and mapping/policy/<...> are built on it), for the replicas
 * [first_replica, first_replica + n_replicas) at obs[n_obs][obs_dims]; obs_dims = the projector's input dimensions, minus the action's
 * for the Q agents (GRLX_ENV_EXTERNAL included).  Host pointers; each call waits for the stream of the context's last grlx_run, copies
 * in, runs HIP kernels and copies out, in chunks of observations so that no call holds more than 256 MiB of device scratch (results do
 * not depend on the chunking).
 * A QUERY CHANGES NOTHING: no table entry is created (grlx_read creates the entries it reads; these do not) -- a slot never touched
 * contributes the value the reference's dense initialisation gave it, or a loaded image's (grlx_load_weights); table occupancy, random
 * streams, traces, per-step agent state and the target network are untouched, a snapshot taken after a query holds the bytes of one
 * taken before.  A query before the first launch is allowed and does not count as one (grlx_set_replica_params and grlx_snapshot_load
 * stay allowed).  The MAIN parameters are read, never a target network's (q.cpp:106 reads representation_; the target's values stay
 * behind grlx_get_target_weights).
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written): null obs, n_obs < 0, a replica range outside
 * the context, an observation that is not finite or whose |x * scaling[i]| reaches 2^30 (TileCodingProjector casts to int,
 * tile_coding.cpp:121-125) -- the message names row and dimension.  n_obs == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * NOT BUILT (GRLX_ERR_INVALID, "not built"): projector/tile_coding:safe >= 1 (a read would have to walk the claim table without
 * claiming). */

/* Replaces QPolicy::values (q.cpp:94-107), QPolicy::value (q.cpp:56-68) and QPolicy::act(in, out) const (q.cpp:129-141) under the
 * greedy sampler, for agents with a policy/discrete/q (SARSA, Q, Expected SARSA, advantage, QV: its table 0); 3 or 5 actions.
 *   q[n_replicas][n_obs][action_steps]   representation_->read(project(obs, action a)): ((w0 + w1) + ... + w15) / 16, clamped to
 *                                        output_min / output_max (linear.cpp:136-184)
 *   greedy, n_max [n_replicas][n_obs]    mai and man of GreedySampler::findmax (greedy.cpp:47-61): the first maximum and the number
 *                                        of maxima.  No random draw: a tie is reported, not broken.
 *   value[n_replicas][n_obs]             v = 0; for every action in order: v += q[a] * dist[a], dist[a] = 1. / man at the maxima and 0
 *                                        elsewhere (q.cpp:56-68 over GreedySampler::distribution, greedy.cpp:88-98)
 * Any output may be NULL. */
int  grlx_query_q(grlx_ctx *ctx, int first_replica, int n_replicas, const double *obs /*[n_obs][obs_dims]*/, int n_obs,
                  double *q, double *value, int32_t *greedy, int32_t *n_max);
/* The read of a table whose projector takes the observation alone: out[n_replicas][n_obs].  Actor-critic: table 0 = the critic's V(s),
 * table 1 = ActionPolicy::read (action.cpp:99-112) -- the greedy action of ActionPolicy::act(in, out) const (action.cpp:160-...) is
 * fmin(fmax(out, action_min), action_max).  QV: table 1 = V(s) (qv.cpp:74-108).  Table 0 of a Q agent takes (observation, action):
 * refused, use grlx_query_q. */
int  grlx_query_state(grlx_ctx *ctx, int table, int first_replica, int n_replicas, const double *obs, int n_obs, double *out);
/* Q agents: grlx_query_q reduced on the device per group of group_size consecutive replicas (the repetitions of one point of a sweep,
 * as in grlx_curve_stats_grouped) and per observation to raw sums: out[n_replicas / group_size][n_obs][2 + 2 * action_steps] =
 * { sum value, sum value * value, sum q[0 .. A), votes[0 .. A) }, votes[a] = the number of replicas whose greedy is a (as a double).
 * Every sum runs over the group's replicas in ascending order into one accumulator (no tree): that order is the specification.
 * n_replicas % group_size != 0 is GRLX_ERR_INVALID. */
int  grlx_query_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, const double *obs, int n_obs, double *out);

/* --- policy evaluation: greedy episodes from start states of the caller's choice -------------------------------------------------
 * For every (replica, start state) pair one episode of the TEST agent (agent/fixed over the learned tables) on the replica's current
 * parameters, from that model state to its end, on the device, in one launch: the test branch of OnlineLearningExperiment::run
 * (online_learning.cpp:172-213) for one episode with states[s] in place of Task::start.  Replicas [first_replica, first_replica +
 * n_replicas); states[n_starts][state_dims], state_dims the MODEL's (grlx_env_dims: pendulum 3, cart-pole and acrobot 5, walker 11).
 * The state carries the time, and the walker's its timeout and step flag, so a state from grlx_get_env_state or a tap continues exactly.
 *   The loop.   Observe the start state -- its terminal code is ignored, as the reference's start ignores it: an episode has at least
 *               one step -- then act, step, add the reward, until the step's terminal code is non-zero or max_steps steps have run.
 *   The action. Q agents (SARSA, Q, Expected SARSA, advantage, QV's table 0; accumulating trace and target network included: the MAIN
 *               parameters are read, as by the queries): actions[mai], mai the FIRST maximum of GreedySampler::findmax (greedy.cpp:
 *               47-61).  No random draw is made; `ties` counts the steps at which there was more than one maximum.  With ties == 0
 *               the episode is the reference's test episode from that state, bit for bit.  Actor-critic: fmin(fmax(read(actor table,
 *               obs), action_min), action_max) (ActionPolicy::act(in, out) const); ties = 0.
 *   ret         ret = 0; ret += reward in step order (online_learning.cpp:202)
 *   disc        g = 1; disc = 0; per step disc += g * reward; g = g * gamma (plain products; the replica's own gamma in a sweep context)
 *   steps       steps taken
 *   terminal    1 timed out, 2 absorbing, 0 cut at max_steps, 3 the step ended outside the portable math's domain (what the rollout
 *               kernels flag and grlx_sync reports as GRLX_ERR_DOMAIN: the step is counted, the episode stops there, no sticky flag is set)
 *   final_state [n_replicas][n_starts][state_dims] the model state after the last step
 * ret, disc, steps, terminal, ties: [n_replicas][n_starts].  Host pointers; any output may be NULL.
 * max_steps: 1 ... GRLX_MAX_EPISODE_STEPS, 0 = that cap.  The kernel never iterates further, whatever time or timeout the state carries.
 * AN EVALUATION CHANGES NOTHING in the context, like a query (above): tables, streams, counters, rows, the environment states and the
 * sticky status are untouched; it is allowed before the first launch and does not count as one; it waits for the stream of the last
 * grlx_run and stages in chunks of start states under the queries' bound (grlx_set_query_chunk_bytes).
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written; row and component named): null states,
 * n_starts < 0, the replica range, max_steps out of range, a state component that is not finite or reaches 2^17 in magnitude (below it
 * the RK4 stages of a step stay inside the branch-free sine's domain at the rates the tasks reach; a hand-made RATE near the bound can
 * still carry an angle out within one step -- the acrobot's does -- which ends the episode with code 3 after that step, its sums and
 * final state then being those of sines taken outside their domain), GRLX_ENV_EXTERNAL (no environment), projector/tile_coding:safe >= 1
 * ("not built"), an (environment, action count) pair without an instantiation (built: pendulum x {3, 5} actions, acrobot, cart-pole and
 * walker x 3; actor-critic: cart-pole and pendulum).  n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * The steps of these episodes: grlx_evaluate_trajectory (below).  The batch path's episodes: grlx_fqi_evaluate (at the end of this file).
 * The samplers -- the drawn tie break, the epsilon-greedy learning policy --: grlx_evaluate_sampled (below).
 * NOT BUILT: acting on the target network. */
int  grlx_evaluate(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/, int n_starts,
                   int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state);

/* --- ensemble evaluation: greedy episodes on a group's vote or mean Q --------------------------------------------------------------
 * Q agents.  The replicas [first_replica, first_replica + n_replicas) form n_replicas / group_size groups of group_size CONSECUTIVE
 * replicas (the repetitions of one point of a sweep, as in grlx_query_ensemble and grlx_curve_stats_grouped).  For every (group, start
 * state) pair one episode, on the device, in one launch: grlx_evaluate's loop -- the ignored terminal code of the start state, the
 * terminal codes 0 / 1 / 2 / 3, max_steps (0 = GRLX_MAX_EPISODE_STEPS), the 2^17 bound on state components -- in which the members of
 * the group share ONE environment state.  Reference: mapping/policy/discrete/multi (multi_discrete.cpp:120-235).
 *   The action at observation o.  Over the members m in ASCENDING replica order: q_m[a], mai_m, man_m exactly as grlx_query_q defines
 *               them (main parameters, peek only, initial_weight for a slot without an entry); votes[a] = the number of members with
 *               mai_m == a; sumq[a] = one accumulator per action from 0.0 with += q_m[a] in that order (the bits of
 *               grlx_query_ensemble's sum q column).  score = votes (GRLX_ENSEMBLE_VOTE) or sumq (GRLX_ENSEMBLE_MEAN_Q);
 *               (mai, man) = findmax(score), the first maximum and the number of maxima; the action is actions[mai].  No random draw.
 *   ties        += (man > 1) per step: the combined score had more than one maximum
 *   member_ties += the number of members with man_m > 1, per step
 *   agreement   += votes[mai] per step, under either rule: agreement / (steps * group_size) is the share of members that would have
 *               taken the step the ensemble took
 *   ret, disc, steps, terminal, final_state   as grlx_evaluate's.  disc uses the gamma of the group's FIRST replica: in a sweep context
 *               a group is one point's repetitions, which share it.
 * ret, disc, steps, terminal, ties, member_ties, agreement: [n_replicas / group_size][n_starts]; final_state has [state_dims] more.
 * Host pointers; any output may be NULL.  group_size == 1 is grlx_evaluate (member_ties = its ties).
 * Deviations from the reference.  Its member "best" is the first strictly greater entry of the member's distribution
 * (multi_discrete.cpp), which under the greedy sampler is mai_m.  It then SAMPLES from softmax(votes); this entry point acts on the
 * first maximum and reports ties, as grlx_evaluate does for a single policy.  GRLX_ENSEMBLE_MEAN_Q is not one of the reference's
 * discrete strategies (its add_prob adds the members' greedy distributions): it is the argmax of grlx_query_ensemble's mean Q.
 * An evaluation changes nothing in the context, waits for the stream of the last grlx_run, does not count as a launch and stages in
 * chunks of start states under grlx_set_query_chunk_bytes' bound, like grlx_evaluate.
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the reason named): everything grlx_evaluate
 * refuses, group_size < 1, n_replicas % group_size != 0, an unknown rule, an actor-critic context ("not built": a vote over
 * continuous actions is mapping/policy/multi's).  n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * The steps of these episodes: grlx_evaluate_ensemble_trajectory (below).
 * The batch path's: grlx_fqi_evaluate_ensemble (at the end of this file).
 * NOT BUILT: the reference's other discrete strategies (multiply, rank voting, density based), sampling from the combined
 * distribution. */
enum { GRLX_ENSEMBLE_VOTE = 0, GRLX_ENSEMBLE_MEAN_Q = 1 };
int  grlx_evaluate_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule,
                            const double *states /*[n_starts][state_dims]*/, int n_starts, int max_steps,
                            double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                            int64_t *member_ties, int64_t *agreement, double *final_state);

/* --- per-step trajectories of the evaluation episodes ----------------------------------------------------------------------------------
 * grlx_evaluate and grlx_evaluate_ensemble with one more output: every step of every episode.  The episodes, the sums and every rule
 * above are the sibling's, bit for bit; kernels of their own write, per step taken, one record of R doubles:
 *   records[pair][max_steps][R], pair = (replica - first_replica) * n_starts + start (ensemble: group * n_starts + start), record t = the
 *   pair's step t from 0.  R = grlx_trajectory_record_words(ctx, ensemble) = 6 + D + S (ensemble: 8 + D + S), D / S the environment's
 *   observation / model state dimensions (grlx_env_dims): 11, 15, 15, 22 (13, 17, 17, 24) for pendulum, acrobot, cart-pole, walker.
 * Small integers are stored as doubles, exactly.  The words of a record:
 *   GRLX_TRAJ_ACTION        the value handed to the environment
 *   GRLX_TRAJ_REWARD        the step's reward; added up in step order it is ret
 *   GRLX_TRAJ_VALUE         Q agents: Q(obs, chosen action) after the representation's clamp, grlx_query_q's `value` at that observation.
 *                           Actor-critic: the actor's read after the representation's clamp and BEFORE the action clip, what
 *                           grlx_query_state(table 1) returns there.  Ensemble: the combined score of the action taken, votes[mai] as a
 *                           double (GRLX_ENSEMBLE_VOTE) or sumq[mai], the sum and not the mean (GRLX_ENSEMBLE_MEAN_Q)
 *   GRLX_TRAJ_ACTION_INDEX  mai (the ensemble: of the combined score); -1 for the actor-critic
 *   GRLX_TRAJ_N_MAX         man, the number of maxima; 1 for the actor-critic
 *   GRLX_TRAJ_TERMINAL      the episode's code AFTER this step: 0 while it goes on and in the last record of an episode cut at max_steps,
 *                           else 1 / 2 / 3 as grlx_evaluate defines them
 *   ensemble only:  GRLX_TRAJ_ENS_AGREEMENT  votes[mai] of this step, under either rule;  GRLX_TRAJ_ENS_MEMBER_TIES  the members with
 *                   man_m > 1 at this step.  Summed over an episode's records they are agreement and member_ties.
 *   GRLX_TRAJ_OBS (ensemble: GRLX_TRAJ_ENS_OBS) ... + D   the observation the policy ACTED ON, i.e. before the step
 *   ... + D ... R           the MODEL state AFTER the step, time included: the last record's is final_state; the start state is the caller's
 * Records at index >= the pair's steps are all-zero bits (+0.0).
 * max_steps: 1 ... GRLX_MAX_EPISODE_STEPS.  It sizes the caller's buffer, so 0 is refused here.  records must not be NULL (without it, call
 * the sibling); the other outputs may be.  Staged in chunks of start states under grlx_set_query_chunk_bytes' bound, records included:
 * a chunk never exceeds the bound, so a single start state's column -- n_replicas (ensemble: groups) * max_steps * R * 8 bytes of records
 * and its sums -- that does not fit is refused, with the remedies named (fewer replicas per call, a smaller max_steps, a larger bound).
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the reason named): everything the sibling
 * refuses, and the three cases above.  Like the siblings they change nothing in the context, wait for the stream of the last grlx_run
 * and do not count as a launch.  The batch path's: grlx_fqi_evaluate_trajectory (at the end of this file), with the same words.
 * Trajectories of the samplers' episodes: grlx_evaluate_sampled_trajectory (below).
 * The same result chunk by chunk, without one array for all of it: grlx_evaluate_trajectory_stream (below). */
enum { GRLX_TRAJ_ACTION = 0, GRLX_TRAJ_REWARD = 1, GRLX_TRAJ_VALUE = 2, GRLX_TRAJ_ACTION_INDEX = 3, GRLX_TRAJ_N_MAX = 4, GRLX_TRAJ_TERMINAL = 5,
       GRLX_TRAJ_OBS = 6, GRLX_TRAJ_ENS_AGREEMENT = 6, GRLX_TRAJ_ENS_MEMBER_TIES = 7, GRLX_TRAJ_ENS_OBS = 8 };
int  grlx_trajectory_record_words(grlx_ctx *ctx, int ensemble);      /* R; a negative status for a context without such episodes */
int  grlx_evaluate_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/, int n_starts,
                              int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state,
                              double *records /*[n_replicas][n_starts][max_steps][R]*/);
int  grlx_evaluate_ensemble_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule,
                                       const double *states /*[n_starts][state_dims]*/, int n_starts, int max_steps,
                                       double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                       int64_t *member_ties, int64_t *agreement, double *final_state,
                                       double *records /*[n_replicas / group_size][n_starts][max_steps][R]*/);

/* --- streamed trajectories: grlx_evaluate_trajectory's result handed to a callback chunk by chunk ---------------------------------------
 * The episodes, the record words and the sums are grlx_evaluate_trajectory's, bit for bit, for the same agents and contexts; the caller
 * never holds more than one chunk.  The start states are cut into chunks of consecutive ones; for each chunk, in ascending order, the
 * sink is called once with the chunk's arrays:
 *   first_start, n_starts   the chunk covers start states first_start ... first_start + n_starts - 1 of the call; the chunks are
 *                           contiguous, do not overlap and together cover 0 ... n_starts - 1
 *   rows                    n_replicas;  max_steps, record_words (R), state_dims (S): the call's
 *   ret, disc, steps, terminal, ties   [rows][n_starts], element (row, s) at row * n_starts + s -- the CHUNK's n_starts
 *   final_state             [rows][n_starts][state_dims];   records  [rows][n_starts][max_steps][record_words]
 * Records behind an episode's end are +0.0.  The pointers lead into page-locked staging memory of the context and are valid only until
 * the sink returns.  The sink runs on the calling thread, never concurrently with itself; while it runs, the next chunk's kernel and copy
 * are in flight.  The call returns after the last sink call, with nothing in flight.  Nothing in the context changes; like its sibling
 * the call waits for the stream of the last grlx_run and does not count as a launch.
 * Staging: two chunks are staged at a time and share grlx_set_query_chunk_bytes' bound, so a chunk holds the start states whose columns
 * (records, sums, state) fit HALF the bound, and the call never holds more than the bound on the device, nor more than the bound in
 * page-locked host memory.  The staging belongs to the context: allocated at the first streamed call, grown when a later call needs
 * more, released by grlx_destroy.
 * Stopping: a nonzero return of the sink ends the stream -- no further chunk is delivered, nothing more is enqueued, what is in flight
 * is waited for -- and the call returns GRLX_ERR_STOPPED with the sink's value in the message.  After a HIP error the call likewise
 * enqueues nothing more, waits, and returns GRLX_ERR_HIP.
 * Validated on the host before anything is launched or allocated (GRLX_ERR_INVALID, the sink is not called, the reason and this
 * function named): everything grlx_evaluate_trajectory refuses; sink == NULL; max_steps == 0; a single start state's column that exceeds
 * half the staging bound (the bytes, the half bound and the remedies named).  n_starts == 0 or n_replicas == 0: GRLX_OK, no sink call.
 * Calls from inside the sink.  While the streamed call has not returned, the context serves no other call: GRLX_ERR_INVALID, "a streamed
 * call is in progress".  Checked: grlx_run, grlx_run_steps, grlx_reset_run, grlx_snapshot_load, grlx_destroy, grlx_load_weights,
 * grlx_set_replica_params, grlx_set_diag, a nested grlx_evaluate_trajectory_stream, and every call that waits for the last grlx_run before
 * it touches the context's device memory -- which is every other call that reads or writes it (the queries and evaluations, the reads
 * named grlx_get_..., grlx_read_... and grlx_export_..., grlx_snapshot_size and _save, grlx_grow_tables, grlx_read, _write and _update,
 * the per-step entry points).  So read-only calls on the SAME context are NOT allowed from inside the sink either; calls that take no context (grlx_project,
 * grlx_env_step, grlx_math ...) and calls on another context are.
 * NOT BUILT: the ensemble, sampled, noisy and batch-path trajectories as streams; a file-descriptor sink (the callback is the primitive). */
typedef struct grlx_trajectory_chunk {
  int32_t struct_size;
  int32_t first_start, n_starts;
  int32_t rows, max_steps, record_words, state_dims;
  const double *ret, *disc;
  const int32_t *steps, *terminal, *ties;
  const double *final_state;
  const double *records;
} grlx_trajectory_chunk;
typedef int (*grlx_trajectory_sink)(void *user, const grlx_trajectory_chunk *chunk);
int  grlx_evaluate_trajectory_stream(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/, int n_starts,
                                     int max_steps, grlx_trajectory_sink sink, void *user);

/* --- sampled evaluation: the episodes of grlx_evaluate acted by the reference's samplers ------------------------------------------------
 * Q agents.  For every (replica, start state) pair one episode, on the device, in one launch: grlx_evaluate's loop, unchanged -- the
 * ignored terminal code of the start state, the terminal codes 0 / 1 / 2 / 3, max_steps (0 = GRLX_MAX_EPISODE_STEPS; the trajectory call
 * refuses 0), the 2^17 bound on state components, ret, disc (the replica's own gamma in a sweep context) and final_state as there, on
 * grlx_query_q's Q-values (main parameters, peek only, initial_weight for a slot without an entry) -- in which the action index comes
 * from a SAMPLER (greedy.cpp:63-86, 144-218) instead of the first maximum.  Nothing in the context changes; the call waits for the stream
 * of the last grlx_run, does not count as a launch and stages in chunks of start states under grlx_set_query_chunk_bytes' bound.
 *   Streams.    Every episode carries two 48-bit rand48 states, streams[n_replicas][n_starts][2]:
 *               [..][0] the sampler's private stream (the role of the learning policy's sampler stream: the epsilon draw),
 *               [..][1] the global stream (the random action index and the tie break).
 *               streams == NULL: every episode of replica r starts from COPIES of that replica's sampler stream and global stream
 *               as they stand (grlx_get_rng's words 2 and 0); the context's own streams do not move.
 *               streams_out[n_replicas][n_starts][2] receives both states after the episode's last step; it may be NULL.
 *               grlx_episode_streams (below) makes disjoint streams from one seed.
 *   A step.     (mai, man) = GreedySampler::findmax(Q(obs, .)); then, in exactly the order of draws of the rollout kernels' sampler:
 *               GRLX_SAMPLER_GREEDY          man > 1: the global stream advances, jj = lrand48 % man, the (jj + 1)-th maximal entry acts
 *                                            and ties++; else mai acts and no draw is made.  epsilon is ignored but must be valid.
 *               GRLX_SAMPLER_EPSILON_GREEDY  the sampler's stream advances, rnd = drand48; rnd < e: the global stream advances,
 *                                            lrand48 % action_steps acts and explored++; else as the greedy sampler.
 *               e is `epsilon` for every replica, or with GRLX_EPSILON_OWN the product eps_decay * epsilon as the rollout kernels form
 *               it: the replica's current decay (EpsilonGreedySampler::decay_) times the configuration's epsilon, in a sweep context
 *               that replica's own.  THE ONE DEVIATION: the decay is never advanced -- the reference decays once more at episode time 0
 *               -- which is the price of changing nothing in the context.
 *   ties        steps at which a tie break was DRAWN (man > 1 on a step that did not explore)
 *   explored    steps at which the action was the random draw
 * ret, disc, steps, terminal, ties, explored: [n_replicas][n_starts]; final_state has [state_dims] more.  Host pointers; any output may be NULL.
 * Consequences.  With GRLX_SAMPLER_GREEDY and the replica's own streams (streams == NULL) an episode from the task's test start state is
 * the reference's next test episode, bit for bit, WITH OR WITHOUT TIES.  With ties == 0 under GRLX_SAMPLER_GREEDY every output equals
 * grlx_evaluate's and streams_out == streams.
 *   Records.    grlx_evaluate_sampled_trajectory: records[pair][max_steps][R], R = grlx_sampled_trajectory_record_words(ctx) =
 *               grlx_trajectory_record_words(ctx, 0) + 1.  Every word of grlx_evaluate_trajectory keeps its index:
 *               GRLX_TRAJ_ACTION_INDEX is the index that ACTED, GRLX_TRAJ_N_MAX is man, GRLX_TRAJ_VALUE is Q of the action taken; the new
 *               last word GRLX_TRAJ_SAMPLED_EXPLORED = R - 1 is 1.0 where the action was the random draw, else 0.0.  Records behind an
 *               episode's end are zeros.  The staging rule and its refusal (a start state's column that exceeds the bound) are the sibling's.
 * Agents: everything grlx_evaluate accepts as a Q agent -- SARSA, Q, Expected SARSA, advantage learning, QV's table 0, an accumulating
 * trace, a context with a target network (the main parameters are read), the five (environment, actions) pairs that are built.
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the reason and the function named): everything
 * grlx_evaluate refuses; an unknown sampler; epsilon that is not finite; epsilon outside [0, 1] that is not exactly GRLX_EPSILON_OWN;
 * a stream word >= 2^48 (row and word named); the actor-critic ("not built": its Gaussian / Ornstein-Uhlenbeck exploration needs the
 * policy's noise state, which grlx_evaluate_noisy below carries).  n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * NOT BUILT: a sampled ensemble (softmax(votes)), the tie-breaking draw of grlx_fqi_evaluate, the
 * decay at episode time 0. */
enum { GRLX_SAMPLER_GREEDY = 0, GRLX_SAMPLER_EPSILON_GREEDY = 1 };
#define GRLX_EPSILON_OWN (-1.0)
int  grlx_evaluate_sampled(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/, int n_starts,
                           int max_steps, int sampler, double epsilon, const uint64_t *streams /*[n_replicas][n_starts][2] or NULL*/,
                           double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int32_t *explored,
                           double *final_state, uint64_t *streams_out /*[n_replicas][n_starts][2]*/);
int  grlx_sampled_trajectory_record_words(grlx_ctx *ctx);      /* R = grlx_trajectory_record_words(ctx, 0) + 1; a negative status otherwise */
int  grlx_evaluate_sampled_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/,
                                      int n_starts, int max_steps, int sampler, double epsilon,
                                      const uint64_t *streams /*[n_replicas][n_starts][2] or NULL*/, double *ret, double *disc,
                                      int32_t *steps, int32_t *terminal, int32_t *ties, int32_t *explored, double *final_state,
                                      uint64_t *streams_out /*[n_replicas][n_starts][2]*/,
                                      double *records /*[n_replicas][n_starts][max_steps][R]*/);
/* Host only, no context: out[n_pairs][2], the streams of the pairs first_pair ... first_pair + n_pairs - 1.  Stream k = 2 * pair + which
 * is srand48(seed) advanced by k * 2^20 draws.  An episode draws at most one value per stream and step and 2^20 exceeds
 * GRLX_MAX_EPISODE_STEPS, so the streams of different episodes are disjoint.  first_pair < 0 or out == NULL: nothing is written. */
void grlx_episode_streams(long seed, int64_t first_pair, int64_t n_pairs, uint64_t *out /*[n_pairs][2]*/);

/* Noisy evaluation episodes: grlx_evaluate's episodes of the ACTOR-CRITIC acted by the policy that collects its data instead of the
 * noise-free actor -- ActionPolicy::act(time, in, out) (action.cpp:127-158): the actor's read plus Gaussian or Ornstein-Uhlenbeck noise
 * drawn by Box-Muller (Rand::getNormal, utils.h:120-125), clipped to the action range.  For every (replica, start state) pair one episode,
 * on the device, in one launch per chunk; the loop, terminal, max_steps, the replica range, the staging and "changes nothing" are
 * grlx_evaluate's.  What it answers: the return the learning policy gives up to its exploration at a sigma, how robust a learned actor is
 * to action noise, a sweep over sigma from fixed start states without retraining.
 *   State.      Every episode carries ONE rand48 state (the role of the thread-local stream) and ONE double (the noise state,
 *               ActionPolicy::n_) in and out.  streams[n_replicas][n_starts] / noise[n_replicas][n_starts].
 *               streams == NULL: every episode of replica r starts from a COPY of that replica's thread-local stream as it stands
 *               (grlx_get_rng's word 1); the context's own stream does not move.  noise == NULL: 0.0 for every episode.
 *               streams_out / noise_out [n_replicas][n_starts] receive both after the episode's last step; either may be NULL.
 *               grlx_episode_stream_words (below) makes disjoint streams from one seed: an episode draws two values per step and
 *               2^20 exceeds 2 * GRLX_MAX_EPISODE_STEPS.
 *   A step.     u = the actor's read at the observation, clamped to the actor representation's output range (grlx_evaluate's).  If the
 *               model time of the state acted on is 0, noise = 0.  If sg != 0: U1 = drand48, U2 = drand48 of the episode's stream,
 *               nrm = sqrt(-2 * log(U1)) * cos(2 * pi * U2) * sg + 0, noise = (1 - theta) * noise + nrm, out = u + noise -- the
 *               operations and their order are the rollout kernels', on the portable log and cos; otherwise out = u, nothing is drawn
 *               and the noise state stays.  action = fmin(fmax(out, action_min), action_max); clipped++ where out lay outside.
 *   sg          `sigma` (>= 0) for every replica, or with GRLX_SIGMA_OWN the product ac_decay * sigma as the rollout kernels form it:
 *               the replica's current decay (ActionPolicy::decay_) times the configuration's sigma.  THE ONE DEVIATION, as under
 *               GRLX_EPSILON_OWN: the decay is never advanced -- the reference decays once more at episode time 0.
 *   theta       the caller's, in [0, 1] (1: independent Gaussian noise, 0: a running sum), or with GRLX_THETA_OWN the configuration's.
 *   clipped     steps whose noisy action lay outside [action_min, action_max]
 * ret, disc, steps, terminal, clipped: [n_replicas][n_starts]; final_state has [state_dims] more.  Host pointers; any output may be NULL.
 * Consequences.  With sigma == 0 every output equals grlx_evaluate's, streams_out == streams and noise_out == noise wherever the start
 * state's time is not 0.
 *   Records.    grlx_evaluate_noisy_trajectory: records[pair][max_steps][R], R = grlx_noisy_trajectory_record_words(ctx) =
 *               grlx_trajectory_record_words(ctx, 0) + 2.  Every word of grlx_evaluate_trajectory's actor-critic record keeps its index:
 *               GRLX_TRAJ_ACTION is the action that ACTED (noisy, clipped), GRLX_TRAJ_VALUE the actor's read before noise and clip; the
 *               two new last words are the noise state after the step (R - 2) and 1.0 where the step clipped (R - 1).  Records behind an
 *               episode's end are zeros.  The staging rule and its refusal are the sibling's.
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the reason and the function named): everything
 * grlx_evaluate refuses; a Q agent ("actor-critic only": grlx_evaluate_sampled serves those); sigma that is not finite, or negative and
 * not exactly GRLX_SIGMA_OWN; theta that is not finite, or outside [0, 1] and not exactly GRLX_THETA_OWN; a stream word >= 2^48 (row
 * named); a noise entry that is not finite (row named); for the trajectory call max_steps == 0 and a column beyond the staging bound.
 * n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * NOT BUILT: noise for the Q agents, a noisy actor-critic ensemble, the decay at episode time 0, per-dimension sigma / theta (actions
 * here are one-dimensional). */
#define GRLX_SIGMA_OWN (-1.0)
#define GRLX_THETA_OWN (-1.0)
int  grlx_evaluate_noisy(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/, int n_starts,
                         int max_steps, double sigma, double theta, const uint64_t *streams /*[n_replicas][n_starts] or NULL*/,
                         const double *noise /*[n_replicas][n_starts] or NULL*/, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                         int32_t *clipped, double *final_state, uint64_t *streams_out /*[n_replicas][n_starts]*/,
                         double *noise_out /*[n_replicas][n_starts]*/);
int  grlx_noisy_trajectory_record_words(grlx_ctx *ctx);        /* R = grlx_trajectory_record_words(ctx, 0) + 2; a negative status otherwise */
int  grlx_evaluate_noisy_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][state_dims]*/,
                                    int n_starts, int max_steps, double sigma, double theta,
                                    const uint64_t *streams /*[n_replicas][n_starts] or NULL*/,
                                    const double *noise /*[n_replicas][n_starts] or NULL*/, double *ret, double *disc, int32_t *steps,
                                    int32_t *terminal, int32_t *clipped, double *final_state, uint64_t *streams_out, double *noise_out,
                                    double *records /*[n_replicas][n_starts][max_steps][R]*/);
/* Host only, no context: out[n_pairs], the EVEN streams of grlx_episode_streams -- stream 2 * pair of the seed, srand48(seed) advanced
 * by pair * 2^21 draws -- one per pair, for calls whose episodes carry one stream.  first_pair < 0 or out == NULL: nothing is written. */
void grlx_episode_stream_words(long seed, int64_t first_pair, int64_t n_pairs, uint64_t *out /*[n_pairs]*/);

/* --- actor-critic ensembles: episodes on the members' combined action ------------------------------------------------------------------
 * The ACTOR-CRITIC's counterpart of grlx_evaluate_ensemble.  One episode runs per (group, start state): a group is group_size CONSECUTIVE
 * replicas of [first_replica, first_replica + n_replicas) sharing ONE environment state.  Grouping, the pair index group * n_starts +
 * start, the staging in chunks, max_steps (0 = GRLX_MAX_EPISODE_STEPS), the terminal codes 0 / 1 / 2 / 3, ret, disc and final_state are
 * exactly grlx_evaluate_ensemble's; disc uses the context's gamma (an actor-critic context has no sweep).  Reference:
 * mapping/policy/multi (base/src/policies/multi.cpp), which combines the continuous actions of several policies.
 *   At every step, for the members m in ASCENDING replica order, a_m is the action grlx_evaluate would hand the environment for that
 *   replica at this observation: the actor's read after the representation's clamp, then clipped to [action_min, action_max]; noise-free,
 *   ActionPolicy::act(in, out) with sigma 0.  The rule combines a_0 ... a_{G-1} into the action that acts.  No clip follows the
 *   combination (the reference has none, and the task's actuate does its own).  No random draw is made anywhere: where the reference
 *   draws rand() among tied candidates, the FIRST acts and `ties` counts the step.  lo / hi are the context's action_min / action_max.
 * GRLX_ACTOR_ENSEMBLE_MEAN (csMean, multi.cpp:507-523):
 *   m = a_0; m = m + a_i for i = 1 ... G-1; action = m / (double)G.
 * GRLX_ACTOR_ENSEMBLE_BINNING (csBinning, :126-181), parameter `bins` B with 1 <= B <= 64:
 *   bin(a) = min((int)floor(((double)B * (a - lo)) / (hi - lo)), B - 1).  Build the histogram of the members' bins.  binmax is the first
 *   bin of strictly greatest count, found by an ascending scan with cnt < hist[b] from cnt = 0.  Then s = 0.0, n = 0; for i ascending, if
 *   hist[bin(a_i)] == hist[binmax] then s += a_i and ++n; action = s / n.  Members of ANOTHER bin with the same count are included: that is
 *   what the reference does.  Tie: more than one bin holds that count.
 * GRLX_ACTOR_ENSEMBLE_DATA_CENTER (csDataCenter, :251-336), parameter `bins` K >= 1, the number of members kept:
 *   All members start alive.  mean is the serial sum of the alive members in ascending order, starting from the first one and not from
 *   0.0, divided by their count.  While more than K are alive: d_i = (a_i - mean) * (a_i - mean) for the alive i; the first alive member
 *   with the greatest d is removed (if every d is 0, that is the first alive member); mean is recomputed the same way.  action = mean.
 *   Tie: at some removal of this step more than one alive member had the greatest d; it counts once per step.  Deviation: the reference
 *   never clears its tie list between removals and indexes it with rand().
 * GRLX_ACTOR_ENSEMBLE_DENSITY (csDensityBased, :183-248), parameter `r` > 0:
 *   n_i = -1 + 2 * ((a_i - lo) / (hi - lo)).  rho_i is the sum over j ascending, from 0.0, of pexp((-1 * ((n_i - n_j) * (n_i - n_j))) /
 *   (r * r)), pexp the portable exponential (GRLX_MATH's, specified by the oracle's orc_pexp).  The first i of strictly greatest rho is
 *   selected, scanning from -inf; action = a_i.  Tie: more than one member has that rho.  At the reference's default r = 0.001 nearly
 *   every rho is exactly 1.0, nearly every step ties and the group's first member acts.
 * Outputs per pair, [n_replicas / group_size][n_starts] (final_state has [state_dims] more); host pointers, any may be NULL:
 *   ret, disc, steps, terminal, final_state   as grlx_evaluate_ensemble defines them
 *   ties    (int32)   the steps at which the rule's selection tied; 0 under MEAN
 *   kept    (int64)   per step, the members that entered the action taken: G under MEAN, n under BINNING, min(G, K) under DATA_CENTER,
 *                     1 under DENSITY; added up over the steps
 *   spread  (double)  per step max_m a_m - min_m a_m, added up in step order: where the members stop agreeing
 * With group_size == 1 every rule hands the member's own action on (a / 1): the episode is grlx_evaluate's, bit for bit.
 *   Records.  grlx_evaluate_actor_ensemble_trajectory: records[group][start][max_steps][R], R = grlx_actor_ensemble_trajectory_record_words(ctx)
 *   = grlx_trajectory_record_words(ctx, 0) + 2.  Every word of the actor-critic's record keeps its index: GRLX_TRAJ_ACTION is the combined
 *   action; GRLX_TRAJ_VALUE the members' arithmetic mean, MEAN's expression, under every rule; GRLX_TRAJ_ACTION_INDEX the selected member's
 *   index in the group under DENSITY, binmax under BINNING, -1 otherwise; GRLX_TRAJ_N_MAX the number of tied candidates -- the members of
 *   greatest rho (DENSITY), the bins of greatest count (BINNING), the greatest number of members tied at one removal of the step
 *   (DATA_CENTER) --, 1 where the rule selects nothing; the two new last words are the step's kept (R - 2) and its spread (R - 1).
 *   Records behind an episode's end are zeros.  The staging rule and its refusals are grlx_evaluate_ensemble_trajectory's.
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the function and the reason named): everything
 * grlx_evaluate refuses; a Q agent ("actor-critic only": grlx_evaluate_ensemble serves those); group_size < 1; n_replicas % group_size
 * != 0; group_size > GRLX_ACTOR_ENSEMBLE_MAX; an unknown rule; bins outside its range for the two rules that read it; r not finite or
 * <= 0 for DENSITY.  n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.  The calls change nothing in the context, do not count
 * as a launch and wait for the stream of the last grlx_run.
 * NOT BUILT: the reference's other strategies (mean_mov, data_center_mean_mov, random, static, value_based), a noisy ensemble, the
 * draws among tied candidates, groups above GRLX_ACTOR_ENSEMBLE_MAX, a streamed variant. */
#define GRLX_ACTOR_ENSEMBLE_MAX 256
enum { GRLX_ACTOR_ENSEMBLE_MEAN = 0, GRLX_ACTOR_ENSEMBLE_BINNING = 1, GRLX_ACTOR_ENSEMBLE_DATA_CENTER = 2, GRLX_ACTOR_ENSEMBLE_DENSITY = 3 };
int  grlx_evaluate_actor_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, int bins, double r,
                                  const double *states /*[n_starts][state_dims]*/, int n_starts, int max_steps,
                                  double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                  int64_t *kept, double *spread, double *final_state);
int  grlx_actor_ensemble_trajectory_record_words(grlx_ctx *ctx);      /* R = grlx_trajectory_record_words(ctx, 0) + 2; a negative status otherwise */
int  grlx_evaluate_actor_ensemble_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, int bins, double r,
                                             const double *states /*[n_starts][state_dims]*/, int n_starts, int max_steps,
                                             double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                             int64_t *kept, double *spread, double *final_state,
                                             double *records /*[n_replicas / group_size][n_starts][max_steps][R]*/);

/* ---------------------------------------------------------------------------------------------------------------
 * The per-step plug-in interfaces on the replicas of a context: one call of the reference's interface for EVERY replica per
 * call, for graphs in which only one side of the loop of OnlineLearningExperiment::run (online_learning.cpp:172-213) lives on the
 * GPU -- the agent beside an environment of the caller's, or the environment beside an agent of the caller's -- from the first
 * step of a trial on.  (grlx_run stays the fast path: it fuses both sides.)  Host pointers, [n_replicas] rows each.
 *   active   NULL = every replica takes part; else only those with a non-zero entry (episodes of different replicas end at
 *            different steps); the output rows of the others are left as the caller passed them.
 * The loop is the caller's: trial / step counters, rows and the steps budget are not advanced by these calls.  State between
 * calls lives where the fused kernels keep it between launches (streams, decay, the predictor's trace), so grlx_run and these
 * calls can be mixed on one context at trial boundaries. */

/* Environment::start (environment.h:48 -> ModeledEnvironment::start, modeled.cpp:132-158): test = 0 a learning trial's start state,
 * 1 a test trial's; the start state is drawn from the replica's own random streams; obs[n_replicas][obs_dims]. */
int  grlx_env_start(grlx_ctx *ctx, int test, const int32_t *active, double *obs);
/* Environment::step (environment.h:49-51 -> ModeledEnvironment::step, modeled.cpp:160-213) on the replicas' model states:
 * action[n_replicas] -> obs[n_replicas][obs_dims], reward[n_replicas], terminal[n_replicas] (0, 1 = timed out, 2 = absorbing); tau = 1
 * (discrete_time).  (grlx_env_step above is the stateless form: explicit states, no context.) */
int  grlx_env_advance(grlx_ctx *ctx, const int32_t *active, const double *action, double *obs, double *reward, int32_t *terminal);
/* Agent::start (agent.h:44-47): test = 0 the learning agent (agent/td, td.cpp:50-61: the predictor's trace is cleared -- not the
 * actor-critic's critic, ac.cpp:170-173 --, time_ = 0, the policy acts), test = 1 the test agent (agent/fixed, fixed.cpp:47-51: the
 * greedy / noise-free policy over the same tables).  obs[n_replicas][obs_dims] -> action[n_replicas]. */
int  grlx_agent_start(grlx_ctx *ctx, int test, const int32_t *active, const double *obs, double *action);
/* Agent::step (agent.h:49-52; td.cpp:63-74: act at obs, then predictor->update(prev_obs, prev_action, tau, reward, obs, action);
 * fixed.cpp:53-61: act).  tau must be 1.  terminal: NULL, or [n_replicas]: a replica whose entry is 2 gets Agent::end instead
 * (online_learning.cpp:210-213) and no action. */
int  grlx_agent_step(grlx_ctx *ctx, int test, const int32_t *active, double tau, const double *obs, const double *reward,
                     const int32_t *terminal, double *action);
/* Agent::end (agent.h:54-56; td.cpp:76-81: the update with an empty next action, target = reward; agent/fixed: nothing). */
int  grlx_agent_end(grlx_ctx *ctx, int test, const int32_t *active, double tau, const double *obs, const double *reward);
/* Built for agent/td with predictor/critic/{sarsa, q, expected_sarsa} (3 or 5 actions, replacing or no trace, no target network,
 * safe = 0) and for the actor-critic agent; GRLX_ERR_INVALID otherwise. */

/* device math used by the environments (bit-identical to the documented
 * portable specification): op 0 sin, 1 cos, 2 log, 3 fmod(x, y[i]), 4 sqrt, 5 x/6 (the 3-operation exact form used by RK4),
 * 6 / 7 / 8 the small-angle-aware sin, cos and sin+cos the compass walker uses (bitwise equal to 0 / 1 / their sum),
 * 9 / 10 / 11 / 12 the UNCHECKED forms the rollout kernels and the environment servers call, with their constants held in
 * registers: sin, sin with the sign set by an integer add (the served pendulum's), cos, sin+cos of one reduction (bitwise equal
 * to 0 / 0 / 1 / their sum on |x| < 2^20; an argument outside, or not finite, is GRLX_ERR_INVALID and nothing is launched),
 * 13 exp (the batch path's logistic; NaN -> NaN, x > 709.782712893384 -> +inf, x < -745.2 -> +0) */
int  grlx_math(int op, const double *x, const double *y, int n, double *out);

/* Rand / RandGen streams (utils.h:84-137) evaluated on the device:
 * out[n] = drand48 of the stream seeded by srand48(seed) after `skip[i]` draws. */
int  grlx_rand48_at(int64_t seed, const uint64_t *skip, int n, double *out);

/* ---------------------------------------------------------------------------------------------------------------
 * The batch path (BASELINE.json configs[4]): experiment/batch_learning + predictor/fqi + representation/iterative +
 * representation/parameterized/ann over projector/pre/normalizing, as the reference's tests/pendulum-fqi-ann.yaml
 * composes them; n_replicas independent-seed copies per GPU.
 * PARITY UNPINNED: the reference's ANN initialisation (Eigen's Random over libc rand(), ann.cpp:97) and its
 * hidden-layer delta (mismatched Eigen dimensions, ann.cpp:249) cannot be reproduced; the four documented
 * deviations are listed at the top of oracle/fqi.c and in DESIGN.md.  Everything else follows the cited lines. */
typedef struct {
  uint32_t struct_size;               /* = sizeof(grlx_fqi_config)                                                */
  int32_t  n_replicas;
  int32_t  env;                       /* GRLX_ENV_PENDULUM (the task must support invert(), pendulum.cpp:147-155) */
  int32_t  integration_steps;         /* model/dynamical                                                          */
  double   control_step;
  double   timeout;                   /* task/pendulum/swingup                                                    */
  double   action_min, action_max;    /* discretizer/uniform over the task's action range                         */
  int32_t  action_steps;
  int32_t  batch_size;                /* experiment/batch_learning:batch_size (transitions drawn per batch)       */
  double   gamma;                     /* predictor/fqi                                                            */
  int32_t  iterations;
  int32_t  epochs;                    /* representation/iterative:epochs                                          */
  int32_t  hidden;                    /* representation/parameterized/ann:hiddens = [hidden]                      */
  int32_t  max_batches;               /* batches reserved (transition store and rows): experiment:batches         */
  double   eta;                       /* representation/parameterized/ann:eta (ann.cpp:198-221): 0 = RPROP        */
} grlx_fqi_config;
typedef struct grlx_fqi_ctx grlx_fqi_ctx;
/* Fill *cfg with the values of the reference's tests/pendulum-fqi-ann.yaml. */
void grlx_fqi_config_pendulum(grlx_fqi_config *cfg);
/* Replaces Configurator::instantiate of that experiment for n_replicas clones after srand48(seeds[r]). */
int  grlx_fqi_create(const grlx_fqi_config *cfg, const int64_t *seeds, grlx_fqi_ctx **out);
int  grlx_fqi_destroy(grlx_fqi_ctx *ctx);
/* Replaces one pass of the batch loop of BatchLearningExperiment::run (batch_learning.cpp:105-188) for every replica:
 * batch_size random transitions (one model step each), FQIPredictor::rebuild over the whole store (fqi.cpp:205-285),
 * one greedy test trial -> one row.  Asynchronous on `stream`. */
int  grlx_fqi_run_batch(grlx_fqi_ctx *ctx, void *stream);
int  grlx_fqi_sync(grlx_fqi_ctx *ctx, void *stream);
/* rows of `<output>-<run>.txt` (batch_learning.cpp:179): batch, batch*batch_size, return of the test trial */
int  grlx_fqi_read_rows(grlx_fqi_ctx *ctx, int replica, int first, int count, int64_t *batch, int64_t *transitions, double *reward);
/* ANNRepresentation::params_: layer 1 (inputs+1) x hidden column-major, then layer 2 (hidden+1) x 1; n must match */
int  grlx_fqi_get_params(grlx_fqi_ctx *ctx, int replica, double *out, int n);
/* the transition store (FQIPredictor::transitions_) as the kernels hold it: normalised (obs, action) inputs [count][3],
 * next observations [count][2], rewards, and the targets of the last iteration; any pointer may be NULL */
int  grlx_fqi_get_transitions(grlx_fqi_ctx *ctx, int replica, int first, int count, double *in, double *next_obs, double *reward, double *targets);
/* state of a replica after the last batch: transitions stored, L-infinity target change and iteration count of the last
 * rebuild (fqi.cpp:213), mean squared error of its last epoch (ann.cpp:201), RNG streams {global, thread-local} */
int  grlx_fqi_info(grlx_fqi_ctx *ctx, int replica, int64_t *n_transitions, double *maxdelta, int32_t *iterations, double *error, uint64_t rng[2]);
/* The batch path's policy query (see the policy queries of the online path above): q[n_replicas][n_obs][action_steps] = Q(s, a_k) of
 * the replicas [first_replica, first_replica + n_replicas) at obs[n_obs][2] -- the projector's normalisation (normalizing.cpp:78-87) and
 * ANNRepresentation::read (ann.cpp:133-160) on the replica's CURRENT parameters, as QPolicy::values forms them (q.cpp:94-107).  Waits
 * for the device; changes nothing in the context.  Validated before anything is launched: null obs, n_obs < 0, the replica range, an
 * observation that is not finite (row and dimension named); n_obs == 0 or n_replicas == 0: GRLX_OK, nothing written.  Staged in
 * chunks of observations like the online queries. */
int  grlx_fqi_query(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *obs /*[n_obs][2]*/, int n_obs, double *q);
/* The batch path's greedy evaluation episodes and their per-step trajectories: grlx_evaluate and grlx_evaluate_trajectory (above)
 * restated for a grlx_fqi_ctx.  For every (replica, start state) pair one episode on the replica's CURRENT parameters, on the device, in
 * one launch per chunk; pair = (replica - first_replica) * n_starts + start; states[n_starts][3] are MODEL states of the pendulum
 * (angle, velocity, time).
 *   The loop.   obs = observe(state); the start state's own terminal code is ignored, so an episode has at least one step.  Per step:
 *               q[k] = Q(obs, a_k), k < action_steps, by the operations of grlx_fqi_query; (mai, man) = the first maximum and the number
 *               of maxima (greedy.cpp:47-61: strict >, counting ==); actions[mai] acts; the model steps; ret += reward;
 *               disc += g * reward; g = g * gamma^control_step (the factor the predictor applies to one step's successor value).
 *               This is the test trial of grlx_fqi_run_batch from a state of the caller's choice WITHOUT its tie-breaking draw: `ties`
 *               counts the steps with man > 1, and with ties == 0 an episode from the task's start (pi, 0, 0) returns, as ret, the
 *               reward of the row the last batch wrote, bit for bit.
 *   terminal    the task's code, 1 or 2; 3 when the step ended outside the portable math's domain (it outranks the task's code and sets
 *               no sticky flag); 0 for an episode cut at max_steps.  max_steps: 1 ... GRLX_MAX_EPISODE_STEPS, 0 = that cap.
 *   records     grlx_fqi_evaluate_trajectory: records[n_replicas][n_starts][max_steps][R], R = grlx_fqi_trajectory_record_words() =
 *               6 + 2 + 3 = 11, the GRLX_TRAJ_* words unchanged: action, reward, value = q[mai], action index, number of maxima, the
 *               code after the step, the observation acted on, the model state after the step.  Records at index >= the pair's steps
 *               are all-zero bits.  max_steps sizes the buffer, so 0 is refused there, as is a null records.
 * ret, disc, steps, terminal, ties: [n_replicas][n_starts]; final_state has [3] more.  Host pointers; any output but records may be NULL.
 * AN EVALUATION CHANGES NOTHING in the context: no row, no batch counter, no stream, no status bit, no parameter.  It is allowed before
 * the first grlx_fqi_run_batch and waits for the device as grlx_fqi_query does.  Staged in chunks of start states under
 * grlx_set_query_chunk_bytes' bound, records included: a single start state's column of records that does not fit is refused, with
 * the remedies named (fewer replicas per call, a smaller max_steps, a larger bound).
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written; row and component named): a null ctx, null
 * states, n_starts < 0, the replica range, max_steps out of range, a state component that is not finite or reaches 2^17 in magnitude.
 * n_starts == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * The same episodes on a group's vote or mean Q: grlx_fqi_evaluate_ensemble (below).
 * NOT BUILT: the reference's tie-breaking draw, tasks other than the pendulum's swing-up. */
int  grlx_fqi_evaluate(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][3]*/, int n_starts, int max_steps,
                       double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state);
int  grlx_fqi_trajectory_record_words(grlx_fqi_ctx *ctx);      /* R = 11; a negative status for a null ctx */
int  grlx_fqi_evaluate_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states /*[n_starts][3]*/, int n_starts,
                                  int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state,
                                  double *records /*[n_replicas][n_starts][max_steps][R]*/);
/* The batch path's ensemble: grlx_query_ensemble, grlx_evaluate_ensemble and grlx_evaluate_ensemble_trajectory (above) restated for a
 * grlx_fqi_ctx, whose replicas are independently seeded networks fitted to independently drawn transition sets (bagged FQI).  The
 * replicas [first_replica, first_replica + n_replicas) form n_replicas / group_size groups of group_size CONSECUTIVE replicas; grouping,
 * outputs and refusals follow the online siblings.
 *   Member values.  For each member m in ASCENDING replica order: q_m[k] = Q(obs, a_k) by the operations of grlx_fqi_query on the
 *               replica's CURRENT parameters; (mai_m, man_m) = the first maximum and the number of maxima (strict >, counting ==);
 *               votes[mai_m] += 1; sumq[k] += q_m[k], one accumulator per action from 0.0 (no tree: that order is the specification);
 *               member_ties += (man_m > 1).
 *   Acting.     score = votes (GRLX_ENSEMBLE_VOTE) or sumq (GRLX_ENSEMBLE_MEAN_Q); (mai, man) = findmax(score); actions[mai] acts, no
 *               draw; ties += (man > 1); agreement += votes[mai] under either rule.
 *   The episode.  grlx_fqi_evaluate's, the members sharing ONE model state: the start state's terminal code is ignored; terminal 0 cut at
 *               max_steps, 1 timed out, 3 left the portable math's domain; max_steps 0 = GRLX_MAX_EPISODE_STEPS; disc uses the context's
 *               gamma^control_step.  group_size == 1 is grlx_fqi_evaluate bit for bit (member_ties = its ties; under GRLX_ENSEMBLE_VOTE one
 *               vote never ties).
 *   records     grlx_fqi_evaluate_ensemble_trajectory: records[groups][n_starts][max_steps][R], R =
 *               grlx_fqi_ensemble_trajectory_record_words() = 8 + 2 + 3 = 13, the online ensemble's words (GRLX_TRAJ_*, GRLX_TRAJ_ENS_*):
 *               GRLX_TRAJ_VALUE is (double)votes[mai] or sumq[mai] (the sum, not the mean), GRLX_TRAJ_ENS_AGREEMENT votes[mai],
 *               GRLX_TRAJ_ENS_MEMBER_TIES the members with man_m > 1 at the step, the observation acted on at GRLX_TRAJ_ENS_OBS, the model
 *               state after the step behind it.  Records at index >= the pair's steps are all-zero bits.  max_steps == 0 and a null
 *               records are refused; so is a start state's column of records (groups * max_steps * R * 8 bytes, with its sums) that
 *               exceeds grlx_set_query_chunk_bytes' bound, with the remedies named.
 *   grlx_fqi_query_ensemble   out[groups][n_obs][2 + 2 * action_steps] = { sum value, sum value * value, sum q[0 .. A), votes[0 .. A) },
 *               grlx_query_ensemble's columns: a member's value is grlx_query_q's (v = 0; for a in order: v += q[a] * dist[a], dist =
 *               1. / man at the maxima and 0 elsewhere); every sum runs in ascending replica order into one accumulator, on the device.
 * ret, disc, steps, terminal, ties, member_ties, agreement: [groups][n_starts]; final_state has [3] more.  Host pointers; any output but
 * records may be NULL.  All four calls wait for the device as grlx_fqi_query does, stage in chunks of start states or observations under
 * grlx_set_query_chunk_bytes' bound and CHANGE NOTHING in the context: no row, no batch counter, no stream, no status bit, no parameter.
 * Validated on the host before anything is launched (GRLX_ERR_INVALID, nothing written, the entry point and the reason named):
 * everything grlx_fqi_evaluate / grlx_fqi_query refuse, group_size < 1, n_replicas % group_size != 0, an unknown rule.  n_starts == 0,
 * n_obs == 0 or n_replicas == 0: GRLX_OK, nothing written.
 * NOT BUILT: sampling from the combined distribution, the reference's other discrete strategies (multiply, rank voting, density based),
 * the reference's tie-breaking draw. */
int  grlx_fqi_query_ensemble(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, const double *obs /*[n_obs][2]*/, int n_obs,
                             double *out);
int  grlx_fqi_evaluate_ensemble(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule,
                                const double *states /*[n_starts][3]*/, int n_starts, int max_steps,
                                double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                int64_t *member_ties, int64_t *agreement, double *final_state);
int  grlx_fqi_ensemble_trajectory_record_words(grlx_fqi_ctx *ctx);      /* R = 13; a negative status for a null ctx */
int  grlx_fqi_evaluate_ensemble_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule,
                                           const double *states /*[n_starts][3]*/, int n_starts, int max_steps,
                                           double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                           int64_t *member_ties, int64_t *agreement, double *final_state,
                                           double *records /*[n_replicas / group_size][n_starts][max_steps][R]*/);

#ifdef __cplusplus
}
#endif
#endif /* GRLX_H_ */
