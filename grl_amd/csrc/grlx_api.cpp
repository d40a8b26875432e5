// grlx_api.cpp -- the C ABI declared in include/grlx.h.
//
// Host-side logic only: validation (grl's bad_param conditions become
// GRLX_ERR_INVALID with a message), the reference's instantiate-order RNG
// seeding, device memory management and kernel launches.  No compute happens on
// the host: without a HIP device every compute entry point fails.
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>
#include "grlx_internal.h"
#include "grlx_snapshot.h"
#include "grlx_query.h"
#include "grlx_evaluate.h"
#include "../../include/grlx_diag.h"

using namespace grlx;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

} // namespace
namespace grlx {
void set_last_error(const char *msg) { g_err = msg; }     // other translation units of the library (grlx_fqi.hip)
void set_fqi_query_chunk_bytes(uint64_t bytes);            // grlx_fqi.hip: the staging bound of grlx_fqi_query
}
namespace {
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e__ = (expr);                                                            \
    if (e__ != hipSuccess)                                                              \
      return fail(GRLX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

bool have_device()
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return false; }
  return n > 0;
}

// host copy of the drand48-family LCG (utils.h:84-137), used only to seed the replicas
constexpr uint64_t kA = 0x5DEECE66DULL, kC = 0xBULL, kM = (1ULL << 48) - 1;
inline uint64_t h_seed(long s) { return ((((uint64_t)s) & 0xFFFFFFFFULL) << 16) | 0x330EULL; }   // srand48
inline uint64_t h_next(uint64_t x) { return (kA * x + kC) & kM; }
inline uint64_t h_jump(uint64_t x, uint64_t n)
{
  uint64_t a = kA, c = kC;
  while (n)
  {
    if (n & 1) x = (a * x + c) & kM;
    c = ((a + 1) * c) & kM;
    a = (a * a) & kM;
    n >>= 1;
  }
  return x;
}

int env_dims(int env, int *S, int *D)
{
  switch (env)
  {
    case GRLX_ENV_PENDULUM: *S = 3; *D = 2; return GRLX_OK;
    case GRLX_ENV_ACROBOT: *S = 5; *D = 4; return GRLX_OK;
    case GRLX_ENV_CART_POLE: *S = 5; *D = 4; return GRLX_OK;
    case GRLX_ENV_COMPASS_WALKER: *S = 11; *D = 5; return GRLX_OK;
    case GRLX_ENV_CART_POLE_BALANCING: *S = 5; *D = 4; return GRLX_OK;
    default: return GRLX_ERR_INVALID;
  }
}

// TileCodingProjector::configure (tile_coding.cpp:45-80)
int make_tile_params(const grlx_tile_spec &ts, TileParams *tp)
{
  if (ts.dims < 1 || ts.dims > GRLX_MAX_DIMS) return fail(GRLX_ERR_INVALID, "projector/tile_coding:resolution (dims %d)", ts.dims);
  if (ts.tilings < 1 || ts.tilings > 32) return fail(GRLX_ERR_INVALID, "projector/tile_coding:tilings (%d)", ts.tilings);
  if (ts.memory < 1 || ts.memory >= (1 << 26)) return fail(GRLX_ERR_INVALID, "projector/tile_coding:memory (1 .. 2^26-1 supported)");
  if (ts.safe < 0 || ts.safe > 2) return fail(GRLX_ERR_INVALID, "projector/tile_coding:safe must be 0, 1 or 2");
  memset(tp, 0, sizeof(*tp));
  tp->T = ts.tilings;
  tp->D = ts.dims;
  tp->memory = ts.memory;
  for (int i = 0; i < ts.dims; ++i)
  {
    if (!(ts.resolution[i] > 0)) return fail(GRLX_ERR_INVALID, "projector/tile_coding:resolution[%d]", i);
    tp->scaling[i] = ts.tilings / ts.resolution[i];
    double w = ts.wrapping[i] * tp->scaling[i];
    if (fabs(w - round(w)) > 0.001)
      return fail(GRLX_ERR_INVALID, "projector/tile_coding:wrapping (scaled wrapping for dimension %d (%.5f) is not an integer)", i, w);
    tp->wrap[i] = (int)round(w);
  }
  return GRLX_OK;
}

int make_linear_params(const grlx_linear_spec &ls, uint64_t draws_before, LinearParams *lp)
{
  lp->init_min = ls.init_min;
  lp->init_range = ls.init_max - ls.init_min;     // utils.h:110-113: a + get()*(b-a)
  lp->out_min = ls.output_min;
  lp->out_max = ls.output_max;
  lp->limit = ls.limit;
  lp->draws_before = draws_before;
  return GRLX_OK;
}

int make_params(const grlx_config &c, DevParams *P)
{
  memset(P, 0, sizeof(*P));
  if (c.struct_size != sizeof(grlx_config)) return fail(GRLX_ERR_INVALID, "grlx_config.struct_size %u != %zu (ABI mismatch)", c.struct_size, sizeof(grlx_config));
  int S, D;
  const bool external = c.env == GRLX_ENV_EXTERNAL;        // the environment is the caller's: per-step agent entry points only
  if (external)
  {
    S = 0;
    D = (c.agent == GRLX_AGENT_AC) ? c.projector.dims : c.projector.dims - 1;
    if (D < 1 || D >= GRLX_MAX_DIMS) return fail(GRLX_ERR_INVALID, "projector/tile_coding:resolution (an external environment's observation has %d dimensions)", D);
    if (!is_td_agent(c.agent) && c.agent != GRLX_AGENT_AC)
      return fail(GRLX_ERR_INVALID, "an external environment is served by the per-step agent entry points: SARSA / Q / Expected SARSA or actor-critic");
  }
  else if (env_dims(c.env, &S, &D) != GRLX_OK) return fail(GRLX_ERR_INVALID, "environment %d is not supported by the fused path", c.env);
  if (!is_td_agent(c.agent) && c.agent != GRLX_AGENT_AC && c.agent != GRLX_AGENT_ADVANTAGE && c.agent != GRLX_AGENT_QV) return fail(GRLX_ERR_INVALID, "agent %d is not supported by the fused path", c.agent);
  // "is it built?" is asked of the kernel table (kernel_built: a row with this key).  An external environment has no rollout kernel: its
  // per-step entry points (grlx_step.h) take what the pendulum's rows take.
  const int row_env = external ? GRLX_ENV_PENDULUM : c.env;
  if (c.agent == GRLX_AGENT_ADVANTAGE)
  {
    if (!(c.kappa > 0)) return fail(GRLX_ERR_INVALID, "predictor/critic/advantage:kappa");
    if (!kernel_built(FAM_TD, c.env, c.action_steps, 4, MODE_ADVANTAGE))
      return fail(GRLX_ERR_INVALID, "advantage learning is built for the pendulum and the acrobot with 3 actions");
  }
  const bool ac = c.agent == GRLX_AGENT_AC;
  const bool qv = c.agent == GRLX_AGENT_QV;
  if (qv && !kernel_built(FAM_QV, c.env, c.action_steps, 4, MODE_IN_PLACE))
    return fail(GRLX_ERR_INVALID, "predictor/critic/qv is built for the pendulum and the acrobot with 3 actions");
  if (qv && !(c.beta > 0)) return fail(GRLX_ERR_INVALID, "predictor/critic/qv:beta");
  if (ac && !external && !kernel_built(FAM_AC, c.env, 0, 4, MODE_DEFERRED)) return fail(GRLX_ERR_INVALID, "actor-critic is built for cart-pole and pendulum");
  if (!external)
  {
  if (c.discrete_time != 1) return fail(GRLX_ERR_INVALID, "environment/modeled:discrete_time must be 1");
  if (!(c.control_step >= 0.00001)) return fail(GRLX_ERR_INVALID, "model/dynamical:control_step");
  if (c.integration_steps < 1 || c.integration_steps > 1000) return fail(GRLX_ERR_INVALID, "model/dynamical:integration_steps (1..1000 supported)");
  // The rollout kernels leave the step loop only when the task reports a terminal state, i.e. (at the
  // latest) on time > timeout: a non-finite or huge timeout would be a kernel that never ends -- on a
  // GPU a hang, not a killable loop.  Episodes are capped at GRLX_MAX_EPISODE_STEPS control steps.
  if (!std::isfinite(c.timeout) || c.timeout < 0) return fail(GRLX_ERR_INVALID, "task:timeout must be finite and >= 0");
  if (!std::isfinite(c.control_step) || c.control_step > 1e6) return fail(GRLX_ERR_INVALID, "model/dynamical:control_step");
  {
    const double horizon = (c.env == GRLX_ENV_COMPASS_WALKER) ? 2 * c.timeout : c.timeout;   // test episodes of the walker: 2 x timeout
    if (std::ceil(horizon / c.control_step) + 1 > (double)GRLX_MAX_EPISODE_STEPS)
      return fail(GRLX_ERR_INVALID, "task:timeout / control_step = %.0f steps per episode exceeds GRLX_MAX_EPISODE_STEPS (%d)",
                  std::ceil(horizon / c.control_step), GRLX_MAX_EPISODE_STEPS);
  }
  }
  if (!ac && (c.action_steps < 1 || c.action_steps > GRLX_MAX_ACTIONS)) return fail(GRLX_ERR_INVALID, "discretizer/uniform:steps (1..%d supported)", GRLX_MAX_ACTIONS);
  if (!ac && !qv && c.agent != GRLX_AGENT_ADVANTAGE && c.trace != GRLX_TRACE_ACCUMULATING && c.env != GRLX_ENV_CART_POLE_BALANCING)
  { // the instantiations of rollout_kernel: anything else has no kernel to run
    if (!kernel_built(FAM_TD, row_env, c.action_steps, 4, MODE_DEFERRED))
      return fail(GRLX_ERR_INVALID, "discretizer/uniform:steps = %d is not built for this environment (pendulum: 3 or 5 actions; "
                                    "acrobot, cart-pole, compass walker: 3 actions)", c.action_steps);
  }
  if (ac && c.trace != GRLX_TRACE_REPLACING && c.trace != GRLX_TRACE_NONE) return fail(GRLX_ERR_INVALID, "trace type %d is not supported by the fused path", c.trace);
  if (c.trace == GRLX_TRACE_ACCUMULATING)
  { // its own (uncached, read-modify-write) kernel: SARSA / Q / Expected SARSA on the pendulum and the acrobot
    if (!is_td_agent(c.agent) || !kernel_built(FAM_ACC, c.env, c.action_steps, 4, MODE_IN_PLACE))
      return fail(GRLX_ERR_INVALID, "trace/enumerated/accumulating is built for SARSA / Q / Expected SARSA on the pendulum and the acrobot with 3 actions");
  }
  else if (c.trace != GRLX_TRACE_NONE && c.trace != GRLX_TRACE_REPLACING) return fail(GRLX_ERR_INVALID, "trace type %d is not supported by the fused path", c.trace);

  P->test_interval = c.test_interval;
  P->env = c.env;
  P->agent = c.agent;
  P->trace_kind = c.trace;
  P->integration_steps = c.integration_steps;
  P->h = external ? 0. : c.control_step / (double)(size_t)c.integration_steps;      // modeled.cpp:257
  P->timeout = c.timeout;
  P->randomization = c.randomization;

  P->control_step = c.control_step;
  P->slope_angle = c.slope_angle;
  P->initial_state_variation = c.initial_state_variation;
  P->negative_reward = c.negative_reward;
  // CSWModel::setTiming (SWModel.cpp:126-130): whole microseconds, then the sub-step of singleStep (:151)
  P->walker_dt = external ? 0. : 1.0E-6 * (double)(uint64_t)floor((c.control_step + 0.5E-6) * 1E6) / c.integration_steps;
  P->end_stop_penalty = c.end_stop_penalty;
  P->action_penalty = c.action_penalty;
  P->action_min = c.action_min;
  P->action_max = c.action_max;
  // UniformDiscretizer::configure (uniform.cpp:60-95)
  P->A = ac ? 0 : c.action_steps;
  if (!ac)
  {
    double range = c.action_max - c.action_min;
    double delta = range / ((double)c.action_steps - 1);
    if (std::isnan(delta)) delta = 0.;
    for (int k = 0; k < c.action_steps; ++k)
      P->actions[k] = c.action_min + delta * k;
  }

  int rc = make_tile_params(c.projector, &P->tile);
  if (rc != GRLX_OK) return rc;
  if (P->tile.T != kLanesPerReplica) return fail(GRLX_ERR_INVALID, "projector/tile_coding:tilings must be %d on the fused path", kLanesPerReplica);
  if (!ac && P->tile.D != D + 1) return fail(GRLX_ERR_INVALID, "projector/tile_coding:resolution must have %d entries (observation + action)", D + 1);
  make_linear_params(c.representation, 0, &P->lin);
  if (ac)
  { // policy/action + predictor/ac/action: actor table first in the yaml, then the critic's (ac_tc.yaml:36-65)
    if (P->tile.D != D) return fail(GRLX_ERR_INVALID, "critic projector/tile_coding:resolution must have %d entries (observation)", D);
    rc = make_tile_params(c.actor_projector, &P->tile_actor);
    if (rc != GRLX_OK) return rc;
    if (P->tile_actor.T != kLanesPerReplica) return fail(GRLX_ERR_INVALID, "actor projector/tile_coding:tilings must be %d on the fused path", kLanesPerReplica);
    if (P->tile_actor.D != D) return fail(GRLX_ERR_INVALID, "actor projector/tile_coding:resolution must have %d entries (observation)", D);
    make_linear_params(c.actor_representation, 0, &P->lin_actor);
    P->lin.draws_before = (uint64_t)c.actor_projector.memory;         // both tables draw from one thread-local stream
    P->actor_alpha = c.actor_alpha;
    P->sigma = c.sigma;
    P->theta = c.theta;
    P->ac_decay_rate = c.ac_decay_rate;
    P->ac_decay_min = c.ac_decay_min;
    P->ac_step_limit = c.ac_step_limit;
    P->ac_update_method = c.ac_update_method;
    if (c.ac_update_method != 0 && c.ac_update_method != 1) return fail(GRLX_ERR_INVALID, "predictor/ac/action:update_method");
    { // equal tile codings (cfg/cart_pole/ac_tc.yaml: the critic's projector copies the actor's resolution and memory): twin tables
      const TileParams &a = P->tile_actor, &b = P->tile;
      bool same = a.T == b.T && a.D == b.D && a.memory == b.memory && c.actor_projector.safe == c.projector.safe;
      for (int i = 0; i < a.D && same; ++i) same = a.scaling[i] == b.scaling[i] && a.wrap[i] == b.wrap[i];
      P->twin_tables = same ? 1 : 0;
    }
    if (!(c.action_min < c.action_max)) return fail(GRLX_ERR_INVALID, "policy/action:{output_min,output_max}");
  }

  if (qv)
  { // predictor/critic/qv: table 0 = the policy's Q representation (first in the yaml), table 1 = v_representation
    rc = make_tile_params(c.actor_projector, &P->tile_actor);
    if (rc != GRLX_OK) return rc;
    if (P->tile_actor.T != kLanesPerReplica) return fail(GRLX_ERR_INVALID, "v_projector/tile_coding:tilings must be %d on the fused path", kLanesPerReplica);
    if (P->tile_actor.D != D) return fail(GRLX_ERR_INVALID, "v_projector/tile_coding:resolution must have %d entries (observation)", D);
    make_linear_params(c.actor_representation, (uint64_t)c.projector.memory, &P->lin_actor);   // drawn after the Q table
    P->beta = c.beta;
  }

  if (c.projector.safe >= 1)
  { // claim table of the tile coding: its own (plain) kernel
    if ((c.agent != GRLX_AGENT_SARSA && c.agent != GRLX_AGENT_Q) || !kernel_built(FAM_TGT, row_env, c.action_steps, 4, MODE_IN_PLACE, 0, 1) ||
        c.trace == GRLX_TRACE_ACCUMULATING)
      return fail(GRLX_ERR_INVALID, "projector/tile_coding:safe >= 1 is built for predictor/critic/sarsa and predictor/critic/q with 3 actions, replacing or no trace");
    if (c.target_interval > 0 && !kernel_built(FAM_TGT, c.env, c.action_steps, 4, MODE_IN_PLACE, 1, 1)) return fail(GRLX_ERR_INVALID, "safe >= 1 together with a target network is built for the pendulum");
    P->tile_safe = c.projector.safe;         // 2: the policy's batch projections claim too
  }
  if ((ac || qv) && c.actor_projector.safe != 0) return fail(GRLX_ERR_INVALID, "projector/tile_coding:safe on the second table");
  if (c.target_interval < 0 || !std::isfinite(c.target_tau)) return fail(GRLX_ERR_INVALID, "representation/parameterized/linear:{interval,tau}");
  if (c.target_interval > 0)
  { // target network of the Q table: its own (plain) kernel
    if (c.agent != GRLX_AGENT_SARSA && c.agent != GRLX_AGENT_Q)
      return fail(GRLX_ERR_INVALID, "representation/parameterized/linear:interval (a target network is built for predictor/critic/sarsa and predictor/critic/q)");
    if (!kernel_built(FAM_TGT, row_env, c.action_steps, 4, MODE_IN_PLACE, 1, 0) || c.trace == GRLX_TRACE_ACCUMULATING)
      return fail(GRLX_ERR_INVALID, "representation/parameterized/linear:interval (built for 3 actions, replacing or no trace)");
    if (c.target_tau < 0 || c.target_tau > 1) return fail(GRLX_ERR_INVALID, "representation/parameterized/linear:tau");
    P->target_interval = c.target_interval;
    P->target_tau = c.target_tau;
    P->lin.draws_before = (uint64_t)c.projector.memory;     // the target is instantiated -- and draws -- first (representation.h:186-190)
  }
  if (c.test_trials < 0) return fail(GRLX_ERR_INVALID, "experiment/online_learning:test_trials");
  P->test_trials = c.test_trials > 1 ? c.test_trials : 1;
  if (P->test_trials > 1 && c.tap_capacity > 0) return fail(GRLX_ERR_INVALID, "test_trials > 1 is not available with taps");
  P->epsilon = c.epsilon;
  P->decay_rate = c.decay_rate;
  P->decay_min = c.decay_min;
  P->alpha = c.alpha;
  P->kappa = c.kappa;
  P->gamma = c.gamma;                     // pow(gamma, tau) with tau = 1
  P->gl = c.gamma * c.lambda;             // pow(gamma*lambda, tau) with tau = 1
  if (c.trace == GRLX_TRACE_ACCUMULATING)
  { // trace.h:249-261: pops while the total decay < 1e-4; the position trace holds 20 entries
    if (!(P->gl > 0 && P->gl < 1)) return fail(GRLX_ERR_INVALID, "predictor: gamma*lambda must be in (0,1) with a trace");
    double tot = 1;
    int n = 0;
    while (tot >= 0.0001 && n <= 20) { tot *= P->gl; n++; }
    if (n > 20) return fail(GRLX_ERR_INVALID, "predictor: gamma*lambda = %g needs an accumulating trace longer than 20 entries", P->gl);
  }
  if (c.trace == GRLX_TRACE_REPLACING)
  { // the register trace holds kMaxTrace entries: the reference pops while the total decay < 0.01 (trace.h:227-231)
    if (!(P->gl > 0 && P->gl < 1)) return fail(GRLX_ERR_INVALID, "predictor: gamma*lambda must be in (0,1) with a trace");
    double tot = 1;
    int n = 0;
    while (tot >= 0.01 && n <= kMaxTrace) { tot *= P->gl; n++; }
    if (n > kMaxTrace) return fail(GRLX_ERR_INVALID, "predictor: gamma*lambda = %g needs a trace longer than %d entries", P->gl, kMaxTrace);
  }
  return GRLX_OK;
}

} // namespace

struct grlx_ctx {
  grlx_config cfg;
  DevParams   P;
  int         S, D;
  Entry        *tables = nullptr;
  ReplicaState *states = nullptr;
  double       *row_reward = nullptr, *row_time = nullptr;
  int64_t      *row_steps = nullptr, *row_trial = nullptr;
  grlx_tap     *taps = nullptr;
  uint32_t     *tap_count = nullptr;
  uint64_t     *scratch = nullptr;        // 8 x u64
  uint32_t     *queue = nullptr;          // work queue of the wide actor-critic kernel: next unstarted replica
  uint32_t     *max_load = nullptr;       // fullest table of the context after the last grlx_run (max_load_kernel)
  uint32_t     logC_max = 26;             // growth bound of the sparse tables
  unsigned long long *diag = nullptr;
  uint32_t     *trace_state = nullptr;
  double       *tvals = nullptr;          // target network values per table position (target_interval > 0)
  // loaded policy images (grlx_load_weights): image k serves the replicas r with image_of[table][r] == k;
  // an image no replica refers to any more is freed at the next load, the rest with the context
  std::vector<double *> images;
  std::vector<int>      image_of[2];
  std::vector<double *> target_images;    // per replica: the target network's dense vector after a load with tau != 0 (ReplicaState::target_base)
  hipStream_t  run_stream = nullptr;      // stream of the last grlx_run / grlx_curve_stats
  bool         run_pending = false;       // ... with work possibly still in flight on it
  int          n_tables = 1;
  int64_t      trials_run = 0;
  const KernelRow *last_row = nullptr;    // the row of the kernel table launched last
  bool         poison = false;            // GRLX_POISON_REGISTERS=<pattern>: diagnostic, see launch_poison_registers
  uint32_t     poison_pattern = 0;
  // the environment server of the pendulum rollout kernels (grlx_env_server.h): mailboxes, its stream, and the fork / join events
  int          env_server = 1;            // GRLX_ENV_SERVER=0 turns it off
  void         *park = nullptr;           // 32-replica waves of the compass walker: parked lane state of the sub-batches beyond the third, per wave
  EnvMail      *env_mail = nullptr;
  size_t       env_mail_bytes = 0;        // per replica: kEnvMailBytes (pendulum kernels) or kWideMailBytes (wide kernels)
  hipStream_t  srv_stream = nullptr;
  hipEvent_t   srv_go = nullptr, srv_done = nullptr;
  // per-step entry points (grlx_env_start / _advance, grlx_agent_start / _step / _end): agent state between calls and the staging
  // buffers of their host arguments, created at the first such call
  AgentRep     *agent_rep = nullptr;
  uint32_t     *agent_lane = nullptr;
  double       *stage_f64 = nullptr;      // [N][GRLX_MAX_DIMS] obs | [N] reward | [N] action
  int32_t      *stage_i32 = nullptr;      // [N] active | [N] terminal
  uint64_t     step_calls = 0;            // agent calls since the last look at the tables' load
  // hyper-parameter sweep (grlx_set_replica_params): the per-replica values as given ([GRLX_PARAM_*][replica]; empty = none set: not a
  // sweep context) and their device records, handed to the SpecSweep rows once the context is a sweep context
  std::vector<double> sweep_host[4];
  SweepParams  *sweep_dev = nullptr;
  bool         sweep = false;
  // A context WITHOUT a trace (GRLX_TRACE_NONE).  The deferred update stores p's weight straight into the table, behind the loads of the
  // next step's weights that are already in flight, and no trace entry forwards it to them (p of consecutive steps is often the same
  // slot); only the instantiations that load again after such an update, or that update in place, equal the reference there:
  //   no_trace_td: SARSA / Q / Expected SARSA without target network and claim table run the sweep kernels on records that all hold the
  //                configuration's values (sweep_dev, made at create): at most 8 replicas per wave, no environment server
  //   no_trace_ac: the actor-critic runs the instantiation that updates the critic in place: 4 replicas per wave
  // (QV, advantage learning, target networks, the claim table and the per-step entries update in place anyway.)
  bool         no_trace_td = false, no_trace_ac = false;
  double       snap_pack_ms = -1, snap_unpack_ms = -1;   // diagnostic: device time of the snapshot kernels in the last save / load
  bool         launched = false;          // a rollout or per-step kernel has run in this context: its replicas' parameters are fixed
};

// small RAII helper for the copy-in / copy-out entry points
namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  template <typename T> T *as() { return (T *)p; }
};
}

// Read-back and fine-grained entry points run on the NULL stream or copy synchronously: wait for the rollouts
// of the last grlx_run first (its stream may be non-blocking with respect to the NULL stream).
static int drain(grlx_ctx *ctx)
{
  if (ctx->run_pending)
  {
    HIP_TRY(hipStreamSynchronize(ctx->run_stream));
    ctx->run_pending = false;
  }
  return GRLX_OK;
}
#define DRAIN(ctx)                          \
  do {                                      \
    int rc__ = drain(ctx);                  \
    if (rc__ != GRLX_OK) return rc__;       \
  } while (0)

extern "C" {

const char *grlx_last_error(void) { return g_err.c_str(); }
int grlx_abi_version(void) { return GRLX_ABI_VERSION; }
#ifndef GRLX_BUILD_PIPELINE
#define GRLX_BUILD_PIPELINE ""
#endif
const char *grlx_build_pipeline(void) { return GRLX_BUILD_PIPELINE; }

int grlx_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

void grlx_config_pendulum_sarsa(grlx_config *c)
{ // the reference's tests/pendulum-sarsa-tc.yaml
  memset(c, 0, sizeof(*c));
  c->struct_size = sizeof(grlx_config);
  c->n_replicas = 1;
  c->test_interval = 10;
  c->env = GRLX_ENV_PENDULUM;
  c->control_step = 0.03;
  c->integration_steps = 5;
  c->discrete_time = 1;
  c->timeout = 2.99;
  c->randomization = 0;
  c->action_min = -3;
  c->action_max = 3;
  c->action_steps = 3;
  c->agent = GRLX_AGENT_SARSA;
  c->projector.tilings = 16;
  c->projector.memory = 8388608;
  c->projector.dims = 3;
  c->projector.resolution[0] = 0.31415;
  c->projector.resolution[1] = 3.1415;
  c->projector.resolution[2] = 3;
  c->projector.wrapping[0] = 6.283;
  c->representation.init_min = 0;
  c->representation.init_max = 1;
  c->representation.output_min = -DBL_MAX;
  c->representation.output_max = DBL_MAX;
  c->representation.limit = 1;
  c->epsilon = 0.05;
  c->decay_rate = 1;
  c->decay_min = 0;
  c->alpha = 0.2;
  c->gamma = 0.97;
  c->lambda = 0.65;
  c->trace = GRLX_TRACE_REPLACING;
  c->ac_step_limit = -1;
  c->table_log2_capacity = 0;
  c->max_rows = 256;
  c->tap_replica = -1;
  c->tap_capacity = 0;
  c->end_stop_penalty = 1;
  c->action_penalty = 0;
  c->slope_angle = 0.004;
  c->initial_state_variation = 0.2;
  c->negative_reward = -100;
}

void grlx_config_cart_pole_ac(grlx_config *c)
{ // the reference's cfg/cart_pole/ac_tc.yaml
  grlx_config_pendulum_sarsa(c);
  c->env = GRLX_ENV_CART_POLE;
  c->control_step = 0.05;
  c->integration_steps = 5;
  c->timeout = 9.99;
  c->randomization = 0;
  c->end_stop_penalty = 0;
  c->action_penalty = 0;
  c->action_min = -15;
  c->action_max = 15;
  c->action_steps = 0;
  c->agent = GRLX_AGENT_AC;
  const double res[4] = {2.5, 0.157075, 2.5, 1.57075}, wrap[4] = {0, 6.283, 0, 0};
  grlx_tile_spec *ts[2] = {&c->projector, &c->actor_projector};
  for (int t = 0; t < 2; ++t)
  {
    memset(ts[t], 0, sizeof(grlx_tile_spec));
    ts[t]->tilings = 16;
    ts[t]->memory = 8388608;
    ts[t]->dims = 4;
    for (int i = 0; i < 4; ++i) { ts[t]->resolution[i] = res[i]; ts[t]->wrapping[i] = wrap[i]; }
  }
  c->actor_representation.init_min = 0;
  c->actor_representation.init_max = 1;
  c->actor_representation.output_min = -15;       // output_min/max: task action_min/max
  c->actor_representation.output_max = 15;
  c->actor_representation.limit = 1;
  c->alpha = 0.2; c->gamma = 0.97; c->lambda = 0.65;   // predictor/critic/td
  c->trace = GRLX_TRACE_REPLACING;
  c->actor_alpha = 0.01;                          // predictor/ac/action:alpha
  c->sigma = 5;
  c->theta = 1;
  c->ac_decay_rate = 1;
  c->ac_decay_min = 0;
  c->ac_update_method = 0;                        // proportional
  c->ac_step_limit = -1;
  // initial size; the tables grow between launches (grlx.h).  2^16 entries hold what ONE launch of 32 cart-pole trials creates from
  // empty tables (about 25 000 slots per table) at a load the 4-way buckets take; 16384 replicas then start at 2 x 16 GiB instead of the
  // 2 x 64 GiB that 2^18 reserved up front.  Callers that must not re-hash between timed launches (bench.py) pass their size.
  c->table_log2_capacity = 16;
}

int grlx_env_dims(int env, int *state_dims, int *obs_dims)
{
  int S, D;
  if (env_dims(env, &S, &D) != GRLX_OK) return fail(GRLX_ERR_INVALID, "unknown environment %d", env);
  if (state_dims) *state_dims = S;
  if (obs_dims) *obs_dims = D;
  return GRLX_OK;
}

// Everything grlx_create refuses before it looks for a device.  P: the parameter block, without device pointers, sizes and layout.
static int admit(const grlx_config *cfg, DevParams *P)
{
  if (cfg->n_replicas < 1) return fail(GRLX_ERR_INVALID, "n_replicas must be >= 1");
  if (cfg->max_rows < 1) return fail(GRLX_ERR_INVALID, "max_rows must be >= 1");
  // more than 8 replicas per wave: 12 and 16 for the actor-critic; for the TD agents the layouts rollout_wide_kernel is built in (16: four
  // sub-batches, the acrobot and the compass walker with three actions; 32: eight, the compass walker)
  const int rpw = cfg->replicas_per_wave;
  if (rpw != 0 && rpw != 4 && rpw != 8 && !((rpw == 12 || rpw == 16) && cfg->agent == GRLX_AGENT_AC) &&
      !(is_td_agent(cfg->agent) && kernel_built(FAM_TD, cfg->env, cfg->action_steps, rpw, MODE_DEFERRED)))
    return fail(GRLX_ERR_INVALID, "replicas_per_wave must be 0 (automatic), 4 or 8 (12: actor-critic only; 16: actor-critic, and the TD agents on the acrobot / the compass walker with 3 actions; 32: the TD agents on the compass walker)");
  if (cfg->wave_limit < 0) return fail(GRLX_ERR_INVALID, "wave_limit must be 0 (automatic) or positive");
  if (cfg->tap_deferred && cfg->tap_replica >= 0 && cfg->tap_capacity > 0 &&
      (!is_td_agent(cfg->agent) || cfg->trace == GRLX_TRACE_ACCUMULATING || !kernel_built(FAM_TD, cfg->env, cfg->action_steps, 4, MODE_TAPPED)))
    return fail(GRLX_ERR_INVALID, "tap_deferred is built for SARSA / Q / Expected SARSA on the pendulum (3 or 5 actions) and the acrobot (3 actions)");
  int rc = make_params(*cfg, P);
  if (rc != GRLX_OK) return rc;
  if (cfg->env == GRLX_ENV_CART_POLE_BALANCING)
    return fail(GRLX_ERR_INVALID, "task/cart_pole/balancing is served by grlx_env_step only (no fused TD rollout is built for it)");
  P->n_replicas = cfg->n_replicas;
  P->max_rows = cfg->max_rows;
  P->no_specialisation = cfg->force_generic;
  P->tap_replica = cfg->tap_replica;
  P->tap_capacity = cfg->tap_replica >= 0 ? cfg->tap_capacity : 0;
  P->tap_starts = cfg->tap_starts != 0 ? 1 : 0;
  P->tap_deferred = (cfg->tap_deferred != 0 && P->tap_capacity > 0) ? 1 : 0;
  return GRLX_OK;
}

int grlx_create(const grlx_config *cfg, const int64_t *seeds, grlx_ctx **out)
{
  if (!cfg || !seeds || !out) return fail(GRLX_ERR_INVALID, "null argument");
  *out = nullptr;
  DevParams P;
  int rc = admit(cfg, &P);
  if (rc != GRLX_OK) return rc;
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");

  grlx_ctx *ctx = new grlx_ctx();
  ctx->cfg = *cfg;
  if (const char *es = getenv("GRLX_ENV_SERVER")) ctx->env_server = atoi(es) != 0;
  if (const char *pz = getenv("GRLX_POISON_REGISTERS"))
  { // diagnostic (tests): every rollout launch is preceded by a kernel that fills the register files with this pattern
    ctx->poison = pz[0] != 0;
    ctx->poison_pattern = (uint32_t)strtoul(pz, nullptr, 0);
  }
  if (cfg->env == GRLX_ENV_EXTERNAL) { ctx->S = 0; ctx->D = (cfg->agent == GRLX_AGENT_AC) ? cfg->projector.dims : cfg->projector.dims - 1; }
  else env_dims(cfg->env, &ctx->S, &ctx->D);
  const int N = cfg->n_replicas;
  uint32_t logC = cfg->table_log2_capacity ? (uint32_t)cfg->table_log2_capacity : 17u;
  if (logC < 8 || logC > 26) { delete ctx; return fail(GRLX_ERR_INVALID, "table_log2_capacity must be in 8..26"); }
  if (cfg->table_log2_max != 0 && (cfg->table_log2_max < (int)logC || cfg->table_log2_max > 26))
  { delete ctx; return fail(GRLX_ERR_INVALID, "table_log2_max must be 0 or in table_log2_capacity..26"); }
  ctx->logC_max = cfg->table_log2_max ? (uint32_t)cfg->table_log2_max : 26u;
  P.logC = logC;
  {
    hipDeviceProp_t prop;
    int dev = 0;
    int simds = 1024;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) simds = 4 * prop.multiProcessorCount;
    const Layout L = choose_layout(*cfg, simds);
    ctx->no_trace_td = L.no_trace_td;
    ctx->no_trace_ac = L.no_trace_ac;
    P.replicas_per_wave = L.replicas_per_wave;
    P.wave_limit = L.wave_limit;
  }

  const size_t n_tables = (cfg->agent == GRLX_AGENT_AC || cfg->agent == GRLX_AGENT_QV) ? 2 : 1;
  ctx->n_tables = (int)n_tables;
  const size_t table_bytes = ((size_t)N * n_tables * sizeof(Entry)) << logC;
#define CTX_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      int code__ = (e__ == hipErrorOutOfMemory) ? GRLX_ERR_OOM : GRLX_ERR_HIP;               \
      fail(code__, "%s failed: %s", #expr, hipGetErrorString(e__));                          \
      grlx_destroy(ctx);                                                                     \
      return code__;                                                                         \
    }                                                                                        \
  } while (0)
  CTX_TRY(hipMalloc((void **)&ctx->tables, table_bytes));
  CTX_TRY(hipMemset(ctx->tables, 0, table_bytes));
  CTX_TRY(hipMalloc((void **)&ctx->states, sizeof(ReplicaState) * (size_t)N));
  CTX_TRY(hipMalloc((void **)&ctx->row_reward, sizeof(double) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMalloc((void **)&ctx->row_steps, sizeof(int64_t) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMalloc((void **)&ctx->row_trial, sizeof(int64_t) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMemset(ctx->row_reward, 0, sizeof(double) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMemset(ctx->row_steps, 0, sizeof(int64_t) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMemset(ctx->row_trial, 0, sizeof(int64_t) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMalloc((void **)&ctx->row_time, sizeof(double) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMemset(ctx->row_time, 0, sizeof(double) * (size_t)N * (size_t)cfg->max_rows));
  CTX_TRY(hipMalloc((void **)&ctx->scratch, sizeof(uint64_t) * 8));
  CTX_TRY(hipMalloc((void **)&ctx->queue, sizeof(uint32_t)));
  // (the sub-batches beyond the second of a 12- / 16-replica wave park their lane state in registers since round 4: no buffer)
  if (P.replicas_per_wave == 32)
  { // ... five of the eight sub-batches of a 32-replica wave here (grlx_rollout_wide.h: MEMP)
    CTX_TRY(hipMalloc(&ctx->park, kAcParkBytes * 5 * (((size_t)N + 31) / 32)));
    P.park = ctx->park;
  }
  CTX_TRY(hipMalloc((void **)&ctx->max_load, sizeof(uint32_t)));
  CTX_TRY(hipMemset(ctx->max_load, 0, sizeof(uint32_t)));
  CTX_TRY(hipMalloc((void **)&ctx->tap_count, sizeof(uint32_t)));
  CTX_TRY(hipMemset(ctx->tap_count, 0, sizeof(uint32_t)));
  if (cfg->agent == GRLX_AGENT_AC)
  { // the critic's trace survives launches: positions live here, all entries invalid at first
    const size_t words = (size_t)N * 16 * kMaxTrace * 2;
    CTX_TRY(hipMalloc((void **)&ctx->trace_state, words * sizeof(uint32_t)));
    std::vector<uint32_t> init(words, 0u);
    for (size_t i = 0; i < words; i += 2) init[i] = kInvalidPos;
    CTX_TRY(hipMemcpy(ctx->trace_state, init.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (P.target_interval > 0)
  {
    const size_t bytes = ((size_t)N * sizeof(double)) << logC;
    CTX_TRY(hipMalloc((void **)&ctx->tvals, bytes));
    CTX_TRY(hipMemset(ctx->tvals, 0xFF, bytes));                     // all ones = not materialised
  }
  if (ctx->no_trace_td)
  { // the records of the sweep kernels, every replica with the configuration's values (grlx_set_replica_params overwrites them)
    SweepParams w;
    w.alpha = P.alpha; w.gamma = P.gamma; w.gl = P.gl; w.epsilon = P.epsilon;
    std::vector<SweepParams> rec((size_t)N, w);
    CTX_TRY(hipMalloc((void **)&ctx->sweep_dev, sizeof(SweepParams) * (size_t)N));
    CTX_TRY(hipMemcpy(ctx->sweep_dev, rec.data(), sizeof(SweepParams) * (size_t)N, hipMemcpyHostToDevice));
  }
  if (P.tap_capacity > 0)
  {
    CTX_TRY(hipMalloc((void **)&ctx->taps, sizeof(grlx_tap) * (size_t)P.tap_capacity));
    CTX_TRY(hipMemset(ctx->taps, 0, sizeof(grlx_tap) * (size_t)P.tap_capacity));
  }

  // Seed every replica exactly as `grld -s seed` instantiates the yaml
  // (deployer.cpp:70-74; configurable.cpp:627-654 instantiate order):
  //   srand48(seed) -> representation reset: thread-local Rand seeded by global lrand48 #1,
  //   memory*outputs uniforms drawn -> learning sampler Rand (global #2) -> test sampler Rand (global #3).
  std::vector<ReplicaState> hs((size_t)N);
  uint64_t table_draws = (uint64_t)cfg->projector.memory;              // outputs = 1
  if (cfg->agent == GRLX_AGENT_AC || cfg->agent == GRLX_AGENT_QV) table_draws += (uint64_t)cfg->actor_projector.memory;
  if (cfg->target_interval > 0) table_draws += (uint64_t)cfg->projector.memory;      // the target network's own initial draws
  for (int r = 0; r < N; ++r)
  {
    ReplicaState &s = hs[(size_t)r];
    memset(&s, 0, sizeof(s));
    uint64_t G = h_seed((long)seeds[r]);
    G = h_next(G);
    s.TL0 = h_seed((long)(G >> 17));
    s.TL = h_jump(s.TL0, table_draws);
    G = h_next(G);
    s.S1 = h_seed((long)(G >> 17));
    G = h_next(G);
    s.S2 = h_seed((long)(G >> 17));
    s.G = G;
    s.eps_decay = 1;
    s.ac_decay = 1;
    s.tr_len = 0;
    s.tr_total = 1;
    if (cfg->agent == GRLX_AGENT_AC)
    { // no samplers: only the thread-local seed is drawn, and grlx_get_rng reports the two streams the graph does not have as 0
      s.G = h_next(h_seed((long)seeds[r]));
      s.S1 = s.S2 = 0;
    }
  }
  CTX_TRY(hipMemcpy(ctx->states, hs.data(), sizeof(ReplicaState) * (size_t)N, hipMemcpyHostToDevice));
#undef CTX_TRY

  P.tables = ctx->tables;
  P.states = ctx->states;
  P.row_reward = ctx->row_reward;
  P.row_time = ctx->row_time;
  P.row_steps = ctx->row_steps;
  P.row_trial = ctx->row_trial;
  P.taps = ctx->taps;
  P.trace_state = ctx->trace_state;
  P.tvals = ctx->tvals;
  P.queue = ctx->queue;
  P.tap_count = ctx->tap_count;
  ctx->P = P;
  *out = ctx;
  return GRLX_OK;
}

int grlx_destroy(grlx_ctx *ctx)
{
  if (!ctx) return GRLX_OK;
  (void)hipFree(ctx->tables);
  (void)hipFree(ctx->states);
  (void)hipFree(ctx->row_reward);
  (void)hipFree(ctx->row_time);
  (void)hipFree(ctx->row_steps);
  (void)hipFree(ctx->row_trial);
  (void)hipFree(ctx->taps);
  (void)hipFree(ctx->tap_count);
  (void)hipFree(ctx->scratch);
  (void)hipFree(ctx->queue);
  if (ctx->env_mail) (void)hipFree(ctx->env_mail);
  if (ctx->park) (void)hipFree(ctx->park);
  if (ctx->sweep_dev) (void)hipFree(ctx->sweep_dev);
  if (ctx->agent_rep) (void)hipFree(ctx->agent_rep);
  if (ctx->agent_lane) (void)hipFree(ctx->agent_lane);
  if (ctx->stage_f64) (void)hipFree(ctx->stage_f64);
  if (ctx->stage_i32) (void)hipFree(ctx->stage_i32);
  if (ctx->srv_go) (void)hipEventDestroy(ctx->srv_go);
  if (ctx->srv_done) (void)hipEventDestroy(ctx->srv_done);
  if (ctx->srv_stream) (void)hipStreamDestroy(ctx->srv_stream);
  (void)hipFree(ctx->max_load);
  (void)hipFree(ctx->diag);
  (void)hipFree(ctx->trace_state);
  (void)hipFree(ctx->tvals);
  for (double *timg : ctx->target_images)
    if (timg) (void)hipFree(timg);
  for (double *img : ctx->images)
    if (img) (void)hipFree(img);
  delete ctx;
  return GRLX_OK;
}

int grlx_set_diag(grlx_ctx *ctx, int enable)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  if (enable && ctx->sweep) return fail(GRLX_ERR_INVALID, "diagnostics are not built for a sweep context (grlx_set_replica_params)");
  if (enable == 2 && ctx->cfg.trace == GRLX_TRACE_NONE)
    return fail(GRLX_ERR_INVALID, "stamps of the production ordering (grlx_set_diag 2) are not built for a context without a trace "
                                  "(trace = GRLX_TRACE_NONE): use the in-place stamps (grlx_set_diag 1)");
  const size_t waves = ((size_t)ctx->P.n_replicas + kReplicasPerWave - 1) / kReplicasPerWave;
  if (enable && !ctx->diag)
  {
    HIP_TRY(hipMalloc((void **)&ctx->diag, waves * 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(ctx->diag, 0, waves * 8 * sizeof(unsigned long long)));
  }
  ctx->P.diag_out = enable ? ctx->diag : nullptr;
  ctx->P.diag_deferred = enable == 2 ? 1 : 0;     // 1: in-place instantiation (taps possible), 2: the production ordering
  return GRLX_OK;
}

int grlx_read_diag(grlx_ctx *ctx, uint64_t *out, int cap_waves, int *n_waves)
{
  if (!ctx || !out || !n_waves) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!ctx->diag) return fail(GRLX_ERR_INVALID, "diagnostics are not enabled");
  int waves = (ctx->P.n_replicas + kReplicasPerWave - 1) / kReplicasPerWave;
  if (waves > cap_waves) waves = cap_waves;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(out, ctx->diag, (size_t)waves * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  *n_waves = waves;
  return GRLX_OK;
}

// Re-hash every table of the context into tables of 2^new_logC entries per replica.  Positions are internal to the tables,
// to the persisted actor-critic trace and to the target values (both translated); nothing else refers to them.
static int grow_tables(grlx_ctx *ctx, uint32_t new_logC)
{
  if (new_logC <= ctx->P.logC) return GRLX_OK;
  if (new_logC > 26) return fail(GRLX_ERR_INVALID, "tables cannot grow beyond 2^26 entries");
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)ctx->P.n_replicas, n_tables = (size_t)ctx->n_tables;
  const size_t new_bytes = (N * n_tables * sizeof(Entry)) << new_logC;
  DevBuf nt, remap, ntv;                     // freed on every early return; ownership moves to the context at the end
  if (nt.alloc(new_bytes) != hipSuccess ||
      ((ctx->trace_state || ctx->tvals) && remap.alloc((N * sizeof(uint32_t)) << ctx->P.logC) != hipSuccess) ||
      (ctx->tvals && ntv.alloc((N * sizeof(double)) << new_logC) != hipSuccess))
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "no device memory to grow the sparse tables to 2^%u entries per replica (%.1f GiB)", new_logC,
                (double)new_bytes / 1073741824.);
  }
  HIP_TRY(hipMemset(nt.p, 0, new_bytes));
  if (ntv.p) HIP_TRY(hipMemset(ntv.p, 0xFF, (N * sizeof(double)) << new_logC));
  HIP_TRY(launch_rehash(ctx->P, ctx->n_tables, (Entry *)nt.p, new_logC, (uint32_t *)remap.p, nullptr));
  if (remap.p) HIP_TRY(launch_remap_positions(ctx->P, (const uint32_t *)remap.p, new_logC, (double *)ntv.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  (void)hipFree(ctx->tables);
  if (ctx->tvals) (void)hipFree(ctx->tvals);
  ctx->tables = (Entry *)nt.p;
  ctx->tvals = (double *)ntv.p;
  nt.p = nullptr;
  ntv.p = nullptr;
  ctx->P.tables = ctx->tables;
  ctx->P.tvals = ctx->tvals;
  ctx->P.logC = new_logC;
  return GRLX_OK;
}

int grlx_table_capacity(grlx_ctx *ctx, uint32_t *log2_entries)
{
  if (!ctx || !log2_entries) return fail(GRLX_ERR_INVALID, "bad argument");
  *log2_entries = ctx->P.logC;
  return GRLX_OK;
}

int grlx_grow_tables(grlx_ctx *ctx, uint32_t new_log2)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  DRAIN(ctx);
  return grow_tables(ctx, new_log2);
}

// Experiment::reset() between two runs of one process (online_learning.cpp:307-308 -> {action: reset} over the experiment's subtree):
// every parameter is drawn again from the CONTINUING thread-local stream (linear.cpp:104-125; with lazy initialisation: the stream
// position becomes the new base of the draws and moves on by the tables' sizes, the sparse tables empty), the traces are cleared
// (sarsa.cpp:60-66, td.cpp:64), the exploration decay of sampler/epsilon_greedy and mapping/policy/action goes back to 1
// (greedy.cpp:140-141, action.cpp:93-97), the run's counters (ss, tt) and rows start again.  Nothing is reseeded: the global stream,
// the samplers' private streams and the environment state continue -- which is why run 1 of `runs: 2` differs from a fresh process.
int grlx_reset_run(grlx_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  DRAIN(ctx);
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)ctx->P.n_replicas;
  std::vector<ReplicaState> hs(N);
  HIP_TRY(hipMemcpy(hs.data(), ctx->states, sizeof(ReplicaState) * N, hipMemcpyDeviceToHost));
  uint64_t table_draws = (uint64_t)ctx->cfg.projector.memory;
  if (ctx->cfg.agent == GRLX_AGENT_AC || ctx->cfg.agent == GRLX_AGENT_QV) table_draws += (uint64_t)ctx->cfg.actor_projector.memory;
  // a target network is reached by the walk too (a provided object is a child configurator, visited before the representation itself:
  // configurable.cpp:690-712, 754-757): it draws again first, the representation next, synchronize() blends the two fresh vectors -- the
  // sequence of construction, from the continuing stream; ParameterizedRepresentation::count_ = 0
  if (ctx->cfg.target_interval > 0) table_draws += (uint64_t)ctx->cfg.projector.memory;
  for (ReplicaState &s : hs)
  {
    s.sync_count = 0;
    s.syncs = 0;
    s.TL0 = s.TL;                         // the re-draw starts where the stream stands
    s.TL = h_jump(s.TL, table_draws);
    s.eps_decay = 1;
    s.ac_decay = 1;
    s.tr_len = 0;
    s.tr_total = 1;
    s.tt = 0;
    s.ss = 0;
    s.test_steps = 0;                     // (grlx_step_counts counts per run)
    s.rows = 0;
    s.n_slots[0] = s.n_slots[1] = 0;
    s.lazy_base[0] = s.lazy_base[1] = nullptr;      // a loaded policy is overwritten by the re-draw like every other parameter
    s.target_base = nullptr;
    s.syncs_base = 0;
  }
  HIP_TRY(hipMemcpy(ctx->states, hs.data(), sizeof(ReplicaState) * N, hipMemcpyHostToDevice));
  // (emptying the tables drops the claims of projector/tile_coding:safe with them: tile_coding.cpp:82-89)
  HIP_TRY(hipMemset(ctx->tables, 0, (N * (size_t)ctx->n_tables * sizeof(Entry)) << ctx->P.logC));
  if (ctx->tvals) HIP_TRY(hipMemset(ctx->tvals, 0xFF, (N * sizeof(double)) << ctx->P.logC));      // kTvalUnset: not materialised
  HIP_TRY(hipMemset(ctx->max_load, 0, sizeof(uint32_t)));
  if (ctx->trace_state)
  {
    const size_t words = N * 16 * kMaxTrace * 2;
    std::vector<uint32_t> init(words, 0u);
    for (size_t i = 0; i < words; i += 2) init[i] = kInvalidPos;
    HIP_TRY(hipMemcpy(ctx->trace_state, init.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (ctx->tap_count) HIP_TRY(hipMemset(ctx->tap_count, 0, sizeof(uint32_t)));
  if (ctx->agent_rep) HIP_TRY(hipMemset(ctx->agent_rep, 0, sizeof(AgentRep) * N));
  if (ctx->agent_lane) HIP_TRY(hipMemset(ctx->agent_lane, 0, sizeof(uint32_t) * N * 16 * 2));
  for (double *&timg : ctx->target_images)
    if (timg) { (void)hipFree(timg); timg = nullptr; }
  ctx->trials_run = 0;
  return GRLX_OK;
}

// Mailboxes, stream and events of the environment server, created at the first launch that wants them.  The server is an optimisation: when
// its 1 KB per replica (or a stream, or an event) cannot be had, the context goes on without it.
static bool env_server_ready(grlx_ctx *ctx, size_t mail_bytes)
{
  if (ctx->env_mail) return true;
  ctx->env_mail_bytes = mail_bytes;
  bool ok = mail_bytes != 0 && hipMalloc((void **)&ctx->env_mail, (size_t)ctx->P.n_replicas * ctx->env_mail_bytes) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&ctx->srv_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ctx->srv_go, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ctx->srv_done, hipEventDisableTiming) == hipSuccess;
  if (ok) return true;
  (void)hipGetLastError();
  if (ctx->env_mail) (void)hipFree(ctx->env_mail);
  if (ctx->srv_go) (void)hipEventDestroy(ctx->srv_go);
  if (ctx->srv_done) (void)hipEventDestroy(ctx->srv_done);
  if (ctx->srv_stream) (void)hipStreamDestroy(ctx->srv_stream);
  ctx->env_mail = nullptr; ctx->srv_go = ctx->srv_done = nullptr; ctx->srv_stream = nullptr;
  ctx->env_server = 0;
  return false;
}

static int run_trials(grlx_ctx *ctx, int n_trials, uint64_t steps_budget, void *stream)
{
  if (!ctx || n_trials < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "this context has no environment (GRLX_ENV_EXTERNAL): drive it through grlx_agent_start / _step / _end");
  if (n_trials == 0) return GRLX_OK;
  if (steps_budget != 0 && (ctx->P.tap_capacity > 0 || ctx->P.diag_out))
    return fail(GRLX_ERR_INVALID, "a steps budget is not available with taps or diagnostics");
  if (!ctx->run_pending && ctx->P.logC < ctx->logC_max)
  { // nothing in flight: how full did the last run leave the fullest table?  Beyond a quarter, grow to an eighth.
    uint32_t used = 0;
    HIP_TRY(hipMemcpy(&used, ctx->max_load, sizeof(used), hipMemcpyDeviceToHost));
    if ((uint64_t)used * 4u > (1ull << ctx->P.logC))
    {
      uint32_t want = ctx->P.logC;
      while ((uint64_t)used * 8u > (1ull << want) && want < ctx->logC_max) ++want;
      const int rc = grow_tables(ctx, want);
      if (rc == GRLX_ERR_OOM)
      { // growing needs the old and the new tables at once: when that does not fit, the run goes on in the tables it has
        // (a quarter full is not an overflow; a real one is still reported as GRLX_ERR_TABLE_FULL) and does not try again
        g_err.clear();
        ctx->logC_max = ctx->P.logC;
      }
      else if (rc != GRLX_OK) return rc;
    }
  }
  // a run still pending on ANOTHER stream is waited for first: only one stream is remembered, and the launches below
  // continue from the replica state that run leaves behind
  if (ctx->run_pending && ctx->run_stream != (hipStream_t)stream) DRAIN(ctx);
  // One launch per <= kTrialsPerLaunch trials: replica state (and the actor-critic trace) persists in
  // HBM between launches, so results do not depend on the chunking (tested), and no single kernel
  // runs for minutes (compass walker: up to 1000 steps per episode).
  // A launch also never holds more than ~kStepsPerLaunch control steps of one replica (long episodes: fewer trials).
  const double kStepsPerLaunch = 65536;
  const double horizon = (ctx->cfg.env == GRLX_ENV_COMPASS_WALKER ? 2 : 1) * ctx->cfg.timeout / ctx->cfg.control_step + 1;
  int kTrialsPerLaunch = 32;
  if (horizon * kTrialsPerLaunch > kStepsPerLaunch) kTrialsPerLaunch = (int)fmax(1., floor(kStepsPerLaunch / horizon));
  // with a steps budget the budget bounds what one replica does in a launch (its remaining steps plus one episode): all trials go into
  // ONE launch, so that a replica which has reached its budget does not wait at 32-trial boundaries for the ones that have not
  DevParams Pb = ctx->P;
  Pb.steps_budget = steps_budget;
  if (steps_budget != 0) kTrialsPerLaunch = n_trials;
  ctx->run_stream = (hipStream_t)stream;
  ctx->run_pending = true;
  ctx->launched = true;
  for (int done = 0; done < n_trials; done += kTrialsPerLaunch)
  {
    const int n = (n_trials - done < kTrialsPerLaunch) ? n_trials - done : kTrialsPerLaunch;
    if (done > 0 && ctx->P.logC < ctx->logC_max)
    { // a run of several launches: the tables may grow BETWEEN its launches too (a launch cannot grow them).  One 4-byte read-back per
      // further launch, which waits for the launch before it: a call of more than kTrialsPerLaunch trials is no longer fully asynchronous
      // while the tables may still grow (a deployer runs a whole run as ONE grlx_run; cart-pole actor-critic tables start at 2^16 entries
      // and 32 trials create about 25 000 slots per table)
      uint32_t used = 0;
      HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load, (hipStream_t)stream));
      HIP_TRY(hipMemcpyAsync(&used, ctx->max_load, sizeof(used), hipMemcpyDeviceToHost, (hipStream_t)stream));
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      if ((uint64_t)used * 4u > (1ull << ctx->P.logC))
      {
        uint32_t want = ctx->P.logC;
        while ((uint64_t)used * 8u > (1ull << want) && want < ctx->logC_max) ++want;
        const int rc = grow_tables(ctx, want);
        if (rc == GRLX_ERR_OOM) { g_err.clear(); ctx->logC_max = ctx->P.logC; }
        else if (rc != GRLX_OK) return rc;
        Pb.tables = ctx->P.tables;                 // the launches below work on the new tables
        Pb.tvals = ctx->P.tvals;
        Pb.logC = ctx->P.logC;
      }
    }
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, (hipStream_t)stream));
    // stamps and per-step taps are recorded by instantiations of their own, which a context without a trace may run as they are
    PlanFacts facts;
    facts.sweep = ctx->sweep || (ctx->no_trace_td && !records(Pb));        // (without the environment server)
    facts.ac_in_place = ctx->no_trace_ac;
    facts.server = ctx->env_server != 0;
    const char *walker = getenv("GRLX_ENV_SERVER_WALKER");
    facts.walker_server = walker && atoi(walker) != 0;
    facts.fits = waves_fit_together;
    KernelPlan plan = plan_rollout(Pb, facts);
    if (plan.server && !((size_t)ctx->P.n_replicas * plan.row->mail_bytes < (1ull << 31) && env_server_ready(ctx, plan.row->mail_bytes)))
    { // the server is an optimisation: without its mailboxes the launch is planned again without it
      facts.server = false;
      plan = plan_rollout(Pb, facts);
    }
    if (plan.server)
    { // the server's launch forks off the caller's stream and joins it again: for the caller, still one stream-ordered operation
      Pb.env_mail = ctx->env_mail;
      Pb.env_tune = 3u;        // the rollout wave is the critical path: it issues first, the server fills its gaps (+0.7 %)
      if (const char *tune = getenv("GRLX_ENV_SERVER_TUNE")) Pb.env_tune = (uint32_t)strtoul(tune, nullptr, 0);
      HIP_TRY(hipMemsetAsync(ctx->env_mail, 0, (size_t)ctx->P.n_replicas * ctx->env_mail_bytes, (hipStream_t)stream));
      HIP_TRY(hipEventRecord(ctx->srv_go, (hipStream_t)stream));
      HIP_TRY(hipStreamWaitEvent(ctx->srv_stream, ctx->srv_go, 0));
    }
    HIP_TRY(launch_plan(plan, Pb, n, ctx->sweep_dev, (hipStream_t)stream, ctx->srv_stream));
    ctx->last_row = plan.row;
    if (plan.server)
    {
      HIP_TRY(hipEventRecord(ctx->srv_done, ctx->srv_stream));
      HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ctx->srv_done, 0));
    }
  }
  HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load, (hipStream_t)stream));
  ctx->trials_run += n_trials;
  return GRLX_OK;
}

// diagnostic (not part of include/grlx.h): the mailboxes of the environment server after the last launch (GRLX_ENV_SERVER_STATS builds
// leave cycle counts in EnvMail::stats)
int grlx_env_server_debug(grlx_ctx *ctx, void *out, size_t bytes)
{
  if (!ctx || !out) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!ctx->env_mail) return fail(GRLX_ERR_INVALID, "the environment server has not run in this context");
  DRAIN(ctx);
  const size_t have = (size_t)ctx->P.n_replicas * ctx->env_mail_bytes;
  HIP_TRY(hipMemcpy(out, ctx->env_mail, bytes < have ? bytes : have, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// diagnostic (not part of include/grlx.h): in the last launch that had the environment server, how many replicas took every step from it
// and how many gave up waiting and integrated themselves; both 0 when no launch of this context had it
int grlx_env_server_counts(grlx_ctx *ctx, int *served, int *fell_back)
{
  if (!ctx || !served || !fell_back) return fail(GRLX_ERR_INVALID, "bad argument");
  *served = *fell_back = 0;
  if (!ctx->env_mail) return GRLX_OK;
  DRAIN(ctx);
  std::vector<unsigned long long> flag((size_t)ctx->P.n_replicas);
  HIP_TRY(hipMemcpy2D(flag.data(), sizeof(unsigned long long), (const char *)ctx->env_mail + kEnvMailFlagOffset, ctx->env_mail_bytes,
                      sizeof(unsigned long long), (size_t)ctx->P.n_replicas, hipMemcpyDeviceToHost));
  for (unsigned long long f : flag)
  {
    if (f == 1u) ++*served;
    if (f == 2u) ++*fell_back;
  }
  return GRLX_OK;
}

// diagnostic (not part of include/grlx.h): per replica, the passes its wave took in the wave-uniform loop of rollout_served_kernel
// (grlx_rollout.h) in the last launch that had the environment server; zeros when no launch of this context had it
int grlx_uniform_pass_counts(grlx_ctx *ctx, unsigned long long *out, int count)
{
  if (!ctx || !out || count < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  const int n = count < ctx->P.n_replicas ? count : ctx->P.n_replicas;
  for (int i = 0; i < count; ++i) out[i] = 0;
  if (!ctx->env_mail || n == 0) return GRLX_OK;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy2D(out, sizeof(unsigned long long), (const char *)ctx->env_mail + kEnvMailUniformOffset, ctx->env_mail_bytes,
                      sizeof(unsigned long long), (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// diagnostic (not part of include/grlx.h): per replica, the word grlx_env_server_counts sums -- 1 served to the end of the last launch
// that had the environment server, 2 fell back; zeros when no launch of this context had it
int grlx_env_server_flags(grlx_ctx *ctx, int32_t *out, int count)
{
  if (!ctx || !out || count < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  const int n = count < ctx->P.n_replicas ? count : ctx->P.n_replicas;
  for (int i = 0; i < count; ++i) out[i] = 0;
  if (!ctx->env_mail || n == 0) return GRLX_OK;
  DRAIN(ctx);
  std::vector<unsigned long long> flag((size_t)n);
  HIP_TRY(hipMemcpy2D(flag.data(), sizeof(unsigned long long), (const char *)ctx->env_mail + kEnvMailFlagOffset, ctx->env_mail_bytes,
                      sizeof(unsigned long long), (size_t)n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) out[i] = (int32_t)flag[(size_t)i];
  return GRLX_OK;
}

int grlx_run(grlx_ctx *ctx, int n_trials, void *stream) { return run_trials(ctx, n_trials, 0, stream); }

// The trial loop of OnlineLearningExperiment::run with both of its bounds (online_learning.cpp:154):
//   for (ss = 0, tt = 0; (!trials_ || tt < trials_) && (!steps_ || ss < steps_); ++tt)
// every replica runs at most `max_trials` further trials and starts none once its learning steps of the run (since grlx_create or
// grlx_reset_run) have reached `steps`.  Replicas stop at trials of their own: rows are ragged (grlx_replica_rows, grlx_curve_stats
// counts per row).  One launch: `steps` bounds the work of a replica.
int grlx_run_steps(grlx_ctx *ctx, int max_trials, uint64_t steps, void *stream)
{
  if (steps == 0) return fail(GRLX_ERR_INVALID, "grlx_run_steps: steps must be > 0 (grlx_run has no budget)");
  if (steps > (1ull << 40)) return fail(GRLX_ERR_INVALID, "grlx_run_steps: steps out of range");
  return run_trials(ctx, max_trials, steps, stream);
}

static int status_to_error(uint64_t st)
{
  if (st & ST_TABLE_FULL) return fail(GRLX_ERR_TABLE_FULL, "a replica's sparse weight table overflowed: raise table_log2_capacity");
  if (st & ST_TRACE_OVERFLOW) return fail(GRLX_ERR_INVALID, "register trace overflow");
  if (st & ST_BAD_POS) return fail(GRLX_ERR_INVALID, "internal error: a TD update was queued without a table position");
  if (st & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "sin/cos argument outside |x| < 2^20");
  if (st & ST_ROWS_FULL) return fail(GRLX_ERR_ROWS_FULL, "more test rows than max_rows");
  return GRLX_OK;
}

int grlx_sync(grlx_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  uint64_t h[3];
  if ((hipStream_t)stream != ctx->run_stream) DRAIN(ctx);
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch, (hipStream_t)stream));
  HIP_TRY(hipMemcpyAsync(h, ctx->scratch, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if ((hipStream_t)stream == ctx->run_stream) ctx->run_pending = false;
  return status_to_error(h[2]);
}

int grlx_step_counts(grlx_ctx *ctx, uint64_t *learn_steps, uint64_t *test_steps)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  uint64_t h[3];
  DRAIN(ctx);
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch, nullptr));
  HIP_TRY(hipMemcpy(h, ctx->scratch, sizeof(h), hipMemcpyDeviceToHost));
  if (learn_steps) *learn_steps = h[0];
  if (test_steps) *test_steps = h[1];
  return GRLX_OK;
}

int grlx_rows(grlx_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  ReplicaState s;
  DRAIN(ctx);
  if (hipMemcpy(&s, ctx->states, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemcpy failed");
  return (int)s.rows;
}

int grlx_replica_rows(grlx_ctx *ctx, int replica)
{
  if (!ctx || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  if (hipMemcpy(&s, ctx->states + replica, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemcpy failed");
  return (int)s.rows;
}

int grlx_read_rows(grlx_ctx *ctx, int replica, int first, int count, int64_t *trial, int64_t *steps, double *reward)
{
  if (!ctx || replica < 0 || replica >= ctx->P.n_replicas || first < 0 || count < 0 || first + count > ctx->P.max_rows)
    return fail(GRLX_ERR_INVALID, "bad argument");
  const size_t N = (size_t)ctx->P.n_replicas;
  if (count == 0) return GRLX_OK;
  DRAIN(ctx);
  // rows are stored [row][replica]: one strided copy per column
  const size_t at = (size_t)first * N + (size_t)replica;
  if (reward) HIP_TRY(hipMemcpy2D(reward, sizeof(double), ctx->row_reward + at, N * sizeof(double), sizeof(double), (size_t)count, hipMemcpyDeviceToHost));
  if (steps) HIP_TRY(hipMemcpy2D(steps, sizeof(int64_t), ctx->row_steps + at, N * sizeof(int64_t), sizeof(int64_t), (size_t)count, hipMemcpyDeviceToHost));
  if (trial) HIP_TRY(hipMemcpy2D(trial, sizeof(int64_t), ctx->row_trial + at, N * sizeof(int64_t), sizeof(int64_t), (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_last_kernel(grlx_ctx *ctx) { return ctx && ctx->last_row ? ctx->last_row->variant : GRLX_KERNEL_NONE; }
const char *grlx_last_kernel_name(grlx_ctx *ctx) { return ctx && ctx->last_row ? ctx->last_row->name : ""; }
int grlx_replicas_per_wave(grlx_ctx *ctx) { return ctx ? ctx->P.replicas_per_wave : 0; }

int grlx_read_row_times(grlx_ctx *ctx, int replica, int first, int count, double *episode_time)
{
  if (!ctx || !episode_time || replica < 0 || replica >= ctx->P.n_replicas || first < 0 || count < 0 || first + count > ctx->P.max_rows)
    return fail(GRLX_ERR_INVALID, "bad argument");
  const size_t N = (size_t)ctx->P.n_replicas;
  if (count == 0) return GRLX_OK;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy2D(episode_time, sizeof(double), ctx->row_time + (size_t)first * N + (size_t)replica, N * sizeof(double), sizeof(double),
                      (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_curve_stats_grouped(grlx_ctx *ctx, int first, int count, int group_size, double *out_dev, void *stream)
{
  if (!ctx || !out_dev || first < 0 || count < 0 || first + count > ctx->P.max_rows) return fail(GRLX_ERR_INVALID, "bad argument");
  if (group_size < 1 || ctx->P.n_replicas % group_size != 0)
    return fail(GRLX_ERR_INVALID, "group_size = %d does not divide the %d replicas into whole groups", group_size, ctx->P.n_replicas);
  if (ctx->run_pending && ctx->run_stream != (hipStream_t)stream) DRAIN(ctx);
  HIP_TRY(launch_curve_stats_grouped(ctx->P, first, count, group_size, out_dev, (hipStream_t)stream));
  return GRLX_OK;
}

// ---- hyper-parameter sweep: alpha, gamma, lambda, epsilon per replica --------------------------------------------------------------
namespace {
const char *const kSweepParamName[4] = {"alpha", "gamma", "lambda", "epsilon"};

double sweep_config_value(const grlx_ctx *ctx, int param)
{
  switch (param)
  {
    case GRLX_PARAM_ALPHA: return ctx->cfg.alpha;
    case GRLX_PARAM_GAMMA: return ctx->cfg.gamma;
    case GRLX_PARAM_LAMBDA: return ctx->cfg.lambda;
    default: return ctx->cfg.epsilon;
  }
}

// The record of ONE replica of a sweep context from its four values, validated as make_params validates the shared ones: finite; with a
// replacing trace gamma*lambda in (0,1) and its trace within kMaxTrace entries.  `param`: the GRLX_PARAM_* the caller is setting (the message
// names it and its value).  The one rule for grlx_set_replica_params and grlx_snapshot_load.
int sweep_record(const grlx_config &c, size_t r, double alpha, double gamma, double lambda, double epsilon, int param, SweepParams *w)
{
  const double four[4] = {alpha, gamma, lambda, epsilon};
  for (int i = 0; i < 4; ++i)
  { // the value being set first, then the other three
    const int k = i == 0 ? param : (i <= param ? i - 1 : i);
    if (!std::isfinite(four[k])) return fail(GRLX_ERR_INVALID, "%s of replica %zu is not finite (%g)", kSweepParamName[k], r, four[k]);
  }
  w->alpha = alpha;
  w->gamma = gamma;
  w->gl = gamma * lambda;      // pow(gamma*lambda, tau) with tau = 1, as make_params forms it
  w->epsilon = epsilon;
  if (c.trace == GRLX_TRACE_REPLACING)
  {
    if (!(w->gl > 0 && w->gl < 1))
      return fail(GRLX_ERR_INVALID, "replica %zu: %s = %g gives gamma*lambda = %g, which must be in (0,1) with a trace", r, kSweepParamName[param], four[param], w->gl);
    double tot = 1;
    int n = 0;
    while (tot >= 0.01 && n <= kMaxTrace) { tot *= w->gl; n++; }
    if (n > kMaxTrace)
      return fail(GRLX_ERR_INVALID, "replica %zu: %s = %g gives gamma*lambda = %g, which needs a trace longer than %d entries", r, kSweepParamName[param],
                  four[param], w->gl, kMaxTrace);
  }
  return GRLX_OK;
}

// what a sweep context is built for; the message names what is not
int sweep_admits(const grlx_config &c, const DevParams &P)
{
  if (c.env == GRLX_ENV_EXTERNAL)
    return fail(GRLX_ERR_INVALID, "per-replica parameters are not built for GRLX_ENV_EXTERNAL (the per-step entry points read the shared values)");
  if (!is_td_agent(c.agent))
    return fail(GRLX_ERR_INVALID, "per-replica parameters are built for the agents SARSA, Q and Expected SARSA (agent %d is not)", c.agent);
  if (c.trace != GRLX_TRACE_REPLACING && c.trace != GRLX_TRACE_NONE)
    return fail(GRLX_ERR_INVALID, "per-replica parameters are built for a replacing trace or none (an accumulating trace is not)");
  if (c.target_interval > 0) return fail(GRLX_ERR_INVALID, "per-replica parameters are not built with a target network (representation interval > 0)");
  if (c.projector.safe != 0) return fail(GRLX_ERR_INVALID, "per-replica parameters are not built with projector/tile_coding:safe");
  if (P.tap_capacity > 0) return fail(GRLX_ERR_INVALID, "per-replica parameters are not built with taps");
  if (P.diag_out) return fail(GRLX_ERR_INVALID, "per-replica parameters are not built with diagnostics (grlx_set_diag)");
  if (c.replicas_per_wave != 0 && c.replicas_per_wave != 4 && c.replicas_per_wave != 8)
    return fail(GRLX_ERR_INVALID, "per-replica parameters are built for replicas_per_wave 0, 4 or 8 (%d is not)", c.replicas_per_wave);
  return GRLX_OK;
}
} // namespace

// diagnostic (include/grlx_diag.h): what a context of this configuration would launch on a device of `simds` SIMDs -- the validation of
// grlx_create, the layout choice and plan_rollout, without a device
int grlx_kernel_plan(const grlx_config *cfg, int simds, int flags, int *replicas_per_wave, int *variant, int *grid, char *rollout_name,
                     char *server_name, size_t name_cap)
{
  if (!cfg || simds < 1) return fail(GRLX_ERR_INVALID, "bad argument");
  DevParams P;
  int rc = admit(cfg, &P);
  if (rc != GRLX_OK) return rc;
  const Layout L = choose_layout(*cfg, simds);
  P.replicas_per_wave = L.replicas_per_wave;
  P.wave_limit = L.wave_limit;
  const int stamps = flags & (GRLX_PLAN_STAMPS_IN_PLACE | GRLX_PLAN_STAMPS_DEFERRED);
  if (stamps == GRLX_PLAN_STAMPS_DEFERRED && cfg->trace == GRLX_TRACE_NONE)
    return fail(GRLX_ERR_INVALID, "stamps of the production ordering are not built for a context without a trace");
  static unsigned long long no_stamps_here;          // grlx_set_diag: the plan only asks whether the pointer is set
  if (stamps) P.diag_out = &no_stamps_here;
  P.diag_deferred = stamps == GRLX_PLAN_STAMPS_DEFERRED ? 1 : 0;
  if (flags & GRLX_PLAN_SWEEP)
  { // grlx_set_replica_params
    if ((rc = sweep_admits(*cfg, P)) != GRLX_OK) return rc;
    if (P.replicas_per_wave > 8) P.replicas_per_wave = 8;
  }
  PlanFacts facts;
  facts.sweep = (flags & GRLX_PLAN_SWEEP) || (L.no_trace_td && !records(P));
  facts.ac_in_place = L.no_trace_ac;
  facts.server = !(flags & GRLX_PLAN_SERVER_OFF);
  facts.walker_server = (flags & GRLX_PLAN_WALKER_SERVER) != 0;
  facts.fits = (flags & GRLX_PLAN_FITS_YES) ? +[](const KernelRow &) { return true; } :
               (flags & GRLX_PLAN_FITS_NO) ? +[](const KernelRow &) { return false; } : waves_fit_together;
  if (cfg->env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "this context has no environment (GRLX_ENV_EXTERNAL): it launches no rollout kernel");
  const KernelPlan plan = plan_rollout(P, facts);
  if (!plan.row) return fail(GRLX_ERR_INVALID, "no rollout kernel is built for this launch");
  if (replicas_per_wave) *replicas_per_wave = P.replicas_per_wave;
  if (variant) *variant = plan.row->variant;
  if (grid) *grid = (int)plan.grid;
  if (rollout_name && name_cap) snprintf(rollout_name, name_cap, "%s", plan.row->name);
  if (server_name && name_cap) snprintf(server_name, name_cap, "%s", plan.server ? plan.row->server_name : "");
  return GRLX_OK;
}

int grlx_get_replica_params(grlx_ctx *ctx, int param, double *values)
{
  if (!ctx || !values) return fail(GRLX_ERR_INVALID, "null argument");
  if (param < 0 || param > 3) return fail(GRLX_ERR_INVALID, "param %d is not one of GRLX_PARAM_*", param);
  const size_t N = (size_t)ctx->P.n_replicas;
  for (size_t r = 0; r < N; ++r) values[r] = ctx->sweep_host[param].empty() ? sweep_config_value(ctx, param) : ctx->sweep_host[param][r];
  return GRLX_OK;
}

int grlx_set_replica_params(grlx_ctx *ctx, int param, const double *values)
{
  if (!ctx || !values) return fail(GRLX_ERR_INVALID, "null argument");
  if (param < 0 || param > 3) return fail(GRLX_ERR_INVALID, "param %d is not one of GRLX_PARAM_*", param);
  if (ctx->launched) return fail(GRLX_ERR_INVALID, "grlx_set_replica_params is allowed only before the first launch of the context");
  int rc = sweep_admits(ctx->cfg, ctx->P);
  if (rc != GRLX_OK) return rc;
  const size_t N = (size_t)ctx->P.n_replicas;
  // the four values of every replica with this call applied, validated as make_params validates the shared ones
  std::vector<double> v[4];
  for (int k = 0; k < 4; ++k)
  {
    v[k].resize(N);
    rc = grlx_get_replica_params(ctx, k, v[k].data());
    if (rc != GRLX_OK) return rc;
  }
  v[param].assign(values, values + N);
  std::vector<SweepParams> rec(N);
  for (size_t r = 0; r < N; ++r)
  {
    const int rc_r = sweep_record(ctx->cfg, r, v[GRLX_PARAM_ALPHA][r], v[GRLX_PARAM_GAMMA][r], v[GRLX_PARAM_LAMBDA][r], v[GRLX_PARAM_EPSILON][r], param, &rec[r]);
    if (rc_r != GRLX_OK) return rc_r;
  }
  if (!ctx->sweep_dev)
  {
    hipError_t e = hipMalloc((void **)&ctx->sweep_dev, sizeof(SweepParams) * N);
    if (e != hipSuccess)
    {
      ctx->sweep_dev = nullptr;
      return fail(e == hipErrorOutOfMemory ? GRLX_ERR_OOM : GRLX_ERR_HIP, "hipMalloc of the per-replica parameters failed: %s", hipGetErrorString(e));
    }
  }
  HIP_TRY(hipMemcpy(ctx->sweep_dev, rec.data(), sizeof(SweepParams) * N, hipMemcpyHostToDevice));
  ctx->sweep_host[param] = std::move(v[param]);
  ctx->sweep = true;
  // the layouts of more than 8 replicas per wave are not built for a sweep: the automatic choice falls back to 8
  if (ctx->P.replicas_per_wave > 8) ctx->P.replicas_per_wave = 8;
  return GRLX_OK;
}

int grlx_curve_stats(grlx_ctx *ctx, int first, int count, double *out_dev, void *stream)
{
  if (!ctx || !out_dev || first < 0 || count < 0 || first + count > ctx->P.max_rows) return fail(GRLX_ERR_INVALID, "bad argument");
  if ((hipStream_t)stream != ctx->run_stream) DRAIN(ctx);
  HIP_TRY(launch_curve_stats(ctx->P, first, count, out_dev, (hipStream_t)stream));
  return GRLX_OK;
}

int grlx_get_env_state(grlx_ctx *ctx, int replica, double *state)
{
  if (!ctx || !state || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(&s, ctx->states + replica, sizeof(s), hipMemcpyDeviceToHost));
  memcpy(state, s.x, sizeof(double) * GRLX_MAX_STATE);
  return GRLX_OK;
}

int grlx_get_rng(grlx_ctx *ctx, int replica, uint64_t out[4])
{
  if (!ctx || !out || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(&s, ctx->states + replica, sizeof(s), hipMemcpyDeviceToHost));
  out[0] = s.G; out[1] = s.TL; out[2] = s.S1; out[3] = s.S2;
  return GRLX_OK;
}

int grlx_table_load(grlx_ctx *ctx, int table, int replica, uint32_t *n_slots_used)
{
  if (!ctx || !n_slots_used || table < 0 || table >= ctx->n_tables || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(&s, ctx->states + replica, sizeof(s), hipMemcpyDeviceToHost));
  *n_slots_used = s.n_slots[table];
  return GRLX_OK;
}

int grlx_get_target_weights(grlx_ctx *ctx, int replica, const uint32_t *slots, int n, double *out, uint32_t *n_syncs)
{
  if (!ctx || !slots || !out || n < 0 || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.target_interval <= 0) return fail(GRLX_ERR_INVALID, "this context has no target network (target_interval = 0)");
  DRAIN(ctx);
  if (n_syncs)
  {
    ReplicaState s;
    HIP_TRY(hipMemcpy(&s, ctx->states + replica, sizeof(s), hipMemcpyDeviceToHost));
    *n_syncs = s.syncs;
  }
  if (n == 0) return GRLX_OK;
  DevBuf ds, dout;
  HIP_TRY(ds.alloc(sizeof(uint32_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(hipMemcpy(ds.p, slots, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_get_target_weights(ctx->P, replica, ds.as<uint32_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_read_taps(grlx_ctx *ctx, grlx_tap *out, int cap, int *n)
{
  if (!ctx || !out || !n) return fail(GRLX_ERR_INVALID, "bad argument");
  uint32_t cnt = 0;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(&cnt, ctx->tap_count, sizeof(cnt), hipMemcpyDeviceToHost));
  int m = (int)cnt < cap ? (int)cnt : cap;
  if (m > ctx->P.tap_capacity) m = ctx->P.tap_capacity;
  if (m > 0) HIP_TRY(hipMemcpy(out, ctx->taps, sizeof(grlx_tap) * (size_t)m, hipMemcpyDeviceToHost));
  *n = m;
  return GRLX_OK;
}

int grlx_get_weights(grlx_ctx *ctx, int table, int replica, const uint32_t *slots, int n, double *out)
{
  if (!ctx || !slots || !out || n < 0 || table < 0 || table >= ctx->n_tables || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  if (n == 0) return GRLX_OK;
  DRAIN(ctx);
  DevBuf ds, dout;
  HIP_TRY(ds.alloc(sizeof(uint32_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(hipMemcpy(ds.p, slots, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_get_weights(ctx->P, table, replica, ds.as<uint32_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_export_weights(grlx_ctx *ctx, int table, int replica, double *out)
{
  if (!ctx || !out || table < 0 || table >= ctx->n_tables || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  const size_t memory = (size_t)(table == 1 ? ctx->P.tile_actor.memory : ctx->P.tile.memory);
  DRAIN(ctx);
  DevBuf dout;
  HIP_TRY(dout.alloc(sizeof(double) * memory));
  HIP_TRY(launch_export_weights(ctx->P, table, replica, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * memory, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_load_weights(grlx_ctx *ctx, int table, int first_replica, int n_replicas, const double *dense, uint64_t count)
{
  if (!ctx || !dense || table < 0 || table >= ctx->n_tables) return fail(GRLX_ERR_INVALID, "bad argument");
  const int N = ctx->P.n_replicas;
  if (first_replica < 0 || n_replicas < 0 || first_replica > N || n_replicas > N - first_replica)
    return fail(GRLX_ERR_INVALID, "replica range [%d, %d) outside [0, %d)", first_replica, first_replica + n_replicas, N);
  const size_t memory = (size_t)(table == 1 ? ctx->P.tile_actor.memory : ctx->P.tile.memory);
  if (count != (uint64_t)memory)                       // representation.h:247-252 "Configuration mismatch"
    return fail(GRLX_ERR_INVALID, "configuration mismatch: %llu weights given, the table has %zu", (unsigned long long)count, memory);
  if (ctx->cfg.agent == GRLX_AGENT_AC && ctx->trials_run != 0)
    return fail(GRLX_ERR_INVALID, "actor-critic: load before the first run (the critic's trace refers to table positions)");
  // a target network (table 0 of a SARSA / Q context): setParams is followed by synchronize() (representation.h:256-257) -- target <- tau * image
  // + (1 - tau) * target over the WHOLE parameter vector.  With tau = 0 the target is the image; otherwise every replica needs its own dense
  // vector of the result (its old target differs), `memory` doubles each, held until the next load or reset.
  const bool with_target = ctx->cfg.target_interval > 0 && table == 0;
  const bool target_images = with_target && ctx->cfg.target_tau != 0.;
  if (target_images && (double)n_replicas * (double)memory * sizeof(double) > 8.0 * 1024 * 1024 * 1024)
    return fail(GRLX_ERR_OOM, "loading into a target network with tau != 0 keeps one dense target vector per replica (%zu doubles each): %d replicas exceed the 8 GiB this entry point allows",
                memory, n_replicas);
  if (n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  ctx->run_pending = false;
  double *img = nullptr;
  if (hipMalloc((void **)&img, sizeof(double) * memory) != hipSuccess) return fail(GRLX_ERR_OOM, "no device memory for a %zu-weight policy image", memory);
  // (a target network with tau != 0: one new dense vector per replica, allocated before anything is touched -- a failure leaves the context as it was)
  std::vector<double *> fresh((size_t)n_replicas, nullptr);
  if (target_images)
    for (int k = 0; k < n_replicas; ++k)
      if (hipMalloc((void **)&fresh[(size_t)k], sizeof(double) * memory) != hipSuccess)
      {
        (void)hipGetLastError();
        for (double *t : fresh)
          if (t) (void)hipFree(t);
        (void)hipFree(img);
        return fail(GRLX_ERR_OOM, "no device memory for the target vector of replica %d", first_replica + k);
      }
  ctx->images.push_back(img);
  {
    std::vector<int> &of = ctx->image_of[table];
    if (of.empty()) of.assign((size_t)N, -1);
    const int mine = (int)ctx->images.size() - 1;
    for (int r = first_replica; r < first_replica + n_replicas; ++r) of[(size_t)r] = mine;
  }
  HIP_TRY(hipMemcpy(img, dense, sizeof(double) * memory, hipMemcpyHostToDevice));
  if (with_target)
  { // the target's new values, from its values NOW (entries and lazily defined ones alike), BEFORE the tables are emptied
    if (ctx->target_images.empty()) ctx->target_images.assign((size_t)N, nullptr);
    std::vector<ReplicaState> hs((size_t)n_replicas);
    HIP_TRY(hipMemcpy(hs.data(), ctx->states + first_replica, sizeof(ReplicaState) * (size_t)n_replicas, hipMemcpyDeviceToHost));
    if (target_images)
      for (int k = 0; k < n_replicas; ++k) HIP_TRY(launch_target_after_load(ctx->P, first_replica + k, img, fresh[(size_t)k], nullptr));
    HIP_TRY(hipDeviceSynchronize());          // (the kernels read the vectors of an earlier load for the last time)
    for (int k = 0; k < n_replicas; ++k)
    {
      const int r = first_replica + k;
      if (ctx->target_images[(size_t)r]) (void)hipFree(ctx->target_images[(size_t)r]);
      ctx->target_images[(size_t)r] = fresh[(size_t)k];
      hs[(size_t)k].target_base = fresh[(size_t)k];
      hs[(size_t)k].syncs += 1;                     // the load's synchronize() (count_ = 0, representation.h:284-296)
      hs[(size_t)k].syncs_base = hs[(size_t)k].syncs;
      hs[(size_t)k].sync_count = 0;
    }
    HIP_TRY(hipMemcpy(ctx->states + first_replica, hs.data(), sizeof(ReplicaState) * (size_t)n_replicas, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(ctx->tvals + ((size_t)first_replica << ctx->P.logC), 0xFF, ((size_t)n_replicas * sizeof(double)) << ctx->P.logC));      // kTvalUnset
  }
  // setParams() overwrites every weight: forget the sparse tables of these replicas; every slot is
  // re-created on first touch from the image
  const size_t per_replica = sizeof(Entry) << ctx->P.logC;
  Entry *base = ctx->tables + (((size_t)table * (size_t)N + (size_t)first_replica) << ctx->P.logC);
  if (ctx->P.twin_tables)      // twin tables keep their common key layout: the entries stay and take their values from the image
    HIP_TRY(launch_reload_entries(ctx->P, table, first_replica, n_replicas, img, nullptr));
  else
    HIP_TRY(hipMemset(base, 0, per_replica * (size_t)n_replicas));
  HIP_TRY(launch_set_lazy_base(ctx->P, table, first_replica, n_replicas, img, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  // an earlier image that no replica of any table refers to any more goes now (repeated loads do not accumulate)
  for (size_t k = 0; k + 1 < ctx->images.size(); ++k)
  {
    if (!ctx->images[k]) continue;
    bool used = false;
    for (int t = 0; t < 2 && !used; ++t)
      for (int v : ctx->image_of[t])
        if (v == (int)k) { used = true; break; }
    if (!used)
    {
      (void)hipFree(ctx->images[k]);
      ctx->images[k] = nullptr;
    }
  }
  return GRLX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The per-step plug-in interfaces on a context's replicas (grlx_step.h).  Host pointers; each call copies its arguments in,
// launches one kernel over all replicas and copies the results out.
static int step_buffers(grlx_ctx *ctx)
{
  if (ctx->stage_f64) return GRLX_OK;
  const size_t N = (size_t)ctx->P.n_replicas;
  if (hipMalloc((void **)&ctx->stage_f64, sizeof(double) * N * (GRLX_MAX_DIMS + 2)) != hipSuccess ||
      hipMalloc((void **)&ctx->stage_i32, sizeof(int32_t) * N * 2) != hipSuccess)
  {
    (void)hipGetLastError();
    if (ctx->stage_f64) (void)hipFree(ctx->stage_f64);
    ctx->stage_f64 = nullptr;
    return fail(GRLX_ERR_OOM, "no device memory for the staging buffers of the per-step entry points");
  }
  return GRLX_OK;
}

static const int32_t *stage_active(grlx_ctx *ctx, const int32_t *active, hipError_t *err)
{
  *err = hipSuccess;
  if (!active) return nullptr;
  *err = hipMemcpy(ctx->stage_i32, active, sizeof(int32_t) * (size_t)ctx->P.n_replicas, hipMemcpyHostToDevice);
  return ctx->stage_i32;
}

#define SWEEP_REFUSES(ctx, what)                                                                                                  \
  do {                                                                                                                            \
    if ((ctx) && (ctx)->sweep)                                                                                                    \
      return fail(GRLX_ERR_INVALID, what " is not built for a sweep context (grlx_set_replica_params): it would run on the shared values"); \
  } while (0)

int grlx_env_start(grlx_ctx *ctx, int test, const int32_t *active, double *obs)
{
  SWEEP_REFUSES(ctx, "grlx_env_start");
  if (!ctx || !obs) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "this context has no environment (GRLX_ENV_EXTERNAL)");
  DRAIN(ctx);
  ctx->launched = true;
  int rc = step_buffers(ctx);
  if (rc != GRLX_OK) return rc;
  const size_t N = (size_t)ctx->P.n_replicas, D = (size_t)ctx->D;
  hipError_t e;
  const int32_t *act = stage_active(ctx, active, &e);
  HIP_TRY(e);
  if (active) HIP_TRY(hipMemcpy(ctx->stage_f64, obs, sizeof(double) * N * D, hipMemcpyHostToDevice));     // inactive rows keep the caller's values
  HIP_TRY(launch_env_start(ctx->P, test ? 1 : 0, act, ctx->stage_f64, nullptr));
  HIP_TRY(hipMemcpy(obs, ctx->stage_f64, sizeof(double) * N * D, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_env_advance(grlx_ctx *ctx, const int32_t *active, const double *action, double *obs, double *reward, int32_t *terminal)
{
  SWEEP_REFUSES(ctx, "grlx_env_advance");
  if (!ctx || !action || !obs || !reward || !terminal) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "this context has no environment (GRLX_ENV_EXTERNAL)");
  DRAIN(ctx);
  ctx->launched = true;
  int rc = step_buffers(ctx);
  if (rc != GRLX_OK) return rc;
  const size_t N = (size_t)ctx->P.n_replicas, D = (size_t)ctx->D;
  double *d_obs = ctx->stage_f64, *d_reward = d_obs + N * GRLX_MAX_DIMS, *d_action = d_reward + N;
  int32_t *d_term = ctx->stage_i32 + N;
  hipError_t e;
  const int32_t *act = stage_active(ctx, active, &e);
  HIP_TRY(e);
  if (active)
  { // inactive rows keep the caller's values
    HIP_TRY(hipMemcpy(d_obs, obs, sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_reward, reward, sizeof(double) * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_term, terminal, sizeof(int32_t) * N, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(d_action, action, sizeof(double) * N, hipMemcpyHostToDevice));
  HIP_TRY(launch_env_advance(ctx->P, act, d_action, d_obs, d_reward, d_term, nullptr));
  HIP_TRY(hipMemcpy(obs, d_obs, sizeof(double) * N * D, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(reward, d_reward, sizeof(double) * N, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(terminal, d_term, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  uint64_t h[3];                                        // a state outside the sine's domain is reported at once, as grlx_env_step does
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch, nullptr));
  HIP_TRY(hipMemcpy(h, ctx->scratch, sizeof(h), hipMemcpyDeviceToHost));
  return status_to_error(h[2] & ST_DOMAIN);
}

// the agent kinds the per-step kernels are built for, and the state they keep between calls
static int agent_ready(grlx_ctx *ctx)
{
  const grlx_config &c = ctx->cfg;
  const bool td = is_td_agent(c.agent);
  if (!(td || c.agent == GRLX_AGENT_AC) || c.trace == GRLX_TRACE_ACCUMULATING || c.target_interval > 0 || c.projector.safe != 0 ||
      (td && c.action_steps != 3 && c.action_steps != 5))
    return fail(GRLX_ERR_INVALID, "the per-step agent entry points are built for agent/td with predictor/critic/{sarsa, q, expected_sarsa} (3 or 5 actions, "
                                  "replacing or no trace, no target network, safe = 0) and for the actor-critic agent");
  if (ctx->P.tap_capacity > 0 || ctx->P.diag_out) return fail(GRLX_ERR_INVALID, "the per-step agent entry points are not available with taps or diagnostics");
  if (ctx->agent_rep) return GRLX_OK;
  const size_t N = (size_t)ctx->P.n_replicas;
  int rc = step_buffers(ctx);
  if (rc != GRLX_OK) return rc;
  if (!ctx->trace_state)
  { // the predictor's trace between calls, in the layout the actor-critic kernels persist theirs in: empty
    const size_t words = N * 16 * kMaxTrace * 2;
    if (hipMalloc((void **)&ctx->trace_state, words * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); ctx->trace_state = nullptr; return fail(GRLX_ERR_OOM, "no device memory for the agents' traces"); }
    std::vector<uint32_t> init(words, 0u);
    for (size_t i = 0; i < words; i += 2) init[i] = kInvalidPos;
    HIP_TRY(hipMemcpy(ctx->trace_state, init.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->P.trace_state = ctx->trace_state;
  }
  if (hipMalloc((void **)&ctx->agent_lane, sizeof(uint32_t) * N * 16 * 2) != hipSuccess) { (void)hipGetLastError(); ctx->agent_lane = nullptr; return fail(GRLX_ERR_OOM, "no device memory for the agents' state"); }
  HIP_TRY(hipMemset(ctx->agent_lane, 0, sizeof(uint32_t) * N * 16 * 2));
  if (hipMalloc((void **)&ctx->agent_rep, sizeof(AgentRep) * N) != hipSuccess) { (void)hipGetLastError(); ctx->agent_rep = nullptr; return fail(GRLX_ERR_OOM, "no device memory for the agents' state"); }
  HIP_TRY(hipMemset(ctx->agent_rep, 0, sizeof(AgentRep) * N));
  ctx->P.agent_rep = ctx->agent_rep;
  ctx->P.agent_lane = ctx->agent_lane;
  return GRLX_OK;
}

static int agent_call(grlx_ctx *ctx, int mode, int test, const int32_t *active, double tau, const double *obs, const double *reward,
                      const int32_t *terminal, double *action)
{
  SWEEP_REFUSES(ctx, "grlx_agent_start / _step / _end");
  if (!ctx || !obs || (mode != STEP_START && !reward) || (mode != STEP_END && !action)) return fail(GRLX_ERR_INVALID, "bad argument");
  if (mode != STEP_START && tau != 1.) return fail(GRLX_ERR_INVALID, "Agent::step / end: tau must be 1 (environment/modeled:discrete_time = 1)");
  DRAIN(ctx);
  int rc = agent_ready(ctx);
  if (rc != GRLX_OK) return rc;
  ctx->launched = true;
  // the tables these calls fill grow like the fused path's: looked at every 64 calls, between two calls
  if ((ctx->step_calls++ & 63u) == 63u && ctx->P.logC < ctx->logC_max)
  {
    uint32_t used = 0;
    HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load, nullptr));
    HIP_TRY(hipMemcpy(&used, ctx->max_load, sizeof(used), hipMemcpyDeviceToHost));
    if ((uint64_t)used * 4u > (1ull << ctx->P.logC))
    {
      uint32_t want = ctx->P.logC;
      while ((uint64_t)used * 8u > (1ull << want) && want < ctx->logC_max) ++want;
      rc = grow_tables(ctx, want);
      if (rc == GRLX_ERR_OOM) { g_err.clear(); ctx->logC_max = ctx->P.logC; }
      else if (rc != GRLX_OK) return rc;
    }
  }
  const size_t N = (size_t)ctx->P.n_replicas;
  const size_t D = (size_t)(ctx->cfg.agent == GRLX_AGENT_AC ? ctx->P.tile.D : ctx->P.tile.D - 1);
  double *d_obs = ctx->stage_f64, *d_reward = d_obs + N * GRLX_MAX_DIMS, *d_action = d_reward + N;
  int32_t *d_term = ctx->stage_i32 + N;
  StepArgs A;
  A.mode = mode;
  A.test = test ? 1 : 0;
  hipError_t e;
  A.active = stage_active(ctx, active, &e);
  HIP_TRY(e);
  HIP_TRY(hipMemcpy(d_obs, obs, sizeof(double) * N * D, hipMemcpyHostToDevice));
  A.obs = d_obs;
  A.reward = d_reward;
  if (mode != STEP_START) HIP_TRY(hipMemcpy(d_reward, reward, sizeof(double) * N, hipMemcpyHostToDevice));
  A.terminal = nullptr;
  if (mode == STEP_STEP && terminal)
  {
    HIP_TRY(hipMemcpy(d_term, terminal, sizeof(int32_t) * N, hipMemcpyHostToDevice));
    A.terminal = d_term;
  }
  A.action = d_action;
  if (mode != STEP_END) HIP_TRY(hipMemcpy(d_action, action, sizeof(double) * N, hipMemcpyHostToDevice));    // rows that do not act keep the caller's values
  if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
  HIP_TRY(launch_agent_step(ctx->P, A, nullptr));
  if (mode != STEP_END) HIP_TRY(hipMemcpy(action, d_action, sizeof(double) * N, hipMemcpyDeviceToHost));
  else HIP_TRY(hipDeviceSynchronize());
  return GRLX_OK;
}

int grlx_agent_start(grlx_ctx *ctx, int test, const int32_t *active, const double *obs, double *action)
{
  return agent_call(ctx, STEP_START, test, active, 0., obs, nullptr, nullptr, action);
}

int grlx_agent_step(grlx_ctx *ctx, int test, const int32_t *active, double tau, const double *obs, const double *reward, const int32_t *terminal, double *action)
{
  return agent_call(ctx, STEP_STEP, test, active, tau, obs, reward, terminal, action);
}

int grlx_agent_end(grlx_ctx *ctx, int test, const int32_t *active, double tau, const double *obs, const double *reward)
{
  return agent_call(ctx, STEP_END, test, active, tau, obs, reward, nullptr, nullptr);
}

int grlx_project(const grlx_tile_spec *spec, const double *in, int n, uint32_t *out)
{
  if (!spec || !in || !out || n < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  TileParams tp;
  int rc = make_tile_params(*spec, &tp);
  if (rc != GRLX_OK) return rc;
  if (spec->safe != 0) return fail(GRLX_ERR_INVALID, "grlx_project is stateless: projector/tile_coding:safe needs the claim table of a context");
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  DevBuf din, dout;
  HIP_TRY(din.alloc(sizeof(double) * (size_t)n * (size_t)tp.D));
  HIP_TRY(dout.alloc(sizeof(uint32_t) * (size_t)n * (size_t)tp.T));
  HIP_TRY(hipMemcpy(din.p, in, sizeof(double) * (size_t)n * (size_t)tp.D, hipMemcpyHostToDevice));
  HIP_TRY(launch_project(tp, din.as<double>(), n, dout.as<uint32_t>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(uint32_t) * (size_t)n * (size_t)tp.T, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_env_step(const grlx_config *cfg, double *state, const double *action, int n, double *obs, double *reward, int32_t *terminal)
{
  if (!cfg || !state || !action || !obs || !reward || !terminal || n < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  if (cfg->env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "GRLX_ENV_EXTERNAL is the caller's environment: nothing to step here");
  DevParams P;
  int rc = make_params(*cfg, &P);
  if (rc != GRLX_OK) return rc;
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  int S, D;
  env_dims(cfg->env, &S, &D);
  DevBuf ds, da, dobs, dr, dt, derr;
  HIP_TRY(ds.alloc(sizeof(double) * (size_t)n * S));
  HIP_TRY(da.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dobs.alloc(sizeof(double) * (size_t)n * D));
  HIP_TRY(dr.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dt.alloc(sizeof(int32_t) * (size_t)n));
  HIP_TRY(derr.alloc(sizeof(uint32_t)));
  HIP_TRY(hipMemset(derr.p, 0, sizeof(uint32_t)));
  HIP_TRY(hipMemcpy(ds.p, state, sizeof(double) * (size_t)n * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(da.p, action, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_env_step(P, ds.as<double>(), da.as<double>(), n, dobs.as<double>(), dr.as<double>(), dt.as<int32_t>(), derr.as<uint32_t>(), nullptr));
  HIP_TRY(hipMemcpy(state, ds.p, sizeof(double) * (size_t)n * S, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(obs, dobs.p, sizeof(double) * (size_t)n * D, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(reward, dr.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(terminal, dt.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  uint32_t err = 0;
  HIP_TRY(hipMemcpy(&err, derr.p, sizeof(err), hipMemcpyDeviceToHost));
  if (err & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "environment state left the supported domain (NaN)");
  return GRLX_OK;
}

static int table_op(grlx_ctx *ctx, int table, int op, const int32_t *replica, const uint32_t *idx, int n,
                    const double *arg, double alpha, double *out)
{
  if (!ctx || !replica || !idx || n < 0 || table < 0 || table >= ctx->n_tables) return fail(GRLX_ERR_INVALID, "bad argument");
  if (n == 0) return GRLX_OK;
  for (int i = 0; i < n; ++i)
    if (replica[i] < 0 || replica[i] >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "replica index out of range");
  const int T = ctx->P.tile.T;
  const uint32_t mem = (uint32_t)(table == 1 ? ctx->P.tile_actor.memory : ctx->P.tile.memory);
  for (size_t i = 0; i < (size_t)n * (size_t)T; ++i)
    if (idx[i] != 0xFFFFFFFFu && idx[i] >= mem) return fail(GRLX_ERR_INVALID, "slot index out of range");
  DRAIN(ctx);
  DevBuf dr, di, da, dout;
  HIP_TRY(dr.alloc(sizeof(int32_t) * (size_t)n));
  HIP_TRY(di.alloc(sizeof(uint32_t) * (size_t)n * T));
  HIP_TRY(da.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(hipMemcpy(dr.p, replica, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di.p, idx, sizeof(uint32_t) * (size_t)n * T, hipMemcpyHostToDevice));
  if (arg) HIP_TRY(hipMemcpy(da.p, arg, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_table_op(ctx->P, table, op, dr.as<int32_t>(), di.as<uint32_t>(), n, da.as<double>(), alpha, dout.as<double>(), nullptr));
  if (out) HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return GRLX_OK;
}

int grlx_read(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n, double *out)
{
  if (!out) return fail(GRLX_ERR_INVALID, "bad argument");
  return table_op(ctx, table, 0, replica, idx, n, nullptr, 0, out);
}

int grlx_write(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n, const double *target, double alpha)
{
  if (!target) return fail(GRLX_ERR_INVALID, "bad argument");
  return table_op(ctx, table, 1, replica, idx, n, target, alpha, nullptr);
}

int grlx_update(grlx_ctx *ctx, int table, const int32_t *replica, const uint32_t *idx, int n, const double *delta)
{
  if (!delta) return fail(GRLX_ERR_INVALID, "bad argument");
  return table_op(ctx, table, 2, replica, idx, n, delta, 0, nullptr);
}

// ------------------------------------------------------------------------------------------- policy queries ---
} // extern "C"
namespace {

constexpr uint64_t kQueryChunkDefault = 256ull << 20;
uint64_t g_query_chunk_bytes = kQueryChunkDefault;

bool q_agent(int agent) { return agent != GRLX_AGENT_AC; }      // every other agent acts through a policy/discrete/q on table 0

// what every query checks before it touches the device; tp: the projector of the table read, obs_dims: its share of the observation
int query_admit(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *obs, int n_obs, const TileParams &tp, int obs_dims)
{
  if (ctx->P.tile_safe >= 1)
    return fail(GRLX_ERR_INVALID, "%s is not built for projector/tile_coding:safe >= 1 (a read would have to walk the claim table without claiming)", who);
  if (n_obs < 0) return fail(GRLX_ERR_INVALID, "%s: n_obs = %d", who, n_obs);
  if (first_replica < 0 || n_replicas < 0 || (int64_t)first_replica + n_replicas > ctx->P.n_replicas)
    return fail(GRLX_ERR_INVALID, "%s: replica range [%d, %lld) is outside the context's %d replicas", who, first_replica,
                (long long)first_replica + n_replicas, ctx->P.n_replicas);
  if (!obs) return fail(GRLX_ERR_INVALID, "%s: obs is null", who);
  for (int o = 0; o < n_obs; ++o)
    for (int i = 0; i < obs_dims; ++i)
    { // tile_quant casts floor(x * scaling) to int (tile_coding.cpp:121-125)
      const double x = obs[(size_t)o * obs_dims + i];
      if (!std::isfinite(x)) return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d is not finite (%g)", who, o, i, x);
      if (!(fabs(x * tp.scaling[i]) < 1073741824.))
        return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d (%g) is out of range: |x * scaling| reaches 2^30", who, o, i, x);
    }
  return GRLX_OK;
}

// observations per chunk so that one chunk's device arrays stay within the bound; at least one
int query_chunk(int n_obs, size_t bytes_per_obs)
{
  const uint64_t fit = g_query_chunk_bytes / (bytes_per_obs ? bytes_per_obs : 1);
  return (int)(fit < 1 ? 1 : fit > (uint64_t)n_obs ? (uint64_t)n_obs : fit);
}

// rows [n_replicas] of `width` bytes each: device [r][chunk] -> host [r][n_obs] at observation o0
hipError_t query_copy_out(void *host, const void *dev, size_t elem, int n_replicas, int n_obs, int o0, int nc)
{
  return hipMemcpy2D((char *)host + (size_t)o0 * elem, (size_t)n_obs * elem, dev, (size_t)nc * elem, (size_t)nc * elem, (size_t)n_replicas,
                     hipMemcpyDeviceToHost);
}

int query_q_impl(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas, int group_size, const double *obs, int n_obs,
                 double *q, double *value, int32_t *greedy, int32_t *n_max, double *ensemble)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!q_agent(ctx->cfg.agent)) return fail(GRLX_ERR_INVALID, "%s serves agents with a policy/discrete/q; the actor-critic's tables are read by grlx_query_state", who);
  const int NA = ctx->P.A, D = ctx->P.tile.D - 1;
  if (NA != 3 && NA != 5) return fail(GRLX_ERR_INVALID, "%s is not built for %d actions (3 or 5)", who, NA);
  int rc = query_admit(ctx, who, first_replica, n_replicas, obs, n_obs, ctx->P.tile, D);
  if (rc != GRLX_OK) return rc;
  if (ensemble && (group_size < 1 || n_replicas % group_size != 0))
    return fail(GRLX_ERR_INVALID, "%s: group_size %d does not divide the %d replicas", who, group_size, n_replicas);
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  const int n_groups = ensemble ? n_replicas / group_size : 0, cols = 2 + 2 * NA;
  const size_t per_pair = sizeof(double) * (size_t)NA + sizeof(double) + 2 * sizeof(int32_t);
  const int chunk = query_chunk(n_obs, sizeof(double) * (size_t)D + per_pair * (size_t)n_replicas + sizeof(double) * (size_t)cols * (size_t)n_groups);
  DevBuf dobs, dq, dv, dg, dn, de;
  const size_t pairs = (size_t)n_replicas * (size_t)chunk;
  HIP_TRY(dobs.alloc(sizeof(double) * (size_t)chunk * D));
  if (q || ensemble) HIP_TRY(dq.alloc(sizeof(double) * pairs * NA));
  if (value || ensemble) HIP_TRY(dv.alloc(sizeof(double) * pairs));
  if (greedy || ensemble) HIP_TRY(dg.alloc(sizeof(int32_t) * pairs));
  if (n_max) HIP_TRY(dn.alloc(sizeof(int32_t) * pairs));
  if (ensemble) HIP_TRY(de.alloc(sizeof(double) * (size_t)n_groups * chunk * cols));
  for (int o0 = 0; o0 < n_obs; o0 += chunk)
  {
    const int nc = n_obs - o0 < chunk ? n_obs - o0 : chunk;
    HIP_TRY(hipMemcpy(dobs.p, obs + (size_t)o0 * D, sizeof(double) * (size_t)nc * D, hipMemcpyHostToDevice));
    QueryArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.n_obs = nc;
    A.obs = dobs.as<double>(); A.q = dq.as<double>(); A.value = dv.as<double>(); A.greedy = dg.as<int32_t>(); A.n_max = dn.as<int32_t>();
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
    HIP_TRY(launch_query_q(ctx->P, A, nullptr));
    if (ensemble)
    {
      HIP_TRY(launch_query_reduce(NA, n_groups, group_size, nc, A.q, A.value, A.greedy, de.as<double>(), nullptr));
      HIP_TRY(query_copy_out(ensemble, de.p, sizeof(double) * cols, n_groups, n_obs, o0, nc));
    }
    if (q) HIP_TRY(query_copy_out(q, dq.p, sizeof(double) * NA, n_replicas, n_obs, o0, nc));
    if (value) HIP_TRY(query_copy_out(value, dv.p, sizeof(double), n_replicas, n_obs, o0, nc));
    if (greedy) HIP_TRY(query_copy_out(greedy, dg.p, sizeof(int32_t), n_replicas, n_obs, o0, nc));
    if (n_max) HIP_TRY(query_copy_out(n_max, dn.p, sizeof(int32_t), n_replicas, n_obs, o0, nc));
  }
  return GRLX_OK;
}

} // namespace
extern "C" {

int grlx_set_query_chunk_bytes(uint64_t bytes)
{
  g_query_chunk_bytes = bytes ? bytes : kQueryChunkDefault;
  set_fqi_query_chunk_bytes(bytes);
  return GRLX_OK;
}

int grlx_query_q(grlx_ctx *ctx, int first_replica, int n_replicas, const double *obs, int n_obs, double *q, double *value, int32_t *greedy, int32_t *n_max)
{
  return query_q_impl(ctx, "grlx_query_q", first_replica, n_replicas, 0, obs, n_obs, q, value, greedy, n_max, nullptr);
}

int grlx_query_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, const double *obs, int n_obs, double *out)
{
  if (!out) return fail(GRLX_ERR_INVALID, "bad argument");
  return query_q_impl(ctx, "grlx_query_ensemble", first_replica, n_replicas, group_size, obs, n_obs, nullptr, nullptr, nullptr, nullptr, out);
}

int grlx_query_state(grlx_ctx *ctx, int table, int first_replica, int n_replicas, const double *obs, int n_obs, double *out)
{
  if (!ctx || !out) return fail(GRLX_ERR_INVALID, "bad argument");
  if (table < 0 || table >= ctx->n_tables) return fail(GRLX_ERR_INVALID, "grlx_query_state: table %d (the context has %d)", table, ctx->n_tables);
  if (table == 0 && q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "grlx_query_state: table 0 of a Q agent takes (observation, action): use grlx_query_q");
  const TileParams &tp = table == 1 ? ctx->P.tile_actor : ctx->P.tile;
  int rc = query_admit(ctx, "grlx_query_state", first_replica, n_replicas, obs, n_obs, tp, tp.D);
  if (rc != GRLX_OK) return rc;
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  const int D = tp.D;
  const int chunk = query_chunk(n_obs, sizeof(double) * (size_t)D + sizeof(double) * (size_t)n_replicas);
  DevBuf dobs, dv;
  HIP_TRY(dobs.alloc(sizeof(double) * (size_t)chunk * D));
  HIP_TRY(dv.alloc(sizeof(double) * (size_t)n_replicas * (size_t)chunk));
  for (int o0 = 0; o0 < n_obs; o0 += chunk)
  {
    const int nc = n_obs - o0 < chunk ? n_obs - o0 : chunk;
    HIP_TRY(hipMemcpy(dobs.p, obs + (size_t)o0 * D, sizeof(double) * (size_t)nc * D, hipMemcpyHostToDevice));
    QueryArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.n_obs = nc;
    A.obs = dobs.as<double>(); A.q = nullptr; A.value = dv.as<double>(); A.greedy = nullptr; A.n_max = nullptr;
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
    HIP_TRY(launch_query_state(ctx->P, table, A, nullptr));
    HIP_TRY(query_copy_out(out, dv.p, sizeof(double), n_replicas, n_obs, o0, nc));
  }
  return GRLX_OK;
}

// ---- policy evaluation: greedy episodes from start states of the caller's choice (grlx_evaluate.hip) -----------------------------------
// what both evaluations check before they touch the device
static int evaluate_admit(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL)
    return fail(GRLX_ERR_INVALID, "%s: the context has no environment (GRLX_ENV_EXTERNAL): there is nothing to step", who);
  if (ctx->P.tile_safe >= 1)
    return fail(GRLX_ERR_INVALID, "%s is not built for projector/tile_coding:safe >= 1 (a read would have to walk the claim table without claiming)", who);
  if (!evaluate_built(ctx->cfg.agent, ctx->cfg.env, ctx->P.A))
    return fail(GRLX_ERR_INVALID, "%s is not built for environment %d with %d actions (Q agents: pendulum x {3, 5}, acrobot, cart-pole, walker x 3; actor-critic: cart-pole, pendulum)", who,
                ctx->cfg.env, ctx->cfg.agent == GRLX_AGENT_AC ? 0 : ctx->P.A);
  if (n_starts < 0) return fail(GRLX_ERR_INVALID, "%s: n_starts = %d", who, n_starts);
  if (first_replica < 0 || n_replicas < 0 || (int64_t)first_replica + n_replicas > ctx->P.n_replicas)
    return fail(GRLX_ERR_INVALID, "%s: replica range [%d, %lld) is outside the context's %d replicas", who, first_replica,
                (long long)first_replica + n_replicas, ctx->P.n_replicas);
  if (!states) return fail(GRLX_ERR_INVALID, "%s: states is null", who);
  if (max_steps < 0 || max_steps > GRLX_MAX_EPISODE_STEPS)
    return fail(GRLX_ERR_INVALID, "%s: max_steps = %d is outside 1 ... GRLX_MAX_EPISODE_STEPS (%d; 0 = that cap)", who, max_steps, GRLX_MAX_EPISODE_STEPS);
  const int S = ctx->S;
  for (int s = 0; s < n_starts; ++s)
    for (int i = 0; i < S; ++i)
    { // below 2^17 the RK4 stages of one step stay inside the branch-free sine's domain (the cart-pole's case)
      const double v = states[(size_t)s * S + i];
      if (!std::isfinite(v)) return fail(GRLX_ERR_INVALID, "%s: state row %d, component %d is not finite (%g)", who, s, i, v);
      if (!(fabs(v) < 0x1p17)) return fail(GRLX_ERR_INVALID, "%s: state row %d, component %d (%g) is out of range: its magnitude reaches 2^17", who, s, i, v);
    }
  return GRLX_OK;
}

int grlx_evaluate(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret, double *disc,
                  int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state)
{
  int rc = evaluate_admit(ctx, "grlx_evaluate", first_replica, n_replicas, states, n_starts, max_steps);
  if (rc != GRLX_OK) return rc;
  if (max_steps == 0) max_steps = GRLX_MAX_EPISODE_STEPS;
  const int S = ctx->S;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  const size_t per_pair = 2 * sizeof(double) + 3 * sizeof(int32_t) + sizeof(double) * (size_t)S;
  const int chunk = query_chunk(n_starts, sizeof(double) * (size_t)S + per_pair * (size_t)n_replicas);
  const size_t pairs = (size_t)n_replicas * (size_t)chunk;
  DevBuf dst, dret, ddisc, dsteps, dterm, dties, dfin;
  HIP_TRY(dst.alloc(sizeof(double) * (size_t)chunk * S));
  HIP_TRY(dret.alloc(sizeof(double) * pairs));
  HIP_TRY(ddisc.alloc(sizeof(double) * pairs));
  HIP_TRY(dsteps.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dterm.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dties.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dfin.alloc(sizeof(double) * pairs * S));
  for (int s0 = 0; s0 < n_starts; s0 += chunk)
  {
    const int nc = n_starts - s0 < chunk ? n_starts - s0 : chunk;
    HIP_TRY(hipMemcpy(dst.p, states + (size_t)s0 * S, sizeof(double) * (size_t)nc * S, hipMemcpyHostToDevice));
    EvaluateArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.n_starts = nc; A.max_steps = max_steps;
    A.states = dst.as<double>();
    A.sweep = ctx->sweep ? ctx->sweep_dev : nullptr;
    A.ret = dret.as<double>(); A.disc = ddisc.as<double>();
    A.steps = dsteps.as<int32_t>(); A.terminal = dterm.as<int32_t>(); A.ties = dties.as<int32_t>();
    A.final_state = dfin.as<double>();
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
    HIP_TRY(launch_evaluate(ctx->P, A, nullptr));
    if (ret) HIP_TRY(query_copy_out(ret, dret.p, sizeof(double), n_replicas, n_starts, s0, nc));
    if (disc) HIP_TRY(query_copy_out(disc, ddisc.p, sizeof(double), n_replicas, n_starts, s0, nc));
    if (steps) HIP_TRY(query_copy_out(steps, dsteps.p, sizeof(int32_t), n_replicas, n_starts, s0, nc));
    if (terminal) HIP_TRY(query_copy_out(terminal, dterm.p, sizeof(int32_t), n_replicas, n_starts, s0, nc));
    if (ties) HIP_TRY(query_copy_out(ties, dties.p, sizeof(int32_t), n_replicas, n_starts, s0, nc));
    if (final_state) HIP_TRY(query_copy_out(final_state, dfin.p, sizeof(double) * (size_t)S, n_replicas, n_starts, s0, nc));
    HIP_TRY(hipDeviceSynchronize());               // every output may be NULL: the next chunk's copy-in must not overtake this launch
  }
  return GRLX_OK;
}

// ---- ensemble evaluation: one episode per (group of consecutive replicas, start state) on the group's vote or mean Q ----------------------
int grlx_evaluate_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                           int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                           int64_t *agreement, double *final_state)
{
  const char *who = "grlx_evaluate_ensemble";
  int rc = evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps);
  if (rc != GRLX_OK) return rc;
  if (!q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "%s is not built for the actor-critic agent (a vote over continuous actions is mapping/policy/multi's); it serves agents with a policy/discrete/q", who);
  if (group_size < 1) return fail(GRLX_ERR_INVALID, "%s: group_size = %d is below 1", who, group_size);
  if (n_replicas % group_size != 0) return fail(GRLX_ERR_INVALID, "%s: group_size %d does not divide the %d replicas", who, group_size, n_replicas);
  if (rule != GRLX_ENSEMBLE_VOTE && rule != GRLX_ENSEMBLE_MEAN_Q)
    return fail(GRLX_ERR_INVALID, "%s: unknown rule %d (GRLX_ENSEMBLE_VOTE = 0, GRLX_ENSEMBLE_MEAN_Q = 1)", who, rule);
  if (max_steps == 0) max_steps = GRLX_MAX_EPISODE_STEPS;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  const int S = ctx->S, n_groups = n_replicas / group_size;
  const size_t per_pair = 2 * sizeof(double) + 3 * sizeof(int32_t) + 2 * sizeof(int64_t) + sizeof(double) * (size_t)S;
  int chunk = query_chunk(n_starts, sizeof(double) * (size_t)S + per_pair * (size_t)n_groups);
  if ((int64_t)chunk * n_groups > 0x7fffffff) chunk = 0x7fffffff / n_groups;      // one block per pair: the grid's bound
  const size_t pairs = (size_t)n_groups * (size_t)chunk;
  DevBuf dst, dret, ddisc, dsteps, dterm, dties, dmt, dag, dfin;
  HIP_TRY(dst.alloc(sizeof(double) * (size_t)chunk * S));
  HIP_TRY(dret.alloc(sizeof(double) * pairs));
  HIP_TRY(ddisc.alloc(sizeof(double) * pairs));
  HIP_TRY(dsteps.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dterm.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dties.alloc(sizeof(int32_t) * pairs));
  HIP_TRY(dmt.alloc(sizeof(int64_t) * pairs));
  HIP_TRY(dag.alloc(sizeof(int64_t) * pairs));
  HIP_TRY(dfin.alloc(sizeof(double) * pairs * S));
  for (int s0 = 0; s0 < n_starts; s0 += chunk)
  {
    const int nc = n_starts - s0 < chunk ? n_starts - s0 : chunk;
    HIP_TRY(hipMemcpy(dst.p, states + (size_t)s0 * S, sizeof(double) * (size_t)nc * S, hipMemcpyHostToDevice));
    EnsembleArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.group_size = group_size; A.rule = rule;
    A.n_starts = nc; A.max_steps = max_steps;
    A.states = dst.as<double>();
    A.sweep = ctx->sweep ? ctx->sweep_dev : nullptr;
    A.ret = dret.as<double>(); A.disc = ddisc.as<double>();
    A.steps = dsteps.as<int32_t>(); A.terminal = dterm.as<int32_t>(); A.ties = dties.as<int32_t>();
    A.member_ties = dmt.as<int64_t>(); A.agreement = dag.as<int64_t>();
    A.final_state = dfin.as<double>();
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
    HIP_TRY(launch_evaluate_ensemble(ctx->P, A, nullptr));
    if (ret) HIP_TRY(query_copy_out(ret, dret.p, sizeof(double), n_groups, n_starts, s0, nc));
    if (disc) HIP_TRY(query_copy_out(disc, ddisc.p, sizeof(double), n_groups, n_starts, s0, nc));
    if (steps) HIP_TRY(query_copy_out(steps, dsteps.p, sizeof(int32_t), n_groups, n_starts, s0, nc));
    if (terminal) HIP_TRY(query_copy_out(terminal, dterm.p, sizeof(int32_t), n_groups, n_starts, s0, nc));
    if (ties) HIP_TRY(query_copy_out(ties, dties.p, sizeof(int32_t), n_groups, n_starts, s0, nc));
    if (member_ties) HIP_TRY(query_copy_out(member_ties, dmt.p, sizeof(int64_t), n_groups, n_starts, s0, nc));
    if (agreement) HIP_TRY(query_copy_out(agreement, dag.p, sizeof(int64_t), n_groups, n_starts, s0, nc));
    if (final_state) HIP_TRY(query_copy_out(final_state, dfin.p, sizeof(double) * (size_t)S, n_groups, n_starts, s0, nc));
    HIP_TRY(hipDeviceSynchronize());               // every output may be NULL: the next chunk's copy-in must not overtake this launch
  }
  return GRLX_OK;
}

int grlx_math(int op, const double *x, const double *y, int n, double *out)
{
  if (!x || !out || n < 0 || op < 0 || op > 13 || (op == 3 && !y)) return fail(GRLX_ERR_INVALID, "bad argument");
  if (op >= 9 && op <= 12)      // the unchecked forms: nothing outside their domain reaches them (!(a < b) refuses a NaN too)
    for (int i = 0; i < n; ++i)
      if (!(std::fabs(x[i]) < 0x1p20)) return fail(GRLX_ERR_INVALID, "grlx_math ops 9 to 12 are the unchecked sin/cos forms: every argument must satisfy |x| < 2^20");
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  DevBuf dx, dy, dout;
  HIP_TRY(dx.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dy.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(hipMemcpy(dx.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  if (y) HIP_TRY(hipMemcpy(dy.p, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_math(op, dx.as<double>(), dy.as<double>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_rand48_at(int64_t seed, const uint64_t *skip, int n, double *out)
{
  if (!skip || !out || n < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  DevBuf ds, dout;
  HIP_TRY(ds.alloc(sizeof(uint64_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(hipMemcpy(ds.p, skip, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_rand48_at(h_seed((long)seed), ds.as<uint64_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// ------------------------------------------------------------------------------------------------ exact resume ---
// A snapshot (layout: grlx_snapshot_format.h) is assembled in the caller's buffer section by section; the tables go through the
// compacting kernels of grlx_snapshot.hip.  A load validates and allocates everything first, unpacks into NEW tables, and only then
// touches the context.
} // extern "C"
namespace {

static_assert(sizeof(ReplicaState) == snap::kStateBytes, "grlx_snapshot_format.h: kStateBytes");
static_assert(offsetof(ReplicaState, lazy_base) == snap::kStatePointerOffsets[0] && offsetof(ReplicaState, lazy_base) + 8 == snap::kStatePointerOffsets[1] &&
              offsetof(ReplicaState, target_base) == snap::kStatePointerOffsets[2], "grlx_snapshot_format.h: kStatePointerOffsets");
static_assert(offsetof(ReplicaState, n_slots) == snap::kStateSlotsOffset && offsetof(ReplicaState, rows) == snap::kStateRowsOffset, "grlx_snapshot_format.h: state offsets");
static_assert(snap::kTraceWordsPerReplica == 16 * kMaxTrace * 2, "grlx_snapshot_format.h: kTraceWordsPerReplica");

// the fields of grlx_config a snapshot and the context that loads it must agree in: all but the layout and sizing fields
// (replicas_per_wave, wave_limit, force_generic, table_log2_capacity, table_log2_max) and the tap fields (taps are refused)
struct CfgField { const char *name; size_t off; int kind; };       // kind 0: int32, 1: double
#define CF_I(f) {#f, offsetof(grlx_config, f), 0}
#define CF_D(f) {#f, offsetof(grlx_config, f), 1}
const CfgField kSnapshotCfgFields[] = {
  CF_I(n_replicas), CF_I(test_interval), CF_I(env), CF_D(control_step), CF_I(integration_steps), CF_I(discrete_time), CF_D(timeout), CF_D(randomization),
  CF_D(action_min), CF_D(action_max), CF_I(action_steps), CF_I(agent),
  CF_I(projector.tilings), CF_I(projector.memory), CF_I(projector.dims), CF_I(projector.safe),
  CF_D(representation.init_min), CF_D(representation.init_max), CF_D(representation.output_min), CF_D(representation.output_max), CF_I(representation.limit),
  CF_D(epsilon), CF_D(decay_rate), CF_D(decay_min), CF_D(alpha), CF_D(gamma), CF_D(lambda), CF_I(trace),
  CF_I(actor_projector.tilings), CF_I(actor_projector.memory), CF_I(actor_projector.dims), CF_I(actor_projector.safe),
  CF_D(actor_representation.init_min), CF_D(actor_representation.init_max), CF_D(actor_representation.output_min), CF_D(actor_representation.output_max),
  CF_I(actor_representation.limit),
  CF_D(actor_alpha), CF_D(sigma), CF_D(theta), CF_D(ac_decay_rate), CF_D(ac_decay_min), CF_D(ac_step_limit), CF_I(ac_update_method),
  CF_I(max_rows), CF_I(end_stop_penalty), CF_I(action_penalty), CF_D(slope_angle), CF_D(initial_state_variation), CF_D(negative_reward),
  CF_D(kappa), CF_D(beta), CF_I(target_interval), CF_D(target_tau), CF_I(test_trials),
};
#undef CF_I
#undef CF_D

int snapshot_config_differs(const grlx_config &have, const grlx_config &snapshot)
{
  for (const CfgField &f : kSnapshotCfgFields)
  {
    const char *a = (const char *)&have + f.off, *b = (const char *)&snapshot + f.off;
    if (f.kind == 0)
    {
      int32_t x, y;
      memcpy(&x, a, 4); memcpy(&y, b, 4);
      if (x != y) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the context's %s = %d, the snapshot's is %d", f.name, x, y);
    }
    else
    {
      double x, y;
      memcpy(&x, a, 8); memcpy(&y, b, 8);
      if (memcmp(a, b, 8) != 0) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the context's %s = %.17g, the snapshot's is %.17g", f.name, x, y);
    }
  }
  const struct { const char *name; const grlx_tile_spec *a, *b; } tiles[2] = {{"projector", &have.projector, &snapshot.projector},
                                                                                {"actor_projector", &have.actor_projector, &snapshot.actor_projector}};
  for (const auto &t : tiles)
    for (int i = 0; i < t.a->dims && i < GRLX_MAX_DIMS; ++i)
    {
      if (memcmp(&t.a->resolution[i], &t.b->resolution[i], 8) != 0)
        return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the context's %s.resolution[%d] = %.17g, the snapshot's is %.17g", t.name, i, t.a->resolution[i], t.b->resolution[i]);
      if (memcmp(&t.a->wrapping[i], &t.b->wrapping[i], 8) != 0)
        return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the context's %s.wrapping[%d] = %.17g, the snapshot's is %.17g", t.name, i, t.a->wrapping[i], t.b->wrapping[i]);
    }
  return GRLX_OK;
}

// what this pull of the feature does not carry, for the context a snapshot is taken of or loaded into
int snapshot_not_built(const grlx_ctx *ctx, const char *who)
{
  bool target_image = false;
  for (const double *t : ctx->target_images) target_image = target_image || t != nullptr;
  if (!ctx->images.empty() || target_image)
    return fail(GRLX_ERR_INVALID, "%s: not built for a context that holds a loaded policy (grlx_load_weights): a snapshot carries no dense parameter vectors", who);
  if (ctx->agent_rep) return fail(GRLX_ERR_INVALID, "%s: not built for a context on which a per-step entry point has run (agent state in mid-episode)", who);
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "%s: not built for GRLX_ENV_EXTERNAL", who);
  if (ctx->P.tap_capacity > 0 || ctx->P.diag_out || ctx->diag) return fail(GRLX_ERR_INVALID, "%s: not built for a context with taps or diagnostics (grlx_set_diag)", who);
  return GRLX_OK;
}

// launch one of the two snapshot kernels on the null stream between two events: *ms = its device time (diagnostic, grlx_snapshot_timing)
int timed_snapshot_launch(hipError_t (*launch)(const SnapshotArgs &, hipStream_t), const SnapshotArgs &a, double *ms)
{
  hipEvent_t t0 = nullptr, t1 = nullptr;
  const bool timed = hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess;
  if (!timed) (void)hipGetLastError();
  if (timed) (void)hipEventRecord(t0, nullptr);
  const hipError_t e = launch(a, nullptr);
  if (timed) (void)hipEventRecord(t1, nullptr);
  float f = -1.f;
  if (e == hipSuccess && timed && hipEventSynchronize(t1) == hipSuccess) (void)hipEventElapsedTime(&f, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  *ms = f;
  if (e != hipSuccess) return fail(GRLX_ERR_HIP, "snapshot kernel launch failed: %s", hipGetErrorString(e));
  return GRLX_OK;
}

// the header of a snapshot of the context as it stands (drained), its replica states with the device pointers zeroed, and the
// record count / first record of every stream (table * n_replicas + replica)
int snapshot_plan(grlx_ctx *ctx, snap::Header *h, std::vector<ReplicaState> *hs, std::vector<uint32_t> *counts, std::vector<uint64_t> *offsets)
{
  const size_t N = (size_t)ctx->P.n_replicas, T = (size_t)ctx->n_tables;
  hs->resize(N);
  HIP_TRY(hipMemcpy(hs->data(), ctx->states, sizeof(ReplicaState) * N, hipMemcpyDeviceToHost));
  memset(h, 0, sizeof(*h));
  h->cfg = ctx->cfg;
  h->n_replicas = (uint32_t)N;
  h->n_tables = (uint32_t)T;
  h->logC = ctx->P.logC;
  h->trials_run = ctx->trials_run;
  h->flags = (ctx->sweep ? snap::kFlagSweep : 0u) | (ctx->trace_state ? snap::kFlagTrace : 0u) | (ctx->tvals ? snap::kFlagTarget : 0u) |
             (ctx->P.twin_tables ? snap::kFlagTwin : 0u);
  counts->assign(T * N, 0u);
  offsets->assign(T * N, 0ull);
  for (ReplicaState &s : *hs)
  {
    s.lazy_base[0] = s.lazy_base[1] = nullptr;
    s.target_base = nullptr;
    if (s.rows > h->rows) h->rows = s.rows;
  }
  for (size_t t = 0; t < T; ++t)
    for (size_t r = 0; r < N; ++r)
    {
      (*counts)[t * N + r] = (*hs)[r].n_slots[t];
      (*offsets)[t * N + r] = h->n_records;
      h->n_records += (*hs)[r].n_slots[t];
    }
  if (h->rows > (uint32_t)ctx->cfg.max_rows) h->rows = (uint32_t)ctx->cfg.max_rows;
  snap::fill_sizes(h);
  return GRLX_OK;
}

} // namespace
extern "C" {

int grlx_snapshot_info(const void *buf, uint64_t bytes, grlx_snapshot_info_t *out)
{
  if (!buf || !out) return fail(GRLX_ERR_INVALID, "grlx_snapshot_info: null argument");
  snap::Header h;
  char msg[256];
  if (snap::read_header(buf, bytes, &h, msg, sizeof(msg)) != 0) return fail(GRLX_ERR_INVALID, "%s", msg);
  memset(out, 0, sizeof(*out));
  out->format_version = h.version;
  out->n_replicas = h.n_replicas;
  out->n_tables = h.n_tables;
  out->table_log2 = h.logC;
  out->is_sweep = (h.flags & snap::kFlagSweep) ? 1u : 0u;
  out->has_trace = (h.flags & snap::kFlagTrace) ? 1u : 0u;
  out->has_target = (h.flags & snap::kFlagTarget) ? 1u : 0u;
  out->twin_tables = (h.flags & snap::kFlagTwin) ? 1u : 0u;
  out->rows = h.rows;
  out->record_bytes = h.record_bytes;
  out->trials_run = h.trials_run;
  out->total_bytes = h.total_bytes;
  out->header_bytes = h.header_bytes;
  out->n_records = h.n_records;
  out->checksum = h.checksum;
  for (int s = 0; s < snap::SEC_COUNT; ++s) out->section_bytes[s] = h.section_bytes[s];
  out->config = h.cfg;
  return GRLX_OK;
}

int grlx_snapshot_size(grlx_ctx *ctx, uint64_t *bytes)
{
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (!ctx || !bytes) return fail(GRLX_ERR_INVALID, "grlx_snapshot_size: null argument");
  int rc = snapshot_not_built(ctx, "grlx_snapshot_size");
  if (rc != GRLX_OK) return rc;
  DRAIN(ctx);
  snap::Header h;
  std::vector<ReplicaState> hs;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> offsets;
  if ((rc = snapshot_plan(ctx, &h, &hs, &counts, &offsets)) != GRLX_OK) return rc;
  *bytes = h.total_bytes;
  return GRLX_OK;
}

int grlx_snapshot_save(grlx_ctx *ctx, void *buf, uint64_t cap, uint64_t *written)
{
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (!ctx || !buf || !written) return fail(GRLX_ERR_INVALID, "grlx_snapshot_save: null argument");
  *written = 0;
  int rc = snapshot_not_built(ctx, "grlx_snapshot_save");
  if (rc != GRLX_OK) return rc;
  DRAIN(ctx);
  snap::Header h;
  std::vector<ReplicaState> hs;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> offsets;
  if ((rc = snapshot_plan(ctx, &h, &hs, &counts, &offsets)) != GRLX_OK) return rc;
  if (cap < h.total_bytes) return fail(GRLX_ERR_INVALID, "grlx_snapshot_save: the buffer holds %llu bytes, the snapshot needs %llu", (unsigned long long)cap, (unsigned long long)h.total_bytes);
  const size_t N = (size_t)ctx->P.n_replicas;
  uint8_t *out = (uint8_t *)buf + h.header_bytes;
  memcpy(out, hs.data(), sizeof(ReplicaState) * N);
  out += h.section_bytes[snap::SEC_STATES];
  { // rows [row][replica]: the first h.rows rows of each of the four arrays
    const size_t part = 8 * (size_t)h.rows * N;
    const void *src[4] = {ctx->row_reward, ctx->row_time, ctx->row_steps, ctx->row_trial};
    for (int k = 0; k < 4 && part != 0; ++k) HIP_TRY(hipMemcpy(out + (size_t)k * part, src[k], part, hipMemcpyDeviceToHost));
    // rows at or above a replica's own count are dead (ragged under a steps budget, stale after grlx_reset_run): written as zero, so that
    // equal states give equal bytes
    for (int k = 0; k < 4; ++k)
      for (size_t r = 0; r < N; ++r)
        for (size_t row = hs[r].rows; row < h.rows; ++row) memset(out + (size_t)k * part + 8 * (row * N + r), 0, 8);
    out += h.section_bytes[snap::SEC_ROWS];
  }
  if (h.flags & snap::kFlagTrace)
  {
    HIP_TRY(hipMemcpy(out, ctx->trace_state, h.section_bytes[snap::SEC_TRACE], hipMemcpyDeviceToHost));
    out += h.section_bytes[snap::SEC_TRACE];
  }
  if (h.flags & snap::kFlagSweep)
  {
    for (int k = 0; k < 4; ++k)
      if ((rc = grlx_get_replica_params(ctx, k, (double *)out + (size_t)k * N)) != GRLX_OK) return rc;
    out += h.section_bytes[snap::SEC_SWEEP];
  }
  if (h.n_records != 0)
  {
    DevBuf rec, off, cnt, err;
    if (rec.alloc(h.section_bytes[snap::SEC_RECORDS]) != hipSuccess || off.alloc(offsets.size() * 8) != hipSuccess || cnt.alloc(counts.size() * 4) != hipSuccess ||
        err.alloc(4) != hipSuccess)
    {
      (void)hipGetLastError();
      return fail(GRLX_ERR_OOM, "grlx_snapshot_save: no device memory for the record stream (%.1f MiB)", (double)h.section_bytes[snap::SEC_RECORDS] / 1048576.);
    }
    HIP_TRY(hipMemcpy(off.p, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cnt.p, counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0, 4));
    SnapshotArgs a;
    a.tables = ctx->tables; a.tvals = ctx->tvals; a.logC = ctx->P.logC; a.n_replicas = ctx->P.n_replicas; a.n_tables = ctx->n_tables;
    a.offsets = off.as<uint64_t>(); a.counts = cnt.as<uint32_t>(); a.records = rec.as<uint8_t>(); a.record_bytes = h.record_bytes; a.err = err.as<uint32_t>();
    if ((rc = timed_snapshot_launch(launch_snapshot_pack, a, &ctx->snap_pack_ms)) != GRLX_OK) return rc;
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, err.p, 4, hipMemcpyDeviceToHost));
    if (e != 0) return fail(GRLX_ERR_INVALID, "grlx_snapshot_save: table occupancy and slot count disagree");
    HIP_TRY(hipMemcpy(out, rec.p, h.section_bytes[snap::SEC_RECORDS], hipMemcpyDeviceToHost));
  }
  h.checksum = snap::fnv1a((const uint8_t *)buf + h.header_bytes, h.total_bytes - h.header_bytes);
  snap::write_header(h, (uint8_t *)buf);
  *written = h.total_bytes;
  return GRLX_OK;
}

int grlx_snapshot_load(grlx_ctx *ctx, const void *buf, uint64_t bytes)
{
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (!ctx || !buf) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: null argument");
  if (ctx->launched) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load is allowed only on a context that has launched nothing yet");
  int rc = snapshot_not_built(ctx, "grlx_snapshot_load");
  if (rc != GRLX_OK) return rc;
  // --- validate: the header, the size, the checksum, the configuration, the counts
  snap::Header h;
  char msg[256];
  if (snap::read_header(buf, bytes, &h, msg, sizeof(msg)) != 0) return fail(GRLX_ERR_INVALID, "%s", msg);
  if (bytes != h.total_bytes) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: %llu bytes given, the snapshot's header says %llu", (unsigned long long)bytes, (unsigned long long)h.total_bytes);
  if (snap::fnv1a((const uint8_t *)buf + h.header_bytes, h.total_bytes - h.header_bytes) != h.checksum)
    return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: checksum mismatch (the snapshot is damaged)");
  if ((rc = snapshot_config_differs(ctx->cfg, h.cfg)) != GRLX_OK) return rc;
  const size_t N = (size_t)ctx->P.n_replicas, T = (size_t)ctx->n_tables;
  const uint32_t want_flags = (ctx->trace_state ? snap::kFlagTrace : 0u) | (ctx->P.target_interval > 0 ? snap::kFlagTarget : 0u) | (ctx->P.twin_tables ? snap::kFlagTwin : 0u);
  if (h.n_tables != T || (h.flags & ~snap::kFlagSweep) != want_flags)
    return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the snapshot's tables (%u, flags %u) are not those of its configuration (%zu, flags %u)", h.n_tables, h.flags, T, want_flags);
  if (h.logC > ctx->logC_max)
    return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the snapshot's tables hold 2^%u entries, beyond the context's table_log2_max = %u", h.logC, ctx->logC_max);
  if (ctx->sweep && !(h.flags & snap::kFlagSweep))
    return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the context has per-replica parameters (grlx_set_replica_params), the snapshot has none");
  const uint8_t *in = (const uint8_t *)buf + h.header_bytes;
  std::vector<ReplicaState> hs(N);
  memcpy(hs.data(), in, sizeof(ReplicaState) * N);
  in += h.section_bytes[snap::SEC_STATES];
  const uint8_t *rows_in = in;
  in += h.section_bytes[snap::SEC_ROWS];
  const uint8_t *trace_in = in;
  in += h.section_bytes[snap::SEC_TRACE];
  const double *sweep_in = (const double *)in;
  in += h.section_bytes[snap::SEC_SWEEP];
  const uint8_t *records_in = in;
  std::vector<uint32_t> counts(T * N, 0u);
  std::vector<uint64_t> offsets(T * N, 0ull);
  uint64_t n_records = 0;
  for (size_t t = 0; t < T; ++t)
    for (size_t r = 0; r < N; ++r)
    {
      if (hs[r].n_slots[t] > (1u << h.logC)) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: replica %zu, table %zu: %u records exceed the capacity 2^%u", r, t, hs[r].n_slots[t], h.logC);
      counts[t * N + r] = hs[r].n_slots[t];
      offsets[t * N + r] = n_records;
      n_records += hs[r].n_slots[t];
    }
  if (n_records != h.n_records) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: the replicas' slot counts add up to %llu records, the header says %llu", (unsigned long long)n_records, (unsigned long long)h.n_records);
  for (ReplicaState &s : hs)
  {
    if (s.rows > h.rows) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: a replica has %u rows, the header says at most %u", s.rows, h.rows);
    if (s.tr_len < 0 || s.tr_len > kMaxTrace) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: a replica's trace length %d", s.tr_len);
    s.lazy_base[0] = s.lazy_base[1] = nullptr;         // whatever the file says
    s.target_base = nullptr;
  }
  std::vector<SweepParams> sweep_rec;
  if (h.flags & snap::kFlagSweep)
  { // as grlx_set_replica_params validates them, all four at once
    if ((rc = sweep_admits(ctx->cfg, ctx->P)) != GRLX_OK) return rc;
    sweep_rec.resize(N);
    for (size_t r = 0; r < N; ++r)
      if ((rc = sweep_record(ctx->cfg, r, sweep_in[GRLX_PARAM_ALPHA * N + r], sweep_in[GRLX_PARAM_GAMMA * N + r], sweep_in[GRLX_PARAM_LAMBDA * N + r],
                             sweep_in[GRLX_PARAM_EPSILON * N + r], GRLX_PARAM_GAMMA, &sweep_rec[r])) != GRLX_OK)
        return rc;
  }
  // --- allocate: the tables at the snapshot's capacity and everything the unpacking needs, before anything of the context is touched
  HIP_TRY(hipDeviceSynchronize());
  const size_t table_bytes = (N * T * sizeof(Entry)) << h.logC, tval_bytes = (N * sizeof(double)) << h.logC;
  DevBuf nt, ntv, rec, off, cnt, err, nsw;
  if (nt.alloc(table_bytes) != hipSuccess || (ctx->tvals && ntv.alloc(tval_bytes) != hipSuccess) || rec.alloc(h.section_bytes[snap::SEC_RECORDS]) != hipSuccess ||
      off.alloc(offsets.size() * 8) != hipSuccess || cnt.alloc(counts.size() * 4) != hipSuccess || err.alloc(4) != hipSuccess ||
      (!sweep_rec.empty() && !ctx->sweep_dev && nsw.alloc(sizeof(SweepParams) * N) != hipSuccess))
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "grlx_snapshot_load: no device memory for tables of 2^%u entries per replica (%.1f GiB) and the record stream", h.logC, (double)table_bytes / 1073741824.);
  }
  HIP_TRY(hipMemset(nt.p, 0, table_bytes));
  if (ntv.p) HIP_TRY(hipMemset(ntv.p, 0xFF, tval_bytes));
  if (h.n_records != 0)
  {
    HIP_TRY(hipMemcpy(rec.p, records_in, h.section_bytes[snap::SEC_RECORDS], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(off.p, offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cnt.p, counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.p, 0, 4));
    SnapshotArgs a;
    a.tables = (Entry *)nt.p; a.tvals = (double *)ntv.p; a.logC = h.logC; a.n_replicas = (int32_t)N; a.n_tables = (int32_t)T;
    a.offsets = off.as<uint64_t>(); a.counts = cnt.as<uint32_t>(); a.records = rec.as<uint8_t>(); a.record_bytes = h.record_bytes; a.err = err.as<uint32_t>();
    if ((rc = timed_snapshot_launch(launch_snapshot_unpack, a, &ctx->snap_unpack_ms)) != GRLX_OK) return rc;
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, err.p, 4, hipMemcpyDeviceToHost));
    if (e != 0) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: a table record has an empty key, a position beyond the capacity, or is out of order");
  }
  // --- commit
  HIP_TRY(hipMemcpy(ctx->states, hs.data(), sizeof(ReplicaState) * N, hipMemcpyHostToDevice));
  {
    const size_t part = 8 * (size_t)h.rows * N;
    void *dst[4] = {ctx->row_reward, ctx->row_time, ctx->row_steps, ctx->row_trial};
    for (int k = 0; k < 4 && part != 0; ++k) HIP_TRY(hipMemcpy(dst[k], rows_in + (size_t)k * part, part, hipMemcpyHostToDevice));
  }
  if (ctx->trace_state) HIP_TRY(hipMemcpy(ctx->trace_state, trace_in, h.section_bytes[snap::SEC_TRACE], hipMemcpyHostToDevice));
  if (!sweep_rec.empty())
  {
    if (!ctx->sweep_dev) { ctx->sweep_dev = (SweepParams *)nsw.p; nsw.p = nullptr; }
    HIP_TRY(hipMemcpy(ctx->sweep_dev, sweep_rec.data(), sizeof(SweepParams) * N, hipMemcpyHostToDevice));
    for (int k = 0; k < 4; ++k) ctx->sweep_host[k].assign(sweep_in + (size_t)k * N, sweep_in + (size_t)(k + 1) * N);
    ctx->sweep = true;
    if (ctx->P.replicas_per_wave > 8) ctx->P.replicas_per_wave = 8;       // as grlx_set_replica_params
  }
  (void)hipFree(ctx->tables);
  if (ctx->tvals) (void)hipFree(ctx->tvals);
  ctx->tables = (Entry *)nt.p;
  ctx->tvals = (double *)ntv.p;
  nt.p = nullptr;
  ntv.p = nullptr;
  ctx->P.tables = ctx->tables;
  ctx->P.tvals = ctx->tvals;
  ctx->P.logC = h.logC;
  HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load, nullptr));      // what the run before the snapshot left there
  HIP_TRY(hipDeviceSynchronize());
  ctx->trials_run = h.trials_run;
  ctx->launched = true;
  return GRLX_OK;
}

// diagnostics (include/grlx_diag.h)
int grlx_snapshot_timing(grlx_ctx *ctx, double *pack_ms, double *unpack_ms)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  if (pack_ms) *pack_ms = ctx->snap_pack_ms;
  if (unpack_ms) *unpack_ms = ctx->snap_unpack_ms;
  return GRLX_OK;
}

int grlx_snapshot_naive_copy(grlx_ctx *ctx, uint64_t *bytes, double *out_ms, double *back_ms)
{
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (!ctx || !bytes || !out_ms || !back_ms) return fail(GRLX_ERR_INVALID, "grlx_snapshot_naive_copy: null argument");
  DRAIN(ctx);
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)ctx->P.n_replicas, rows = 8 * (size_t)ctx->cfg.max_rows * N;
  struct { void *dev; size_t n; } arr[8] = {
    {ctx->tables, (N * (size_t)ctx->n_tables * sizeof(Entry)) << ctx->P.logC}, {ctx->tvals, ctx->tvals ? (N * sizeof(double)) << ctx->P.logC : 0},
    {ctx->states, sizeof(ReplicaState) * N}, {ctx->row_reward, rows}, {ctx->row_time, rows}, {ctx->row_steps, rows}, {ctx->row_trial, rows},
    {ctx->trace_state, ctx->trace_state ? N * 16 * kMaxTrace * 2 * sizeof(uint32_t) : 0}};
  size_t total = 0;
  for (const auto &a : arr) total += a.n;
  char *host = (char *)malloc(total);
  if (!host) return fail(GRLX_ERR_OOM, "grlx_snapshot_naive_copy: no host memory for %.1f GiB", (double)total / 1073741824.);
  for (int dir = 0; dir < 2; ++dir)
  {
    const auto t0 = std::chrono::steady_clock::now();
    size_t at = 0;
    for (const auto &a : arr)
    {
      if (a.n == 0) continue;
      const hipError_t e = dir == 0 ? hipMemcpy(host + at, a.dev, a.n, hipMemcpyDeviceToHost) : hipMemcpy(a.dev, host + at, a.n, hipMemcpyHostToDevice);
      if (e != hipSuccess) { free(host); return fail(GRLX_ERR_HIP, "grlx_snapshot_naive_copy: hipMemcpy failed: %s", hipGetErrorString(e)); }
      at += a.n;
    }
    (dir == 0 ? *out_ms : *back_ms) = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  free(host);
  *bytes = total;
  return GRLX_OK;
}

} // extern "C"
