// grlx_api_config.cpp -- the C ABI declared in include/grlx.h: configuration and admission -- the parameter block from a grlx_config, the two default configurations, what grlx_create refuses before it looks for a device, and the launch plan of a configuration without a device.
#include "grlx_host.h"

namespace grlx {

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

static int make_linear_params(const grlx_linear_spec &ls, uint64_t draws_before, LinearParams *lp)
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

// Everything grlx_create refuses before it looks for a device.  P: the parameter block, without device pointers, sizes and layout.
int admit(const grlx_config *cfg, DevParams *P)
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

} // namespace grlx

extern "C" {

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
    sweep_limits_layout(P);
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

} // extern "C"
