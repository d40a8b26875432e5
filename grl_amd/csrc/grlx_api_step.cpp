// grlx_api_step.cpp -- the C ABI declared in include/grlx.h: the per-step entry points of a context (environment and agent, one call per step) and the stateless operators.
#include "grlx_host.h"

// ---------------------------------------------------------------------------------------------------------------
// The per-step plug-in interfaces on a context's replicas (grlx_step.h).  Host pointers; each call copies its arguments in,
// launches one kernel over all replicas and copies the results out.
static int step_buffers(grlx_ctx *ctx)
{
  if (ctx->stage_f64) return GRLX_OK;
  const size_t N = (size_t)ctx->P.n_replicas;
  Dev<double> f64;
  Dev<int32_t> i32;
  if (f64.alloc(sizeof(double) * N * (GRLX_MAX_DIMS + 2)) != hipSuccess || i32.alloc(sizeof(int32_t) * N * 2) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "no device memory for the staging buffers of the per-step entry points");
  }
  ctx->stage_f64 = std::move(f64);
  ctx->stage_i32 = std::move(i32);
  return GRLX_OK;
}

static const int32_t *stage_active(grlx_ctx *ctx, const int32_t *active, hipError_t *err)
{
  *err = hipSuccess;
  if (!active) return nullptr;
  *err = hipMemcpy(ctx->stage_i32.get(), active, sizeof(int32_t) * (size_t)ctx->P.n_replicas, hipMemcpyHostToDevice);
  return ctx->stage_i32.get();
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
  Dev<uint32_t> trace, lane;               // the whole group or nothing: the context is touched once all of it exists
  Dev<AgentRep> rep;
  if (!ctx->trace_state)
  { // the predictor's trace between calls, in the layout the actor-critic kernels persist theirs in: empty
    if (trace.alloc(trace_words(N) * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return fail(GRLX_ERR_OOM, "no device memory for the agents' traces"); }
    HIP_TRY(upload_empty_trace(trace.get(), N));
  }
  if (lane.alloc(sizeof(uint32_t) * N * 16 * 2) != hipSuccess) { (void)hipGetLastError(); return fail(GRLX_ERR_OOM, "no device memory for the agents' state"); }
  HIP_TRY(hipMemset(lane.get(), 0, sizeof(uint32_t) * N * 16 * 2));
  if (rep.alloc(sizeof(AgentRep) * N) != hipSuccess) { (void)hipGetLastError(); return fail(GRLX_ERR_OOM, "no device memory for the agents' state"); }
  HIP_TRY(hipMemset(rep.get(), 0, sizeof(AgentRep) * N));
  if (trace) ctx->trace_state = std::move(trace);
  ctx->agent_lane = std::move(lane);
  ctx->agent_rep = std::move(rep);
  bind_params(ctx, ctx->P.logC, &ctx->P);
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
    HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load.get(), nullptr));
    HIP_TRY(hipMemcpy(&used, ctx->max_load.get(), sizeof(used), hipMemcpyDeviceToHost));
    if ((rc = grow_if_loaded(ctx, used)) != GRLX_OK) return rc;
  }
  const size_t N = (size_t)ctx->P.n_replicas;
  const size_t D = (size_t)(ctx->cfg.agent == GRLX_AGENT_AC ? ctx->P.tile.D : ctx->P.tile.D - 1);
  double *d_obs = ctx->stage_f64.get(), *d_reward = d_obs + N * GRLX_MAX_DIMS, *d_action = d_reward + N;
  int32_t *d_term = ctx->stage_i32.get() + N;
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

extern "C" {

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
  if (active) HIP_TRY(hipMemcpy(ctx->stage_f64.get(), obs, sizeof(double) * N * D, hipMemcpyHostToDevice));     // inactive rows keep the caller's values
  HIP_TRY(launch_env_start(ctx->P, test ? 1 : 0, act, ctx->stage_f64.get(), nullptr));
  HIP_TRY(hipMemcpy(obs, ctx->stage_f64.get(), sizeof(double) * N * D, hipMemcpyDeviceToHost));
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
  double *d_obs = ctx->stage_f64.get(), *d_reward = d_obs + N * GRLX_MAX_DIMS, *d_action = d_reward + N;
  int32_t *d_term = ctx->stage_i32.get() + N;
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
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch.get(), nullptr));
  HIP_TRY(hipMemcpy(h, ctx->scratch.get(), sizeof(h), hipMemcpyDeviceToHost));
  return status_to_error(h[2] & ST_DOMAIN);
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
  int o = 0, i = 0;                                     // what the queries admit (quant_admit_rows, grlx_host_rules.h); nothing is written
  if (int why = quant_admit_rows(in, n, tp.D, tp.scaling, &o, &i))
  {
    const double x = in[(size_t)o * (size_t)tp.D + (size_t)i];
    if (why == 1) return fail(GRLX_ERR_INVALID, "grlx_project: input row %d, dimension %d is not finite (%g)", o, i, x);
    return fail(GRLX_ERR_INVALID, "grlx_project: input row %d, dimension %d (%g) is out of range: |x * scaling| reaches 2^30", o, i, x);
  }
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  DevBuf din, dout;
  HIP_TRY(din.upload(in, sizeof(double) * (size_t)n * (size_t)tp.D));
  HIP_TRY(dout.alloc(sizeof(uint32_t) * (size_t)n * (size_t)tp.T));
  HIP_TRY(launch_project(tp, din.as<double>(), n, dout.as<uint32_t>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(uint32_t) * (size_t)n * (size_t)tp.T, hipMemcpyDeviceToHost));
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
  HIP_TRY(ds.upload(state, sizeof(double) * (size_t)n * S));
  HIP_TRY(da.upload(action, sizeof(double) * (size_t)n));
  HIP_TRY(dobs.alloc(sizeof(double) * (size_t)n * D));
  HIP_TRY(dr.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dt.alloc(sizeof(int32_t) * (size_t)n));
  HIP_TRY(derr.alloc(sizeof(uint32_t)));
  HIP_TRY(hipMemset(derr.get(), 0, sizeof(uint32_t)));
  HIP_TRY(launch_env_step(P, ds.as<double>(), da.as<double>(), n, dobs.as<double>(), dr.as<double>(), dt.as<int32_t>(), derr.as<uint32_t>(), nullptr));
  HIP_TRY(hipMemcpy(state, ds.get(), sizeof(double) * (size_t)n * S, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(obs, dobs.get(), sizeof(double) * (size_t)n * D, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(reward, dr.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(terminal, dt.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  uint32_t err = 0;
  HIP_TRY(hipMemcpy(&err, derr.get(), sizeof(err), hipMemcpyDeviceToHost));
  if (err & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "environment state left the supported domain (NaN)");
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
  HIP_TRY(dx.upload(x, sizeof(double) * (size_t)n));
  HIP_TRY(dy.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  if (y) HIP_TRY(hipMemcpy(dy.get(), y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_math(op, dx.as<double>(), dy.as<double>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_rand48_at(int64_t seed, const uint64_t *skip, int n, double *out)
{
  if (!skip || !out || n < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!have_device()) return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback");
  if (n == 0) return GRLX_OK;
  DevBuf ds, dout;
  HIP_TRY(ds.upload(skip, sizeof(uint64_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(launch_rand48_at(h_seed((long)seed), ds.as<uint64_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

} // extern "C"
