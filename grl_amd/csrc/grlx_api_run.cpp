// grlx_api_run.cpp -- the C ABI declared in include/grlx.h: the run loop and its read-backs -- grlx_run / grlx_sync, step counts, rows, curve statistics, the environment server's diagnostics and the per-replica parameters of a sweep.
#include "grlx_host.h"

// Mailboxes, stream and events of the environment server, created at the first launch that wants them.  The server is an optimisation: when
// its 1 KB per replica (or a stream, or an event) cannot be had, the context goes on without it.
static bool env_server_ready(grlx_ctx *ctx, size_t mail_bytes)
{
  if (ctx->env_mail) return true;
  Dev<EnvMail> mail;
  DevStream stream;
  DevEvent go, done;
  if (mail_bytes == 0 || mail.alloc((size_t)ctx->P.n_replicas * mail_bytes) != hipSuccess || stream.create(hipStreamNonBlocking) != hipSuccess ||
      go.create(hipEventDisableTiming) != hipSuccess || done.create(hipEventDisableTiming) != hipSuccess)
  {
    (void)hipGetLastError();
    ctx->env_server = 0;
    return false;
  }
  ctx->env_mail_bytes = mail_bytes;
  ctx->env_mail = std::move(mail);
  ctx->srv_stream = std::move(stream);
  ctx->srv_go = std::move(go);
  ctx->srv_done = std::move(done);
  return true;
}

static int run_trials(grlx_ctx *ctx, int n_trials, uint64_t steps_budget, void *stream)
{
  if (!ctx || n_trials < 0) return fail(GRLX_ERR_INVALID, "bad argument");
  STREAM_REFUSES(ctx, "grlx_run / grlx_run_steps");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "this context has no environment (GRLX_ENV_EXTERNAL): drive it through grlx_agent_start / _step / _end");
  if (n_trials == 0) return GRLX_OK;
  if (steps_budget != 0 && (ctx->P.tap_capacity > 0 || ctx->P.diag_out))
    return fail(GRLX_ERR_INVALID, "a steps budget is not available with taps or diagnostics");
  if (!ctx->run_pending && ctx->P.logC < ctx->logC_max)
  { // nothing in flight: how full did the last run leave the fullest table?
    uint32_t used = 0;
    HIP_TRY(hipMemcpy(&used, ctx->max_load.get(), sizeof(used), hipMemcpyDeviceToHost));
    const int rc = grow_if_loaded(ctx, used);
    if (rc != GRLX_OK) return rc;
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
      HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load.get(), (hipStream_t)stream));
      HIP_TRY(hipMemcpyAsync(&used, ctx->max_load.get(), sizeof(used), hipMemcpyDeviceToHost, (hipStream_t)stream));
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      const int rc = grow_if_loaded(ctx, used);
      if (rc != GRLX_OK) return rc;
      bind_params(ctx, ctx->P.logC, &Pb);          // the launches below work on the tables the context has now
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
      Pb.env_mail = ctx->env_mail.get();
      Pb.env_tune = 3u;        // the rollout wave is the critical path: it issues first, the server fills its gaps (+0.7 %)
      if (const char *tune = getenv("GRLX_ENV_SERVER_TUNE")) Pb.env_tune = (uint32_t)strtoul(tune, nullptr, 0);
      HIP_TRY(hipMemsetAsync(ctx->env_mail.get(), 0, (size_t)ctx->P.n_replicas * ctx->env_mail_bytes, (hipStream_t)stream));
      HIP_TRY(hipEventRecord(ctx->srv_go.get(), (hipStream_t)stream));
      HIP_TRY(hipStreamWaitEvent(ctx->srv_stream.get(), ctx->srv_go.get(), 0));
    }
    HIP_TRY(launch_plan(plan, Pb, n, ctx->sweep_dev.get(), (hipStream_t)stream, ctx->srv_stream.get()));
    ctx->last_row = plan.row;
    if (plan.server)
    {
      HIP_TRY(hipEventRecord(ctx->srv_done.get(), ctx->srv_stream.get()));
      HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ctx->srv_done.get(), 0));
    }
  }
  HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load.get(), (hipStream_t)stream));
  ctx->trials_run += n_trials;
  return GRLX_OK;
}

namespace grlx {

int status_to_error(uint64_t st)
{
  if (st & ST_TABLE_FULL) return fail(GRLX_ERR_TABLE_FULL, "a replica's sparse weight table overflowed: raise table_log2_capacity");
  if (st & ST_TRACE_OVERFLOW) return fail(GRLX_ERR_INVALID, "register trace overflow");
  if (st & ST_BAD_POS) return fail(GRLX_ERR_INVALID, "internal error: a TD update was queued without a table position");
  if (st & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "sin/cos argument outside |x| < 2^20");
  if (st & ST_ROWS_FULL) return fail(GRLX_ERR_ROWS_FULL, "more test rows than max_rows");
  return GRLX_OK;
}

// ---- hyper-parameter sweep: alpha, gamma, lambda, epsilon per replica --------------------------------------------------------------
static const char *const kSweepParamName[4] = {"alpha", "gamma", "lambda", "epsilon"};

static double sweep_config_value(const grlx_ctx *ctx, int param)
{
  const double v[4] = {ctx->cfg.alpha, ctx->cfg.gamma, ctx->cfg.lambda, ctx->cfg.epsilon};      // [GRLX_PARAM_*]
  return v[param];
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


// the layouts of more than 8 replicas per wave are not built for a sweep: the automatic choice falls back to 8
void sweep_limits_layout(DevParams &P)
{
  if (P.replicas_per_wave > 8) P.replicas_per_wave = 8;
}
} // namespace grlx

extern "C" {

// diagnostic (not part of include/grlx.h): the mailboxes of the environment server after the last launch (GRLX_ENV_SERVER_STATS builds
// leave cycle counts in EnvMail::stats)
int grlx_env_server_debug(grlx_ctx *ctx, void *out, size_t bytes)
{
  if (!ctx || !out) return fail(GRLX_ERR_INVALID, "bad argument");
  if (!ctx->env_mail) return fail(GRLX_ERR_INVALID, "the environment server has not run in this context");
  DRAIN(ctx);
  const size_t have = (size_t)ctx->P.n_replicas * ctx->env_mail_bytes;
  HIP_TRY(hipMemcpy(out, ctx->env_mail.get(), bytes < have ? bytes : have, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// diagnostic (not part of include/grlx.h): in the last launch that had the environment server, how many replicas took every step from it
// and how many gave up waiting and integrated themselves; both 0 when no launch of this context had it
int grlx_env_server_counts(grlx_ctx *ctx, int *served, int *fell_back)
{
  if (!ctx || !served || !fell_back) return fail(GRLX_ERR_INVALID, "bad argument");
  *served = *fell_back = 0;
  std::vector<int32_t> flag((size_t)ctx->P.n_replicas);
  const int rc = grlx_env_server_flags(ctx, flag.data(), ctx->P.n_replicas);      // zeros when no launch of this context had the server
  for (int32_t f : flag)
  {
    if (f == 1) ++*served;
    if (f == 2) ++*fell_back;
  }
  return rc;
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
  HIP_TRY(hipMemcpy2D(out, sizeof(unsigned long long), (const char *)ctx->env_mail.get() + kEnvMailUniformOffset, ctx->env_mail_bytes,
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
  HIP_TRY(hipMemcpy2D(flag.data(), sizeof(unsigned long long), (const char *)ctx->env_mail.get() + kEnvMailFlagOffset, ctx->env_mail_bytes,
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

int grlx_sync(grlx_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  uint64_t h[3];
  if ((hipStream_t)stream != ctx->run_stream) DRAIN(ctx);
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch.get(), (hipStream_t)stream));
  HIP_TRY(hipMemcpyAsync(h, ctx->scratch.get(), sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if ((hipStream_t)stream == ctx->run_stream) ctx->run_pending = false;
  return status_to_error(h[2]);
}

int grlx_step_counts(grlx_ctx *ctx, uint64_t *learn_steps, uint64_t *test_steps)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  uint64_t h[3];
  DRAIN(ctx);
  HIP_TRY(launch_step_counts(ctx->P, ctx->scratch.get(), nullptr));
  HIP_TRY(hipMemcpy(h, ctx->scratch.get(), sizeof(h), hipMemcpyDeviceToHost));
  if (learn_steps) *learn_steps = h[0];
  if (test_steps) *test_steps = h[1];
  return GRLX_OK;
}

int grlx_rows(grlx_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  ReplicaState s;
  DRAIN(ctx);
  if (read_state(ctx, 0, &s) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemcpy failed");
  return (int)s.rows;
}

int grlx_replica_rows(grlx_ctx *ctx, int replica)
{
  if (!ctx || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  if (read_state(ctx, replica, &s) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemcpy failed");
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
  if (reward) HIP_TRY(hipMemcpy2D(reward, sizeof(double), ctx->row_reward.get() + at, N * sizeof(double), sizeof(double), (size_t)count, hipMemcpyDeviceToHost));
  if (steps) HIP_TRY(hipMemcpy2D(steps, sizeof(int64_t), ctx->row_steps.get() + at, N * sizeof(int64_t), sizeof(int64_t), (size_t)count, hipMemcpyDeviceToHost));
  if (trial) HIP_TRY(hipMemcpy2D(trial, sizeof(int64_t), ctx->row_trial.get() + at, N * sizeof(int64_t), sizeof(int64_t), (size_t)count, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipMemcpy2D(episode_time, sizeof(double), ctx->row_time.get() + (size_t)first * N + (size_t)replica, N * sizeof(double), sizeof(double),
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
  STREAM_REFUSES(ctx, "grlx_set_replica_params");
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
  Dev<SweepParams> fresh;
  if (!ctx->sweep_dev)
  {
    const hipError_t e = fresh.alloc(sizeof(SweepParams) * N);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? GRLX_ERR_OOM : GRLX_ERR_HIP, "hipMalloc of the per-replica parameters failed: %s", hipGetErrorString(e));
  }
  HIP_TRY(hipMemcpy(fresh ? fresh.get() : ctx->sweep_dev.get(), rec.data(), sizeof(SweepParams) * N, hipMemcpyHostToDevice));
  if (fresh) ctx->sweep_dev = std::move(fresh);
  ctx->sweep_host[param] = std::move(v[param]);
  ctx->sweep = true;
  sweep_limits_layout(ctx->P);
  return GRLX_OK;
}

int grlx_curve_stats(grlx_ctx *ctx, int first, int count, double *out_dev, void *stream)
{
  if (!ctx || !out_dev || first < 0 || count < 0 || first + count > ctx->P.max_rows) return fail(GRLX_ERR_INVALID, "bad argument");
  if ((hipStream_t)stream != ctx->run_stream) DRAIN(ctx);
  HIP_TRY(launch_curve_stats(ctx->P, first, count, out_dev, (hipStream_t)stream));
  return GRLX_OK;
}

} // extern "C"
