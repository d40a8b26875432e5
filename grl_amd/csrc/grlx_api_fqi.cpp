// grlx_api_fqi.cpp -- the C ABI declared in include/grlx.h: the batch path (grlx_fqi_*) -- its context, a batch, the getters, and its read
// side: the policy query, greedy episodes and their trajectories, per replica and per group of replicas (the kernels: grlx_fqi.hip).
#include <memory>
#include "grlx_host.h"
#include "grlx_read.h"
#include "grlx_fqi.h"

struct grlx_fqi_ctx {
  grlx_fqi_config cfg;
  FqiParams F;
  std::vector<DevBuf> bufs;          // what F's pointers and r0 point to
  uint64_t *r0 = nullptr;
  int batches_run = 0;
  FqiLaunchPlan plan;
};

namespace {

template <typename T> int dev_alloc(grlx_fqi_ctx *ctx, T **p, size_t n)
{
  DevBuf b;
  if (b.alloc(n * sizeof(T)) != hipSuccess) return fail(GRLX_ERR_OOM, "out of device memory (%zu bytes)", n * sizeof(T));
  if (hipMemset(b.get(), 0, n * sizeof(T)) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemset failed");
  *p = b.as<T>();
  ctx->bufs.push_back(std::move(b));
  return GRLX_OK;
}

// what both queries check before they touch the device
int fqi_query_admit(const grlx_fqi_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *obs, int n_obs)
{
  if (!obs) return fail(GRLX_ERR_INVALID, "%s: obs is null", who);
  if (n_obs < 0) return fail(GRLX_ERR_INVALID, "%s: n_obs = %d", who, n_obs);
  if (int rc = replica_range_ok(who, ctx->F.R, first_replica, n_replicas)) return rc;
  for (int o = 0; o < n_obs; ++o)
    for (int d = 0; d < kFqiD; ++d)
      if (!std::isfinite(obs[(size_t)o * kFqiD + d])) return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d is not finite", who, o, d);
  return GRLX_OK;
}

// ---- greedy evaluation episodes: one per (replica, start state) pair, or per (group, start state) pair on the group's vote or mean Q.
// The kernels write every output of a pair, and behind an episode's end the zeros of its records, themselves: nothing is cleared here.
// what every episode call checks before it touches the device
int fqi_evaluate_admit(grlx_fqi_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  return episode_pairs_ok(who, ctx->F.R, kFqiS, first_replica, n_replicas, states, n_starts, max_steps);
}

// (the outputs and the chunk of an admitted call: batch_episodes, grlx_read.h, shared with the LSPI context)
int fqi_evaluate_impl(grlx_fqi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                      int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  if (int rc = fqi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kFqiS, n_replicas, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {}, records, kFqiTrajWords))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kFqiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    FqiEvalArgs A;
    A.first_replica = first_replica; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.records = d[6].as<double>();      // (past the outputs: null, the sums alone)
    HIP_TRY(launch_fqi_evaluate(ctx->F, A, n_replicas, nullptr));
    return GRLX_OK;
  });
}

int fqi_evaluate_ensemble_impl(grlx_fqi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size, int rule,
                               const double *states, int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                               int32_t *ties, int64_t *member_ties, int64_t *agreement, double *final_state, double *records)
{
  if (int rc = fqi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_ensemble_admit(who, n_replicas, group_size)) return rc;
  if (rule != GRLX_ENSEMBLE_VOTE && rule != GRLX_ENSEMBLE_MEAN_Q)
    return fail(GRLX_ERR_INVALID, "%s: rule = %d is neither GRLX_ENSEMBLE_VOTE (0) nor GRLX_ENSEMBLE_MEAN_Q (1)", who, rule);
  const int groups = n_replicas / group_size;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kFqiS, groups, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {member_ties, agreement}, records,
                            kFqiEnsTrajWords))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kFqiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    FqiEnsArgs A;
    A.first_replica = first_replica; A.group_size = group_size; A.rule = rule; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.member_ties = d[6].as<int64_t>(); A.agreement = d[7].as<int64_t>(); A.records = d[8].as<double>();
    HIP_TRY(launch_fqi_evaluate_ensemble(ctx->F, A, groups, nullptr));
    return GRLX_OK;
  });
}

// ---- sampled episodes: the samplers of one network, the draw from a group's majority or rank votes; what they check beyond their greedy
// siblings: grlx_read.h (batch_sampled_admit, batch_ensemble_sampled_admit)
int fqi_evaluate_sampled_impl(grlx_fqi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                              int max_steps, int sampler, double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps,
                              int32_t *terminal, int32_t *ties, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  if (int rc = fqi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_sampled_admit(who, n_replicas, n_starts, sampler, epsilon, streams)) return rc;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kFqiS, n_replicas, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {}, records, kFqiSampledTrajWords,
                            {ReadOut{explored, sizeof(int32_t), n_replicas, true}, ReadOut{streams_out, 2 * sizeof(uint64_t), n_replicas, true}},
                            2 * sizeof(uint64_t)))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  ReadIn in_streams = {streams, 2 * sizeof(uint64_t), n_replicas, nullptr};      // [replica][start][2]: a chunk is strided, not contiguous
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kFqiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    FqiSampledArgs T;
    FqiEvalArgs &A = T.e;
    A.first_replica = first_replica; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.records = d[8].as<double>();      // (past the outputs: null, the sums alone)
    T.sampler = sampler; T.epsilon = epsilon; T.streams = (const uint64_t *)in_streams.dev;
    T.explored = d[6].as<int32_t>(); T.streams_out = d[7].as<uint64_t>();
    HIP_TRY(launch_fqi_evaluate_sampled(ctx->F, T, n_replicas, nullptr));
    return GRLX_OK;
  }, &in_streams);
}

int fqi_evaluate_ensemble_sampled_impl(grlx_fqi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size, int strategy,
                                       double tau, int member, double member_param, const double *states, int n_starts, int max_steps,
                                       const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                       int64_t *member_ties, int64_t *agreement, int32_t *explored, double *final_state, uint64_t *streams_out,
                                       double *records)
{
  if (int rc = fqi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_ensemble_sampled_admit(who, n_replicas, group_size, n_starts, strategy, tau, member, member_param, streams)) return rc;
  const int groups = n_replicas / group_size;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kFqiS, groups, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {member_ties, agreement}, records,
                            kFqiEnsSampledTrajWords,
                            {ReadOut{explored, sizeof(int32_t), groups, true}, ReadOut{streams_out, sizeof(uint64_t), groups, true}}, sizeof(uint64_t)))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  ReadIn in_streams = {streams, sizeof(uint64_t), groups, nullptr};      // [group][start]: a chunk is strided
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kFqiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    FqiEnsSampledArgs T;
    FqiEnsArgs &A = T.e;
    A.first_replica = first_replica; A.group_size = group_size; A.rule = strategy; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.member_ties = d[6].as<int64_t>(); A.agreement = d[7].as<int64_t>(); A.records = d[10].as<double>();
    T.tau = tau; T.member = member; T.member_param = member_param; T.streams = (const uint64_t *)in_streams.dev;
    T.explored = d[8].as<int32_t>(); T.streams_out = d[9].as<uint64_t>();
    HIP_TRY(launch_fqi_evaluate_ensemble_sampled(ctx->F, T, groups, nullptr));
    return GRLX_OK;
  }, &in_streams);
}

} // namespace

extern "C" {

void grlx_fqi_config_pendulum(grlx_fqi_config *c)
{ // the reference's tests/pendulum-fqi-ann.yaml
  memset(c, 0, sizeof(*c));
  c->struct_size = sizeof(grlx_fqi_config);
  c->n_replicas = 1;
  c->env = GRLX_ENV_PENDULUM;
  c->control_step = 0.03;
  c->integration_steps = 5;
  c->timeout = 2.99;
  c->action_min = -3;
  c->action_max = 3;
  c->action_steps = 3;
  c->gamma = 0.97;
  c->batch_size = 1000;
  c->max_batches = 2;
  c->iterations = 10;
  c->epochs = 500;
  c->hidden = 20;
}

int grlx_fqi_create(const grlx_fqi_config *cfg, const int64_t *seeds, grlx_fqi_ctx **out)
{
  if (!cfg || !seeds || !out) return fail(GRLX_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(grlx_fqi_config)) return fail(GRLX_ERR_INVALID, "grlx_fqi_config.struct_size mismatch");
  if (cfg->env != GRLX_ENV_PENDULUM) return fail(GRLX_ERR_INVALID, "experiment/batch_learning: the task must support invert(); built for task/pendulum/swingup");
  if (!(cfg->eta >= -2. && cfg->eta <= 2.)) return fail(GRLX_ERR_INVALID, "representation/parameterized/ann:eta = %g outside [-2, 2] (ann.cpp:61)", cfg->eta);
  if (!fqi_width_built(cfg->hidden))
    return fail(GRLX_ERR_INVALID, "representation/parameterized/ann:hiddens = [%d] is not built (instantiated: [8], [16], [20], [32], [64])", cfg->hidden);
  if (cfg->n_replicas < 1 || cfg->batch_size < 1 || cfg->max_batches < 1 || cfg->iterations < 1 || cfg->epochs < 0)
    return fail(GRLX_ERR_INVALID, "n_replicas, batch_size, max_batches, iterations must be >= 1");
  if (cfg->action_steps < 1 || cfg->action_steps > GRLX_MAX_ACTIONS) return fail(GRLX_ERR_INVALID, "discretizer/uniform:steps");
  if (!(cfg->action_min < cfg->action_max) || !(cfg->control_step > 0) || cfg->integration_steps < 1 || !std::isfinite(cfg->timeout) || cfg->timeout < 0)
    return fail(GRLX_ERR_INVALID, "model / task parameters");
  if (std::ceil(cfg->timeout / cfg->control_step) + 1 > (double)GRLX_MAX_EPISODE_STEPS) return fail(GRLX_ERR_INVALID, "task:timeout exceeds GRLX_MAX_EPISODE_STEPS");
  if ((double)cfg->batch_size * cfg->max_batches > 2e8) return fail(GRLX_ERR_INVALID, "transition store too large");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback"); }

  std::unique_ptr<grlx_fqi_ctx> ctx(new grlx_fqi_ctx());      // released into *out at the end: every refusal below frees what was made
  ctx->cfg = *cfg;
  FqiParams &F = ctx->F;
  memset(&F, 0, sizeof(F));
  F.env.env = GRLX_ENV_PENDULUM;
  F.env.integration_steps = cfg->integration_steps;
  F.env.h = cfg->control_step / (double)(size_t)cfg->integration_steps;
  F.env.timeout = cfg->timeout;
  F.env.randomization = 0;
  F.R = cfg->n_replicas;
  F.H = cfg->hidden;
  F.P = (kFqiNIn + 1) * F.H + F.H + 1;
  F.A = cfg->action_steps;
  F.batch_size = cfg->batch_size;
  F.cap = cfg->batch_size * cfg->max_batches;
  F.chunks_cap = (F.cap + 63) / 64;
  F.max_rows = cfg->max_batches;
  {
    const double range = cfg->action_max - cfg->action_min;
    double delta = range / ((double)cfg->action_steps - 1);
    if (std::isnan(delta)) delta = 0.;
    for (int k = 0; k < cfg->action_steps; ++k) F.actions[k] = cfg->action_min + delta * k;
  }
  const double omin[2] = {0., -12 * M_PI}, omax[2] = {2 * M_PI, 12 * M_PI};      // pendulum.cpp:84-85
  for (int i = 0; i < kFqiD; ++i)
  {
    F.obs_min[i] = omin[i];
    F.obs_range[i] = omax[i] - omin[i];
    F.in_min[i] = omin[i];
    F.in_scale[i] = 1. / (omax[i] - omin[i]) * (1 + 0);
  }
  F.action_min = cfg->action_min;
  F.action_range = cfg->action_max - cfg->action_min;
  F.in_min[kFqiD] = cfg->action_min;
  F.in_scale[kFqiD] = 1. / (cfg->action_max - cfg->action_min) * (1 + 0);
  F.gamma_tau = pow(cfg->gamma, cfg->control_step);                               // pow(gamma_, tau), tau = control_step
  F.eta = cfg->eta;

  const size_t R = (size_t)F.R, cap = (size_t)F.cap;
  int rc = GRLX_OK;
  if ((rc = dev_alloc(ctx.get(), &F.rep, R)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &F.in, R * cap * kFqiNIn)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.next_obs, R * cap * kFqiD)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &F.reward, R * cap)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.targets, R * cap)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &F.absorbing, R * cap)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.net, R * 4 * (size_t)F.P)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.vL, 2 * R * 64 * (size_t)(F.P + 1))) != GRLX_OK || (rc = dev_alloc(ctx.get(), &F.sync, R * 4)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.row_reward, R * (size_t)F.max_rows)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.row_batch, R * (size_t)F.max_rows)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &F.row_transitions, R * (size_t)F.max_rows)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &ctx->r0, R)) != GRLX_OK)
    return rc;
  // instantiate order of the yaml (oracle/fqi.c: orc_fqi_create): sampler/greedy Rand = global lrand48 #1, the
  // thread-local RandGen = global lrand48 #2; the weight-initialisation stream of deviation D1 = srand48_r(seed)
  std::vector<FqiRep> hr(R);
  std::vector<uint64_t> hr0(R);
  for (size_t r = 0; r < R; ++r)
  {
    memset(&hr[r], 0, sizeof(FqiRep));
    uint64_t G = h_seed((long)seeds[r]);
    G = h_next(G);                                   // sampler's private Rand (never drawn from: ties use the global stream)
    G = h_next(G);
    hr[r].TL = h_seed((long)(G >> 17));
    hr[r].G = G;
    hr0[r] = h_seed((long)seeds[r]);
  }
  if (hipMemcpy(F.rep, hr.data(), sizeof(FqiRep) * R, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ctx->r0, hr0.data(), sizeof(uint64_t) * R, hipMemcpyHostToDevice) != hipSuccess)
    return fail(GRLX_ERR_HIP, "hipMemcpy failed");
  {
    int dev = 0, cus = 0, per_cu = 0;
    const hipError_t occ = fqi_epochs_shape(F.H, &ctx->plan, &per_cu);
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        occ != hipSuccess || cus * per_cu < ctx->plan.blocks_per_replica)
      return fail(GRLX_ERR_HIP, "fqi_epochs_kernel: the device cannot hold the %d resident blocks of one replica", ctx->plan.blocks_per_replica);
    ctx->plan.replicas_per_launch = (cus * per_cu) / ctx->plan.blocks_per_replica;
  }
  if (const char *nc = getenv("GRLX_FQI_NO_COOP")) ctx->plan.plain_launch = nc[0] && nc[0] != '0';
  if (const char *st = getenv("GRLX_FQI_STAMPS"))
    if (st[0] && st[0] != '0' && (rc = dev_alloc(ctx.get(), &F.stamps, R * kFqiStampBlocks * 4 * 8)) != GRLX_OK) return rc;
  if (launch_fqi_init(F, ctx->r0, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(GRLX_ERR_HIP, "fqi_init_kernel failed");
  *out = ctx.release();
  return GRLX_OK;
}

int grlx_fqi_destroy(grlx_fqi_ctx *ctx)
{
  delete ctx;
  return GRLX_OK;
}

int grlx_fqi_run_batch(grlx_fqi_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  if (ctx->batches_run >= ctx->cfg.max_batches) return fail(GRLX_ERR_ROWS_FULL, "more batches than max_batches");
  HIP_TRY(launch_fqi_batch(ctx->F, ctx->plan, ctx->batches_run, ctx->cfg.iterations, ctx->cfg.epochs, (hipStream_t)stream));
  ctx->batches_run++;
  return GRLX_OK;
}

int grlx_fqi_sync(grlx_fqi_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  std::vector<FqiRep> hr((size_t)ctx->F.R);
  HIP_TRY(hipMemcpy(hr.data(), ctx->F.rep, sizeof(FqiRep) * hr.size(), hipMemcpyDeviceToHost));
  uint32_t st = 0;
  for (const FqiRep &r : hr) st |= r.status;
  if (st & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "sin/cos argument outside |x| < 2^20");
  if (st & ST_ROWS_FULL) return fail(GRLX_ERR_ROWS_FULL, "more batches than max_batches");
  if (st & ST_SYNC_TIMEOUT) return fail(GRLX_ERR_HIP, "fqi_epochs_kernel: a wait between the blocks of a replica timed out (were all of its blocks resident?)");
  return GRLX_OK;
}

int grlx_fqi_read_rows(grlx_fqi_ctx *ctx, int replica, int first, int count, int64_t *batch, int64_t *transitions, double *reward)
{
  if (!ctx || replica < 0 || replica >= ctx->F.R || first < 0 || count < 0 || first + count > ctx->F.max_rows) return fail(GRLX_ERR_INVALID, "bad argument");
  if (count == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t at = (size_t)replica * (size_t)ctx->F.max_rows + (size_t)first;
  if (batch) HIP_TRY(hipMemcpy(batch, ctx->F.row_batch + at, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost));
  if (transitions) HIP_TRY(hipMemcpy(transitions, ctx->F.row_transitions + at, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(hipMemcpy(reward, ctx->F.row_reward + at, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_fqi_get_params(grlx_fqi_ctx *ctx, int replica, double *out, int n)
{
  if (!ctx || !out || replica < 0 || replica >= ctx->F.R || n != ctx->F.P) return fail(GRLX_ERR_INVALID, "bad argument (the network has %d parameters)", ctx ? ctx->F.P : 0);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ctx->F.net + (size_t)replica * 4 * (size_t)ctx->F.P, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_fqi_get_transitions(grlx_fqi_ctx *ctx, int replica, int first, int count, double *in, double *next_obs, double *reward, double *targets)
{
  if (!ctx || replica < 0 || replica >= ctx->F.R || first < 0 || count < 0 || first + count > ctx->F.cap) return fail(GRLX_ERR_INVALID, "bad argument");
  if (count == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t at = (size_t)replica * (size_t)ctx->F.cap + (size_t)first;
  if (in) HIP_TRY(hipMemcpy(in, ctx->F.in + at * kFqiNIn, sizeof(double) * (size_t)count * kFqiNIn, hipMemcpyDeviceToHost));
  if (next_obs) HIP_TRY(hipMemcpy(next_obs, ctx->F.next_obs + at * kFqiD, sizeof(double) * (size_t)count * kFqiD, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(hipMemcpy(reward, ctx->F.reward + at, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  if (targets) HIP_TRY(hipMemcpy(targets, ctx->F.targets + at, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// diagnostic, not part of include/grlx.h: the stamps of the LAST fqi_epochs_kernel launch (GRLX_FQI_STAMPS=1 at create)
int grlx_fqi_debug_stamps(grlx_fqi_ctx *ctx, unsigned long long *out, int count)
{
  if (!ctx || !out || !ctx->F.stamps || count != ctx->F.R * kFqiStampBlocks * 4 * 8) return fail(GRLX_ERR_INVALID, "no stamps (GRLX_FQI_STAMPS=1 at create; count = R * 512)");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ctx->F.stamps, sizeof(unsigned long long) * (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_fqi_info(grlx_fqi_ctx *ctx, int replica, int64_t *n_transitions, double *maxdelta, int32_t *iterations, double *error, uint64_t rng[2])
{
  if (!ctx || replica < 0 || replica >= ctx->F.R) return fail(GRLX_ERR_INVALID, "bad argument");
  HIP_TRY(hipDeviceSynchronize());
  FqiRep r;
  HIP_TRY(hipMemcpy(&r, ctx->F.rep + replica, sizeof(r), hipMemcpyDeviceToHost));
  if (n_transitions) *n_transitions = r.n;
  if (maxdelta) *maxdelta = r.done ? r.maxdelta_last : __builtin_bit_cast(double, r.maxdelta_bits);
  if (iterations) *iterations = r.iterations;
  if (error) *error = r.last_error;
  if (rng) { rng[0] = r.G; rng[1] = r.TL; }
  return GRLX_OK;
}

// ---- the read side.  Every call reads F.net, F.env and the projector's constants only: nothing of the context changes.  The reads go
// through the skeleton of grlx_read.h without the online contexts' hooks: no poison launch, and grlx_read_kernel_timing does not count them.

// Q(s, a_k) of each replica's CURRENT parameters at observations of the caller's choice: q[replica][n_obs][A]
int grlx_fqi_query(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *obs, int n_obs, double *q)
{
  if (!ctx || !q) return fail(GRLX_ERR_INVALID, "bad argument");
  if (int rc = fqi_query_admit(ctx, "grlx_fqi_query", first_replica, n_replicas, obs, n_obs)) return rc;
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t elem = sizeof(double) * (size_t)ctx->F.A;
  const int chunk = query_chunk(n_obs, sizeof(double) * kFqiD + elem * (size_t)n_replicas);
  const ReadOut outs[1] = {{q, elem, n_replicas, true}};
  return chunked_read(kPlainRead, outs, 1, n_obs, obs, kFqiD, chunk, false, [&](int nc, const double *dobs, const DevPtr *d) -> int {
    HIP_TRY(launch_fqi_query(ctx->F, first_replica, n_replicas, dobs, nc, d[0].as<double>(), nullptr));
    return GRLX_OK;
  });
}

// grlx_query_ensemble's columns over groups of group_size consecutive replicas: out[group][n_obs][2 + 2 A]
int grlx_fqi_query_ensemble(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, const double *obs, int n_obs, double *out)
{
  const char *who = "grlx_fqi_query_ensemble";
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return fail(GRLX_ERR_INVALID, "%s: out is null", who);
  if (int rc = fqi_query_admit(ctx, who, first_replica, n_replicas, obs, n_obs)) return rc;
  if (int rc = batch_ensemble_admit(who, n_replicas, group_size)) return rc;
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const int groups = n_replicas / group_size;
  const size_t elem = sizeof(double) * (2 + 2 * (size_t)ctx->F.A);
  const int chunk = query_chunk(n_obs, sizeof(double) * kFqiD + elem * (size_t)groups);
  const ReadOut outs[1] = {{out, elem, groups, true}};
  return chunked_read(kPlainRead, outs, 1, n_obs, obs, kFqiD, chunk, false, [&](int nc, const double *dobs, const DevPtr *d) -> int {
    HIP_TRY(launch_fqi_query_ensemble(ctx->F, first_replica, groups, group_size, dobs, nc, d[0].as<double>(), nullptr));
    return GRLX_OK;
  });
}

int grlx_fqi_evaluate(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret, double *disc,
                      int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state)
{
  return fqi_evaluate_impl(ctx, "grlx_fqi_evaluate", nullptr, first_replica, n_replicas, states, n_starts, max_steps, ret, disc, steps, terminal, ties,
                           final_state, nullptr);
}

int grlx_fqi_trajectory_record_words(grlx_fqi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_fqi_trajectory_record_words: ctx is null");
  return kFqiTrajWords;
}

int grlx_fqi_evaluate_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret,
                                 double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  return fqi_evaluate_impl(ctx, "grlx_fqi_evaluate_trajectory", "grlx_fqi_evaluate", first_replica, n_replicas, states, n_starts, max_steps, ret, disc, steps,
                           terminal, ties, final_state, records);
}

int grlx_fqi_evaluate_ensemble(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                               int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                               int64_t *agreement, double *final_state)
{
  return fqi_evaluate_ensemble_impl(ctx, "grlx_fqi_evaluate_ensemble", nullptr, first_replica, n_replicas, group_size, rule, states, n_starts, max_steps, ret,
                                    disc, steps, terminal, ties, member_ties, agreement, final_state, nullptr);
}

int grlx_fqi_ensemble_trajectory_record_words(grlx_fqi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_fqi_ensemble_trajectory_record_words: ctx is null");
  return kFqiEnsTrajWords;
}

int grlx_fqi_evaluate_ensemble_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                                          int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                          int64_t *member_ties, int64_t *agreement, double *final_state, double *records)
{
  return fqi_evaluate_ensemble_impl(ctx, "grlx_fqi_evaluate_ensemble_trajectory", "grlx_fqi_evaluate_ensemble", first_replica, n_replicas, group_size, rule,
                                    states, n_starts, max_steps, ret, disc, steps, terminal, ties, member_ties, agreement, final_state, records);
}

int grlx_fqi_evaluate_sampled(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler,
                              double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                              int32_t *explored, double *final_state, uint64_t *streams_out)
{
  return fqi_evaluate_sampled_impl(ctx, "grlx_fqi_evaluate_sampled", nullptr, first_replica, n_replicas, states, n_starts, max_steps, sampler, epsilon, streams,
                                   ret, disc, steps, terminal, ties, explored, final_state, streams_out, nullptr);
}

int grlx_fqi_sampled_trajectory_record_words(grlx_fqi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_fqi_sampled_trajectory_record_words: ctx is null");
  return kFqiSampledTrajWords;
}

int grlx_fqi_evaluate_sampled_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler,
                                         double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                                         int32_t *ties, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  return fqi_evaluate_sampled_impl(ctx, "grlx_fqi_evaluate_sampled_trajectory", "grlx_fqi_evaluate_sampled", first_replica, n_replicas, states, n_starts,
                                   max_steps, sampler, epsilon, streams, ret, disc, steps, terminal, ties, explored, final_state, streams_out, records);
}

int grlx_fqi_evaluate_ensemble_sampled(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int strategy, double tau, int member,
                                       double member_param, const double *states, int n_starts, int max_steps, const uint64_t *streams, double *ret,
                                       double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties, int64_t *agreement,
                                       int32_t *explored, double *final_state, uint64_t *streams_out)
{
  return fqi_evaluate_ensemble_sampled_impl(ctx, "grlx_fqi_evaluate_ensemble_sampled", nullptr, first_replica, n_replicas, group_size, strategy, tau, member,
                                            member_param, states, n_starts, max_steps, streams, ret, disc, steps, terminal, ties, member_ties, agreement,
                                            explored, final_state, streams_out, nullptr);
}

int grlx_fqi_ensemble_sampled_trajectory_record_words(grlx_fqi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_fqi_ensemble_sampled_trajectory_record_words: ctx is null");
  return kFqiEnsSampledTrajWords;
}

int grlx_fqi_evaluate_ensemble_sampled_trajectory(grlx_fqi_ctx *ctx, int first_replica, int n_replicas, int group_size, int strategy, double tau, int member,
                                                  double member_param, const double *states, int n_starts, int max_steps, const uint64_t *streams,
                                                  double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                                                  int64_t *agreement, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  return fqi_evaluate_ensemble_sampled_impl(ctx, "grlx_fqi_evaluate_ensemble_sampled_trajectory", "grlx_fqi_evaluate_ensemble_sampled", first_replica,
                                            n_replicas, group_size, strategy, tau, member, member_param, states, n_starts, max_steps, streams, ret, disc,
                                            steps, terminal, ties, member_ties, agreement, explored, final_state, streams_out, records);
}

} // extern "C"
