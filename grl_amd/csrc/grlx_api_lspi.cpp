// grlx_api_lspi.cpp -- the C ABI declared in include/grlx.h: least-squares policy iteration on the batch path (grlx_lspi_*) -- its
// context, a batch, the getters, the policy query (the kernels: grlx_lspi.hip; the specification: grlx_lspi.h), and the rest of its read
// side: greedy episodes and their trajectories, per replica and per group of replicas (the kernels: grlx_lspi_evaluate.hip), and the
// sampled ones (grlx_lspi_evaluate_sampled.hip).
#include <memory>
#include "grlx_host.h"
#include "grlx_read.h"
#include "grlx_lspi.h"
#include "grlx_lspi_evaluate.h"
#include "grlx_lspi_evaluate_sampled.h"

struct grlx_lspi_ctx {
  grlx_lspi_config cfg;
  LspiParams L;
  std::vector<DevBuf> bufs;          // what L's pointers and r0 point to
  uint64_t *r0 = nullptr;
  int batches_run = 0;
};

namespace {

template <typename T> int dev_alloc(grlx_lspi_ctx *ctx, T **p, size_t n)
{
  DevBuf b;
  if (b.alloc(n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return fail(GRLX_ERR_OOM, "out of device memory (%zu bytes)", n * sizeof(T)); }
  if (hipMemset(b.get(), 0, n * sizeof(T)) != hipSuccess) return fail(GRLX_ERR_HIP, "hipMemset failed");
  *p = b.as<T>();
  ctx->bufs.push_back(std::move(b));
  return GRLX_OK;
}

// what grlx_lspi_create checks before it asks for a device; every refusal names its field
int lspi_admit(const grlx_lspi_config *c)
{
  if (c->struct_size != sizeof(grlx_lspi_config)) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.struct_size mismatch");
  const struct { const char *name; double v; } reals[] = {{"control_step", c->control_step}, {"timeout", c->timeout}, {"action_min", c->action_min},
      {"action_max", c->action_max}, {"gamma", c->gamma}, {"sigma", c->sigma}, {"cutoff", c->cutoff}, {"init_min", c->init_min}, {"init_max", c->init_max}};
  for (const auto &f : reals)
    if (!std::isfinite(f.v)) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.%s is not finite (%g)", f.name, f.v);
  if (c->env != GRLX_ENV_PENDULUM) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.env = %d: experiment/batch_learning needs a task with invert(); built for task/pendulum/swingup", c->env);
  if (c->projector != GRLX_RBF_TRIANGLE && c->projector != GRLX_RBF_GAUSS)
    return fail(GRLX_ERR_INVALID, "grlx_lspi_config.projector = %d is neither GRLX_RBF_TRIANGLE (0) nor GRLX_RBF_GAUSS (1); projector/monomial is not built", c->projector);
  int64_t F = 1;
  for (int d = 0; d < kLspiNIn; ++d)
  {
    if (c->steps[d] < 2) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.steps[%d] = %d is below 2 (projector/rbf:steps)", d, c->steps[d]);
    F *= c->steps[d];
    if (F > kLspiMaxF) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.steps: more than %d features (the kernels are built for F <= %d)", kLspiMaxF, kLspiMaxF);
  }
  if (c->projector == GRLX_RBF_GAUSS)
  {
    if (!(c->sigma > 0)) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.sigma = %g is not above 0 (projector/rbf/gauss)", c->sigma);
    if (!(c->cutoff > 0 && c->cutoff < 1)) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.cutoff = %g is outside (0, 1) (projector/rbf/gauss)", c->cutoff);
  }
  if (c->n_replicas < 1 || c->batch_size < 1 || c->max_batches < 1 || c->iterations < 1)
    return fail(GRLX_ERR_INVALID, "grlx_lspi_config: n_replicas, batch_size, max_batches, iterations must be >= 1");
  if (c->action_steps < 1 || c->action_steps > GRLX_MAX_ACTIONS) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.action_steps (discretizer/uniform:steps) outside 1 ... %d", GRLX_MAX_ACTIONS);
  if (!(c->action_min < c->action_max)) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.action_min is not below action_max");
  if (!(c->control_step > 0) || c->integration_steps < 1) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.control_step / integration_steps (model/dynamical)");
  if (c->timeout < 0) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.timeout is negative");
  if (std::ceil(c->timeout / c->control_step) + 1 > (double)GRLX_MAX_EPISODE_STEPS) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.timeout exceeds GRLX_MAX_EPISODE_STEPS");
  if ((double)c->batch_size * c->max_batches > 2e8) return fail(GRLX_ERR_INVALID, "grlx_lspi_config.batch_size x max_batches: transition store too large");
  return GRLX_OK;
}

int lspi_replica_ok(const grlx_lspi_ctx *ctx, const char *who, int replica)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  if (replica < 0 || replica >= ctx->L.R) return fail(GRLX_ERR_INVALID, "%s: replica %d is outside the context's %d replicas", who, replica, ctx->L.R);
  return GRLX_OK;
}

// what both queries check before they touch the device
int lspi_query_admit(const grlx_lspi_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *obs, int n_obs)
{
  if (!obs) return fail(GRLX_ERR_INVALID, "%s: obs is null", who);
  if (n_obs < 0) return fail(GRLX_ERR_INVALID, "%s: n_obs = %d", who, n_obs);
  if (int rc = replica_range_ok(who, ctx->L.R, first_replica, n_replicas)) return rc;
  for (int o = 0; o < n_obs; ++o)
    for (int d = 0; d < kLspiD; ++d)
      if (!std::isfinite(obs[(size_t)o * kLspiD + d])) return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d is not finite", who, o, d);
  return GRLX_OK;
}

// ---- greedy evaluation episodes, after grlx_api_fqi.cpp's: one per (replica, start state) pair, or per (group, start state) pair on the
// group's vote or mean Q.  The kernels write every output of a pair, and behind an episode's end the zeros of its records, themselves.
int lspi_evaluate_admit(grlx_lspi_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  return episode_pairs_ok(who, ctx->L.R, kLspiS, first_replica, n_replicas, states, n_starts, max_steps);
}

int lspi_evaluate_impl(grlx_lspi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                       int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  if (int rc = lspi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kLspiS, n_replicas, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {}, records, kLspiTrajWords))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kLspiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    LspiEvalArgs A;
    A.first_replica = first_replica; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.records = d[6].as<double>();      // (past the outputs: null, the sums alone)
    HIP_TRY(launch_lspi_evaluate(ctx->L, A, n_replicas, nullptr));
    return GRLX_OK;
  });
}

int lspi_evaluate_ensemble_impl(grlx_lspi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size, int rule,
                                const double *states, int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                                int32_t *ties, int64_t *member_ties, int64_t *agreement, double *final_state, double *records)
{
  if (int rc = lspi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_ensemble_admit(who, n_replicas, group_size)) return rc;
  if (rule != GRLX_ENSEMBLE_VOTE && rule != GRLX_ENSEMBLE_MEAN_Q)
    return fail(GRLX_ERR_INVALID, "%s: rule = %d is neither GRLX_ENSEMBLE_VOTE (0) nor GRLX_ENSEMBLE_MEAN_Q (1)", who, rule);
  const int groups = n_replicas / group_size;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kLspiS, groups, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {member_ties, agreement}, records,
                             kLspiEnsTrajWords))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kLspiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    LspiEnsArgs A;
    A.first_replica = first_replica; A.group_size = group_size; A.rule = rule; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.member_ties = d[6].as<int64_t>(); A.agreement = d[7].as<int64_t>(); A.records = d[8].as<double>();
    HIP_TRY(launch_lspi_evaluate_ensemble(ctx->L, A, groups, nullptr));
    return GRLX_OK;
  });
}

// ---- sampled episodes, after grlx_api_fqi.cpp's: the samplers of one policy, the draw from a group's majority or rank votes (the kernels:
// grlx_lspi_evaluate_sampled.hip; what they check beyond their greedy siblings: grlx_read.h)
int lspi_evaluate_sampled_impl(grlx_lspi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                               int max_steps, int sampler, double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps,
                               int32_t *terminal, int32_t *ties, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  if (int rc = lspi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_sampled_admit(who, n_replicas, n_starts, sampler, epsilon, streams)) return rc;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kLspiS, n_replicas, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {}, records,
                             kLspiSampledTrajWords,
                             {ReadOut{explored, sizeof(int32_t), n_replicas, true}, ReadOut{streams_out, 2 * sizeof(uint64_t), n_replicas, true}},
                             2 * sizeof(uint64_t)))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  ReadIn in_streams = {streams, 2 * sizeof(uint64_t), n_replicas, nullptr};      // [replica][start][2]: a chunk is strided, not contiguous
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kLspiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    LspiSampledArgs T;
    LspiEvalArgs &A = T.e;
    A.first_replica = first_replica; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.records = d[8].as<double>();      // (past the outputs: null, the sums alone)
    T.sampler = sampler; T.epsilon = epsilon; T.streams = (const uint64_t *)in_streams.dev;
    T.explored = d[6].as<int32_t>(); T.streams_out = d[7].as<uint64_t>();
    HIP_TRY(launch_lspi_evaluate_sampled(ctx->L, T, n_replicas, nullptr));
    return GRLX_OK;
  }, &in_streams);
}

int lspi_evaluate_ensemble_sampled_impl(grlx_lspi_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size,
                                        int strategy, double tau, int member, double member_param, const double *states, int n_starts, int max_steps,
                                        const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                        int64_t *member_ties, int64_t *agreement, int32_t *explored, double *final_state, uint64_t *streams_out,
                                        double *records)
{
  if (int rc = lspi_evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  if (int rc = batch_ensemble_sampled_admit(who, n_replicas, group_size, n_starts, strategy, tau, member, member_param, streams)) return rc;
  const int groups = n_replicas / group_size;
  BatchEpisodes e;
  if (int rc = batch_episodes(e, who, sibling, kLspiS, groups, n_starts, &max_steps, ret, disc, steps, terminal, ties, final_state, {member_ties, agreement}, records,
                             kLspiEnsSampledTrajWords,
                             {ReadOut{explored, sizeof(int32_t), groups, true}, ReadOut{streams_out, sizeof(uint64_t), groups, true}}, sizeof(uint64_t)))
    return rc;
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  ReadIn in_streams = {streams, sizeof(uint64_t), groups, nullptr};      // [group][start]: a chunk is strided
  return chunked_read(kPlainRead, e.outs, e.n_outs, n_starts, states, kLspiS, e.chunk, true, [&](int nc, const double *dst, const DevPtr *d) -> int {
    LspiEnsSampledArgs T;
    LspiEnsArgs &A = T.e;
    A.first_replica = first_replica; A.group_size = group_size; A.rule = strategy; A.n_starts = nc; A.max_steps = max_steps; A.states = dst;
    A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
    A.final_state = d[5].as<double>(); A.member_ties = d[6].as<int64_t>(); A.agreement = d[7].as<int64_t>(); A.records = d[10].as<double>();
    T.tau = tau; T.member = member; T.member_param = member_param; T.cap = 0; T.streams = (const uint64_t *)in_streams.dev;
    T.explored = d[8].as<int32_t>(); T.streams_out = d[9].as<uint64_t>();
    HIP_TRY(launch_lspi_evaluate_ensemble_sampled(ctx->L, T, groups, nullptr));
    return GRLX_OK;
  }, &in_streams);
}

} // namespace

extern "C" {

void grlx_lspi_config_pendulum(grlx_lspi_config *c, int projector)
{ // the reference's cfg/pendulum/lspi_triangle.yaml / lspi_gauss.yaml
  memset(c, 0, sizeof(*c));
  c->struct_size = sizeof(grlx_lspi_config);
  c->n_replicas = 1;
  c->env = GRLX_ENV_PENDULUM;
  c->control_step = 0.03;
  c->integration_steps = 5;
  c->timeout = 2.99;
  c->action_min = -3;
  c->action_max = 3;
  c->action_steps = 3;
  c->batch_size = 10000;
  c->max_batches = 10;
  c->gamma = 0.97;
  c->iterations = 10;
  c->projector = projector;
  c->steps[0] = 11; c->steps[1] = 11; c->steps[2] = 3;
  c->sigma = 1;                      // rbf.h: the projector's default
  c->cutoff = 0.01;
  c->init_min = 0;
  c->init_max = 1;
}

int grlx_lspi_create(const grlx_lspi_config *cfg, const int64_t *seeds, grlx_lspi_ctx **out)
{
  if (!cfg || !seeds || !out) return fail(GRLX_ERR_INVALID, "grlx_lspi_create: null argument");
  *out = nullptr;
  if (int rc = lspi_admit(cfg)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(GRLX_ERR_NO_DEVICE, "no HIP device: grlx has no CPU fallback"); }

  std::unique_ptr<grlx_lspi_ctx> ctx(new grlx_lspi_ctx());
  ctx->cfg = *cfg;
  LspiParams &L = ctx->L;
  memset(&L, 0, sizeof(L));
  L.env.env = GRLX_ENV_PENDULUM;
  L.env.integration_steps = cfg->integration_steps;
  L.env.h = cfg->control_step / (double)(size_t)cfg->integration_steps;
  L.env.timeout = cfg->timeout;
  L.env.randomization = 0;
  L.R = cfg->n_replicas;
  L.A = cfg->action_steps;
  L.batch_size = cfg->batch_size;
  L.cap = cfg->batch_size * cfg->max_batches;
  L.max_rows = cfg->max_batches;
  L.projector = cfg->projector;
  {
    const double range = cfg->action_max - cfg->action_min;
    double delta = range / ((double)cfg->action_steps - 1);
    if (std::isnan(delta) || std::isinf(delta)) delta = 0.;
    for (int k = 0; k < cfg->action_steps; ++k) L.actions[k] = cfg->action_min + delta * k;
  }
  const double omin[2] = {0., -12 * M_PI}, omax[2] = {2 * M_PI, 12 * M_PI};      // pendulum.cpp:84-85
  const double imin[kLspiNIn] = {omin[0], omin[1], cfg->action_min}, imax[kLspiNIn] = {omax[0], omax[1], cfg->action_max};
  int F = 1;
  for (int d = 0; d < kLspiNIn; ++d)
  { // RBFProjector::configure (rbf.cpp:81-90)
    L.steps[d] = cfg->steps[d];
    L.stride[d] = F;
    F *= cfg->steps[d];
    L.in_min[d] = imin[d];
    L.delta[d] = (imax[d] - imin[d]) / ((double)cfg->steps[d] - 1);
    L.top[d] = (double)cfg->steps[d] - 1 - 1e-10;
  }
  for (int i = 0; i < kLspiD; ++i) { L.obs_min[i] = omin[i]; L.obs_range[i] = omax[i] - omin[i]; }
  L.action_min = cfg->action_min;
  L.action_range = cfg->action_max - cfg->action_min;
  L.F = F;
  L.Fp = lspi_padded(F);
  L.LP = L.Fp + 16;
  L.sigmasq = cfg->sigma * cfg->sigma;
  L.cutoff_distsq = -L.sigmasq * std::log(cfg->cutoff);                             // rbf.cpp:179-180 (deviation D4)
  L.gamma_tau = pow(cfg->gamma, cfg->control_step);
  L.init_min = cfg->init_min;
  L.init_range = cfg->init_max - cfg->init_min;
  const int T = L.Fp / 16, tiles = std::max(lspi_tiles(T, 0), lspi_tiles(T, 1));
  L.partials_per_replica = (size_t)lspi_splits(L.cap) * (size_t)tiles * 256;

  const size_t R = (size_t)L.R, cap = (size_t)L.cap, Fp = (size_t)L.Fp;
  int rc = GRLX_OK;
  if ((rc = dev_alloc(ctx.get(), &L.rep, R)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.in, R * cap * kLspiNIn)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.next_obs, R * cap * kLspiD)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.reward, R * cap)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.absorbing, R * cap)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.best, R * cap)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.w, R * 2 * Fp)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.As, R * Fp * Fp)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.Asys, R * Fp * Fp)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.b, R * Fp)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.lu, R * Fp * (size_t)L.LP)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.partials, R * L.partials_per_replica)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.row_reward, R * (size_t)L.max_rows)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &L.row_batch, R * (size_t)L.max_rows)) != GRLX_OK ||
      (rc = dev_alloc(ctx.get(), &L.row_transitions, R * (size_t)L.max_rows)) != GRLX_OK || (rc = dev_alloc(ctx.get(), &ctx->r0, R)) != GRLX_OK)
    return rc;
  // the streams of a replica, as grlx_fqi_create seeds them: the sampler's private Rand = global lrand48 #1, the thread-local RandGen =
  // global lrand48 #2; the initialisation stream of deviation D1 = srand48(seed)
  std::vector<LspiRep> hr(R);
  std::vector<uint64_t> hr0(R);
  for (size_t r = 0; r < R; ++r)
  {
    memset(&hr[r], 0, sizeof(LspiRep));
    uint64_t G = h_seed((long)seeds[r]);
    G = h_next(G);
    G = h_next(G);
    hr[r].TL = h_seed((long)(G >> 17));
    hr[r].G = G;
    hr0[r] = h_seed((long)seeds[r]);
  }
  if (hipMemcpy(L.rep, hr.data(), sizeof(LspiRep) * R, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ctx->r0, hr0.data(), sizeof(uint64_t) * R, hipMemcpyHostToDevice) != hipSuccess)
    return fail(GRLX_ERR_HIP, "hipMemcpy failed");
  if (launch_lspi_init(L, ctx->r0, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(GRLX_ERR_HIP, "lspi_init_kernel failed");
  *out = ctx.release();
  return GRLX_OK;
}

int grlx_lspi_destroy(grlx_lspi_ctx *ctx)
{
  delete ctx;
  return GRLX_OK;
}

int grlx_lspi_run_batch(grlx_lspi_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_run_batch: ctx is null");
  if (ctx->batches_run >= ctx->cfg.max_batches) return fail(GRLX_ERR_ROWS_FULL, "more batches than max_batches");
  HIP_TRY(launch_lspi_batch(ctx->L, ctx->batches_run, ctx->cfg.iterations, (hipStream_t)stream));
  ctx->batches_run++;
  return GRLX_OK;
}

int grlx_lspi_sync(grlx_lspi_ctx *ctx, void *stream)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_sync: ctx is null");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  std::vector<LspiRep> hr((size_t)ctx->L.R);
  HIP_TRY(hipMemcpy(hr.data(), ctx->L.rep, sizeof(LspiRep) * hr.size(), hipMemcpyDeviceToHost));
  uint32_t st = 0;
  for (const LspiRep &r : hr) st |= r.status;
  if (st & ST_DOMAIN) return fail(GRLX_ERR_DOMAIN, "sin/cos argument outside |x| < 2^20");
  if (st & ST_ROWS_FULL) return fail(GRLX_ERR_ROWS_FULL, "more batches than max_batches");
  if (st & ST_LSPI_PIVOT) return fail(GRLX_ERR_DOMAIN, "lspi_solve_kernel: a zero or non-finite pivot (the system of an iteration is singular)");
  return GRLX_OK;
}

int grlx_lspi_read_rows(grlx_lspi_ctx *ctx, int replica, int first, int count, int64_t *batch, int64_t *transitions, double *reward)
{
  if (int rc = lspi_replica_ok(ctx, "grlx_lspi_read_rows", replica)) return rc;
  if (first < 0 || count < 0 || (int64_t)first + count > ctx->L.max_rows)
    return fail(GRLX_ERR_INVALID, "grlx_lspi_read_rows: rows [%d, %lld) are outside the context's %d", first, (long long)first + count, ctx->L.max_rows);
  if (count == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t at = (size_t)replica * (size_t)ctx->L.max_rows + (size_t)first;
  if (batch) HIP_TRY(hipMemcpy(batch, ctx->L.row_batch + at, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost));
  if (transitions) HIP_TRY(hipMemcpy(transitions, ctx->L.row_transitions + at, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(hipMemcpy(reward, ctx->L.row_reward + at, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_lspi_get_params(grlx_lspi_ctx *ctx, int replica, int which, double *out, int n)
{
  if (int rc = lspi_replica_ok(ctx, "grlx_lspi_get_params", replica)) return rc;
  if (!out) return fail(GRLX_ERR_INVALID, "grlx_lspi_get_params: out is null");
  if (which != 0 && which != 1) return fail(GRLX_ERR_INVALID, "grlx_lspi_get_params: which = %d is neither 0 (current) nor 1 (of the last greedy choice)", which);
  if (n != ctx->L.F) return fail(GRLX_ERR_INVALID, "grlx_lspi_get_params: n = %d, the representation has %d parameters", n, ctx->L.F);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ctx->L.w + ((size_t)replica * 2 + (size_t)which) * (size_t)ctx->L.Fp, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_lspi_get_transitions(grlx_lspi_ctx *ctx, int replica, int first, int count, double *obs_action, double *next_obs, double *reward, int32_t *best)
{
  if (int rc = lspi_replica_ok(ctx, "grlx_lspi_get_transitions", replica)) return rc;
  if (first < 0 || count < 0 || (int64_t)first + count > ctx->L.cap)
    return fail(GRLX_ERR_INVALID, "grlx_lspi_get_transitions: transitions [%d, %lld) are outside the store's %d", first, (long long)first + count, ctx->L.cap);
  if (count == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t at = (size_t)replica * (size_t)ctx->L.cap + (size_t)first;
  if (obs_action) HIP_TRY(hipMemcpy(obs_action, ctx->L.in + at * kLspiNIn, sizeof(double) * (size_t)count * kLspiNIn, hipMemcpyDeviceToHost));
  if (next_obs) HIP_TRY(hipMemcpy(next_obs, ctx->L.next_obs + at * kLspiD, sizeof(double) * (size_t)count * kLspiD, hipMemcpyDeviceToHost));
  if (reward) HIP_TRY(hipMemcpy(reward, ctx->L.reward + at, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  if (best) HIP_TRY(hipMemcpy(best, ctx->L.best + at, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_lspi_get_system(grlx_lspi_ctx *ctx, int replica, double *A, double *b)
{
  if (int rc = lspi_replica_ok(ctx, "grlx_lspi_get_system", replica)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  const size_t F = (size_t)ctx->L.F, Fp = (size_t)ctx->L.Fp;
  if (A) HIP_TRY(hipMemcpy2D(A, F * sizeof(double), ctx->L.Asys + (size_t)replica * Fp * Fp, Fp * sizeof(double), F * sizeof(double), F, hipMemcpyDeviceToHost));
  if (b) HIP_TRY(hipMemcpy(b, ctx->L.b + (size_t)replica * Fp, F * sizeof(double), hipMemcpyDeviceToHost));
  return GRLX_OK;
}

// include/grlx_diag.h: lspi_solve_kernel on systems of the caller's choice, through the launch an iteration makes
int grlx_lspi_solve_systems(grlx_lspi_ctx *ctx, const double *A, const double *b, double *x)
{
  const char *who = "grlx_lspi_solve_systems";
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  if (!A) return fail(GRLX_ERR_INVALID, "%s: A is null", who);
  if (!b) return fail(GRLX_ERR_INVALID, "%s: b is null", who);
  if (!x) return fail(GRLX_ERR_INVALID, "%s: x is null", who);
  const LspiParams &L = ctx->L;
  const size_t R = (size_t)L.R, F = (size_t)L.F, Fp = (size_t)L.Fp;
  HIP_TRY(hipDeviceSynchronize());
  // rows of F doubles into rows of pitch Fp: the padding stays what it is, zero (the allocation's, or a rebuild's sums over zero columns)
  for (size_t r = 0; r < R; ++r)
    HIP_TRY(hipMemcpy2D(L.Asys + r * Fp * Fp, Fp * sizeof(double), A + r * F * F, F * sizeof(double), F * sizeof(double), F, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(L.b, Fp * sizeof(double), b, F * sizeof(double), F * sizeof(double), R, hipMemcpyHostToDevice));
  HIP_TRY(launch_lspi_solve(L, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy2D(x, F * sizeof(double), L.w, 2 * Fp * sizeof(double), F * sizeof(double), R, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_lspi_info(grlx_lspi_ctx *ctx, int replica, int64_t *n_transitions, int64_t *batches_done, uint32_t *status, int64_t *ties, uint64_t rng[2])
{
  if (int rc = lspi_replica_ok(ctx, "grlx_lspi_info", replica)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  LspiRep r;
  HIP_TRY(hipMemcpy(&r, ctx->L.rep + replica, sizeof(r), hipMemcpyDeviceToHost));
  if (n_transitions) *n_transitions = r.n;
  if (batches_done) *batches_done = r.batches_done;
  if (status) *status = r.status;
  if (ties) *ties = r.ties;
  if (rng) { rng[0] = r.G; rng[1] = r.TL; }
  return GRLX_OK;
}

// Q(s, a_k) of each replica's CURRENT weights at observations of the caller's choice: q[replica][n_obs][A].  Reads L.w only.
int grlx_lspi_query(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, const double *obs, int n_obs, double *q)
{
  const char *who = "grlx_lspi_query";
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  if (!q) return fail(GRLX_ERR_INVALID, "%s: q is null", who);
  if (!obs) return fail(GRLX_ERR_INVALID, "%s: obs is null", who);
  if (n_obs < 0) return fail(GRLX_ERR_INVALID, "%s: n_obs = %d", who, n_obs);
  if (int rc = replica_range_ok(who, ctx->L.R, first_replica, n_replicas)) return rc;
  for (int o = 0; o < n_obs; ++o)
    for (int d = 0; d < kLspiD; ++d)
      if (!std::isfinite(obs[(size_t)o * kLspiD + d])) return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d is not finite", who, o, d);
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const size_t elem = sizeof(double) * (size_t)ctx->L.A;
  const int chunk = query_chunk(n_obs, sizeof(double) * kLspiD + elem * (size_t)n_replicas);
  const ReadOut outs[1] = {{q, elem, n_replicas, true}};
  return chunked_read(kPlainRead, outs, 1, n_obs, obs, kLspiD, chunk, false, [&](int nc, const double *dobs, const DevPtr *d) -> int {
    HIP_TRY(launch_lspi_query(ctx->L, first_replica, n_replicas, dobs, nc, d[0].as<double>(), nullptr));
    return GRLX_OK;
  });
}

// grlx_query_ensemble's columns over groups of group_size consecutive replicas: out[group][n_obs][2 + 2 A]
int grlx_lspi_query_ensemble(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, int group_size, const double *obs, int n_obs, double *out)
{
  const char *who = "grlx_lspi_query_ensemble";
  if (!ctx) return fail(GRLX_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return fail(GRLX_ERR_INVALID, "%s: out is null", who);
  if (int rc = lspi_query_admit(ctx, who, first_replica, n_replicas, obs, n_obs)) return rc;
  if (int rc = batch_ensemble_admit(who, n_replicas, group_size)) return rc;
  if (n_obs == 0 || n_replicas == 0) return GRLX_OK;
  HIP_TRY(hipDeviceSynchronize());
  const int groups = n_replicas / group_size;
  const size_t elem = sizeof(double) * (2 + 2 * (size_t)ctx->L.A);
  const int chunk = query_chunk(n_obs, sizeof(double) * kLspiD + elem * (size_t)groups);
  const ReadOut outs[1] = {{out, elem, groups, true}};
  return chunked_read(kPlainRead, outs, 1, n_obs, obs, kLspiD, chunk, false, [&](int nc, const double *dobs, const DevPtr *d) -> int {
    HIP_TRY(launch_lspi_query_ensemble(ctx->L, first_replica, groups, group_size, dobs, nc, d[0].as<double>(), nullptr));
    return GRLX_OK;
  });
}

int grlx_lspi_evaluate(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret, double *disc,
                       int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state)
{
  return lspi_evaluate_impl(ctx, "grlx_lspi_evaluate", nullptr, first_replica, n_replicas, states, n_starts, max_steps, ret, disc, steps, terminal, ties,
                            final_state, nullptr);
}

int grlx_lspi_trajectory_record_words(grlx_lspi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_trajectory_record_words: ctx is null");
  return kLspiTrajWords;
}

int grlx_lspi_evaluate_trajectory(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret,
                                  double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  return lspi_evaluate_impl(ctx, "grlx_lspi_evaluate_trajectory", "grlx_lspi_evaluate", first_replica, n_replicas, states, n_starts, max_steps, ret, disc,
                            steps, terminal, ties, final_state, records);
}

int grlx_lspi_evaluate_ensemble(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                                int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                                int64_t *agreement, double *final_state)
{
  return lspi_evaluate_ensemble_impl(ctx, "grlx_lspi_evaluate_ensemble", nullptr, first_replica, n_replicas, group_size, rule, states, n_starts, max_steps,
                                     ret, disc, steps, terminal, ties, member_ties, agreement, final_state, nullptr);
}

int grlx_lspi_ensemble_trajectory_record_words(grlx_lspi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_ensemble_trajectory_record_words: ctx is null");
  return kLspiEnsTrajWords;
}

int grlx_lspi_evaluate_ensemble_trajectory(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states,
                                           int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                           int64_t *member_ties, int64_t *agreement, double *final_state, double *records)
{
  return lspi_evaluate_ensemble_impl(ctx, "grlx_lspi_evaluate_ensemble_trajectory", "grlx_lspi_evaluate_ensemble", first_replica, n_replicas, group_size,
                                     rule, states, n_starts, max_steps, ret, disc, steps, terminal, ties, member_ties, agreement, final_state, records);
}

int grlx_lspi_evaluate_sampled(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler,
                               double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                               int32_t *explored, double *final_state, uint64_t *streams_out)
{
  return lspi_evaluate_sampled_impl(ctx, "grlx_lspi_evaluate_sampled", nullptr, first_replica, n_replicas, states, n_starts, max_steps, sampler, epsilon, streams,
                                    ret, disc, steps, terminal, ties, explored, final_state, streams_out, nullptr);
}

int grlx_lspi_sampled_trajectory_record_words(grlx_lspi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_sampled_trajectory_record_words: ctx is null");
  return kLspiSampledTrajWords;
}

int grlx_lspi_evaluate_sampled_trajectory(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler,
                                          double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                                          int32_t *ties, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  return lspi_evaluate_sampled_impl(ctx, "grlx_lspi_evaluate_sampled_trajectory", "grlx_lspi_evaluate_sampled", first_replica, n_replicas, states, n_starts,
                                    max_steps, sampler, epsilon, streams, ret, disc, steps, terminal, ties, explored, final_state, streams_out, records);
}

int grlx_lspi_evaluate_ensemble_sampled(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, int group_size, int strategy, double tau, int member,
                                        double member_param, const double *states, int n_starts, int max_steps, const uint64_t *streams, double *ret,
                                        double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties, int64_t *agreement,
                                        int32_t *explored, double *final_state, uint64_t *streams_out)
{
  return lspi_evaluate_ensemble_sampled_impl(ctx, "grlx_lspi_evaluate_ensemble_sampled", nullptr, first_replica, n_replicas, group_size, strategy, tau, member,
                                             member_param, states, n_starts, max_steps, streams, ret, disc, steps, terminal, ties, member_ties, agreement,
                                             explored, final_state, streams_out, nullptr);
}

int grlx_lspi_ensemble_sampled_trajectory_record_words(grlx_lspi_ctx *ctx)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "grlx_lspi_ensemble_sampled_trajectory_record_words: ctx is null");
  return kLspiEnsSampledTrajWords;
}

int grlx_lspi_evaluate_ensemble_sampled_trajectory(grlx_lspi_ctx *ctx, int first_replica, int n_replicas, int group_size, int strategy, double tau, int member,
                                                   double member_param, const double *states, int n_starts, int max_steps, const uint64_t *streams,
                                                   double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                                                   int64_t *agreement, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  return lspi_evaluate_ensemble_sampled_impl(ctx, "grlx_lspi_evaluate_ensemble_sampled_trajectory", "grlx_lspi_evaluate_ensemble_sampled", first_replica,
                                             n_replicas, group_size, strategy, tau, member, member_param, states, n_starts, max_steps, streams, ret, disc,
                                             steps, terminal, ties, member_ties, agreement, explored, final_state, streams_out, records);
}

} // extern "C"
