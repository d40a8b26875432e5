// grlx_api_read.cpp -- the C ABI declared in include/grlx.h: the read side -- policy queries, greedy, sampled, noisy and actor-ensemble evaluation episodes, chunked over the caller's observations / start states; the streamed trajectories' two-slot pipeline.
#include "grlx_host.h"
#include "grlx_query.h"
#include "grlx_evaluate.h"
#include "grlx_evaluate_sampled.h"
#include "grlx_evaluate_noisy.h"
#include "grlx_evaluate_actor_ensemble.h"
#include "grlx_evaluate_stream.h"

// ------------------------------------------------------------------------------------------- policy queries ---
namespace {

constexpr uint64_t kQueryChunkDefault = 256ull << 20;
uint64_t g_query_chunk_bytes = kQueryChunkDefault;

bool q_agent(int agent) { return agent != GRLX_AGENT_AC; }      // every other agent acts through a policy/discrete/q on table 0

// the replica range every read names: [first_replica, first_replica + n_replicas) inside the context
int replica_range_ok(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas)
{
  if (first_replica < 0 || n_replicas < 0 || (int64_t)first_replica + n_replicas > ctx->P.n_replicas)
    return fail(GRLX_ERR_INVALID, "%s: replica range [%d, %lld) is outside the context's %d replicas", who, first_replica,
                (long long)first_replica + n_replicas, ctx->P.n_replicas);
  return GRLX_OK;
}

// what every query checks before it touches the device; tp: the projector of the table read, obs_dims: its share of the observation
int query_admit(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *obs, int n_obs, const TileParams &tp, int obs_dims)
{
  if (ctx->P.tile_safe >= 1)
    return fail(GRLX_ERR_INVALID, "%s is not built for projector/tile_coding:safe >= 1 (a read would have to walk the claim table without claiming)", who);
  if (n_obs < 0) return fail(GRLX_ERR_INVALID, "%s: n_obs = %d", who, n_obs);
  if (int rc = replica_range_ok(ctx, who, first_replica, n_replicas)) return rc;
  if (!obs) return fail(GRLX_ERR_INVALID, "%s: obs is null", who);
  int o = 0, i = 0;                                     // quant_admit_rows (grlx_host_rules.h): the rule grlx_project applies too
  if (int why = quant_admit_rows(obs, n_obs, obs_dims, tp.scaling, &o, &i))
  {
    const double x = obs[(size_t)o * obs_dims + i];
    if (why == 1) return fail(GRLX_ERR_INVALID, "%s: observation row %d, dimension %d is not finite (%g)", who, o, i, x);
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

// rows [n_replicas] of `elem` bytes per observation: device [r][chunk] -> host [r][n_obs] at observation o0
hipError_t query_copy_out(void *host, const void *dev, size_t elem, int n_replicas, int n_obs, int o0, int nc)
{
  return hipMemcpy2D((char *)host + (size_t)o0 * elem, (size_t)n_obs * elem, dev, (size_t)nc * elem, (size_t)nc * elem, (size_t)n_replicas,
                     hipMemcpyDeviceToHost);
}

// grlx_read_kernel_timing (include/grlx_diag.h): the device time of the chunks' launches, summed since timing was enabled
bool g_read_timing = false;
double g_read_ms = 0;
int g_read_chunks = 0;

struct ReadTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~ReadTimer()
  {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t start()
  {
    if (hipError_t err = hipEventCreate(&e0)) return err;
    if (hipError_t err = hipEventCreate(&e1)) return err;
    return hipEventRecord(e0, nullptr);
  }
  hipError_t stop()
  {
    if (hipError_t err = hipEventRecord(e1, nullptr)) return err;
    if (hipError_t err = hipEventSynchronize(e1)) return err;
    float ms = 0;
    if (hipError_t err = hipEventElapsedTime(&ms, e0, e1)) return err;
    g_read_ms += ms;
    g_read_chunks++;
    return hipSuccess;
  }
};

// One output of a chunked read: `rows` rows of `elem` bytes per column, copied to `host` when that is not null; `on_device`: the kernels
// write it (or a reduction reads it) whether the caller asked for it or not.
struct ReadOut { void *host; size_t elem; int rows; bool on_device; };
constexpr int kMaxReadOuts = 9;
// A second per-column input of a chunked read, laid out like an output: host [rows][cols] of `elem` bytes -> `dev` [rows][chunk], so that
// a chunk's rows begin at its first column for EVERY row (a strided copy, not a contiguous one).  host null: nothing is staged.
struct ReadIn { const void *host; size_t elem; int rows; DevBuf *dev; };

// The skeleton of every read: the columns of `in` (observations or start states, `in_dims` doubles each) go through the device `chunk` at a
// time.  Per chunk: the input in, launch(nc, input, outputs) -- device pointers, null for an output neither asked for nor needed -- and out
// what the caller asked for.  `sync_each`: every output may be null, so the next chunk's copy-in must not overtake the launch.
// `extra`: a second input staged beside the first (ReadIn), or null.
template <typename Launch>
int chunked_read(grlx_ctx *ctx, const ReadOut *outs, int n_outs, int cols, const double *in, int in_dims, int chunk, bool sync_each, Launch launch,
                 const ReadIn *extra = nullptr)
{
  DevBuf din, dout[kMaxReadOuts];
  HIP_TRY(din.alloc(sizeof(double) * (size_t)chunk * in_dims));
  if (extra && extra->host) HIP_TRY(extra->dev->alloc(extra->elem * (size_t)extra->rows * (size_t)chunk));
  for (int k = 0; k < n_outs; ++k)
    if (outs[k].host || outs[k].on_device) HIP_TRY(dout[k].alloc(outs[k].elem * (size_t)outs[k].rows * (size_t)chunk));
  for (int c0 = 0; c0 < cols; c0 += chunk)
  {
    const int nc = cols - c0 < chunk ? cols - c0 : chunk;
    HIP_TRY(hipMemcpy(din.get(), in + (size_t)c0 * in_dims, sizeof(double) * (size_t)nc * in_dims, hipMemcpyHostToDevice));
    if (extra && extra->host)
      HIP_TRY(hipMemcpy2D(extra->dev->get(), (size_t)nc * extra->elem, (const char *)extra->host + (size_t)c0 * extra->elem, (size_t)cols * extra->elem,
                          (size_t)nc * extra->elem, (size_t)extra->rows, hipMemcpyHostToDevice));
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, nullptr));
    if (g_read_timing)
    { // grlx_read_kernel_timing: events around the chunk's launches, waited for here
      ReadTimer timer;
      HIP_TRY(timer.start());
      if (int rc = launch(nc, din.as<double>(), dout)) return rc;
      HIP_TRY(timer.stop());
    }
    else if (int rc = launch(nc, din.as<double>(), dout)) return rc;
    for (int k = 0; k < n_outs; ++k)
      if (outs[k].host) HIP_TRY(query_copy_out(outs[k].host, dout[k].get(), outs[k].elem, outs[k].rows, cols, c0, nc));
    if (sync_each) HIP_TRY(hipDeviceSynchronize());
  }
  return GRLX_OK;
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
  const bool e = ensemble != nullptr;              // the reduction reads q, value and greedy; the caller of grlx_query_ensemble gets only its result
  const ReadOut outs[5] = {{q, sizeof(double) * NA, n_replicas, e}, {value, sizeof(double), n_replicas, e}, {greedy, sizeof(int32_t), n_replicas, e},
                           {n_max, sizeof(int32_t), n_replicas, false}, {ensemble, sizeof(double) * cols, n_groups, false}};
  return chunked_read(ctx, outs, 5, n_obs, obs, D, chunk, false, [&](int nc, const double *dobs, const DevBuf *d) -> int {
    QueryArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.n_obs = nc;
    A.obs = dobs; A.q = d[0].as<double>(); A.value = d[1].as<double>(); A.greedy = d[2].as<int32_t>(); A.n_max = d[3].as<int32_t>();
    HIP_TRY(launch_query_q(ctx->P, A, nullptr));
    if (ensemble) HIP_TRY(launch_query_reduce(NA, n_groups, group_size, nc, A.q, A.value, A.greedy, d[4].as<double>(), nullptr));
    return GRLX_OK;
  });
}

// ---- policy evaluation: greedy episodes from start states of the caller's choice (grlx_evaluate.hip) -----------------------------------
// what both evaluations check before they touch the device
int evaluate_admit(grlx_ctx *ctx, const char *who, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps)
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
  if (int rc = replica_range_ok(ctx, who, first_replica, n_replicas)) return rc;
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

// what both ensemble evaluations check beyond evaluate_admit
int ensemble_admit(grlx_ctx *ctx, const char *who, int n_replicas, int group_size, int rule)
{
  if (!q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "%s is not built for the actor-critic agent (a vote over continuous actions is mapping/policy/multi's: "
                "grlx_evaluate_actor_ensemble combines them); it serves agents with a policy/discrete/q", who);
  if (group_size < 1) return fail(GRLX_ERR_INVALID, "%s: group_size = %d is below 1", who, group_size);
  if (n_replicas % group_size != 0) return fail(GRLX_ERR_INVALID, "%s: group_size %d does not divide the %d replicas", who, group_size, n_replicas);
  if (rule != GRLX_ENSEMBLE_VOTE && rule != GRLX_ENSEMBLE_MEAN_Q)
    return fail(GRLX_ERR_INVALID, "%s: unknown rule %d (GRLX_ENSEMBLE_VOTE = 0, GRLX_ENSEMBLE_MEAN_Q = 1)", who, rule);
  return GRLX_OK;
}

// ---- per-step trajectories: the two evaluations with a record per step (grlx_evaluate.hip: trajectory_*_kernel) -----------------------------
// What a trajectory call checks beyond its sibling, after the sibling's own checks; gives the start states per chunk.  `rows`: replicas or
// groups; `in_and_sums`: a start state's other staged bytes (its state and its rows' sums).  Unlike the other reads a chunk never exceeds
// the bound: the records are what the bound is for, so a column that does not fit is refused instead of staged as "at least one".
int trajectory_admit(const char *who, const char *sibling, const void *records, int max_steps, int rows, int n_starts,
                            int R, size_t in_and_sums, int *chunk)
{
  if (!records) return fail(GRLX_ERR_INVALID, "%s: records is null (for the sums alone call %s)", who, sibling);
  if (max_steps == 0)
    return fail(GRLX_ERR_INVALID, "%s: max_steps = 0: the records are sized by max_steps, so there is no default here (1 ... GRLX_MAX_EPISODE_STEPS = %d)", who,
                GRLX_MAX_EPISODE_STEPS);
  const uint64_t column = (uint64_t)rows * (uint64_t)max_steps * (uint64_t)R * sizeof(double);
  if (column + in_and_sums > g_query_chunk_bytes)
    return fail(GRLX_ERR_INVALID, "%s: one start state's column of records is %llu bytes (%d rows x %d steps x %d words x 8; %llu with its sums) and exceeds "
                "the staging bound of %llu bytes: ask for fewer replicas per call, a smaller max_steps, or raise the bound with grlx_set_query_chunk_bytes", who,
                (unsigned long long)column, rows, max_steps, R, (unsigned long long)(column + in_and_sums), (unsigned long long)g_query_chunk_bytes);
  *chunk = rows ? query_chunk(n_starts, (size_t)column + in_and_sums) : n_starts;
  return GRLX_OK;
}

// ---- sampled evaluation: the episodes of grlx_evaluate acted by the reference's samplers on streams the episodes carry (grlx_evaluate_sampled.hip)
// what both sampled evaluations check beyond evaluate_admit
int sampled_admit(grlx_ctx *ctx, const char *who, int n_replicas, int n_starts, int sampler, double epsilon, const uint64_t *streams)
{
  if (!q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "%s is not built for the actor-critic agent (its Gaussian / Ornstein-Uhlenbeck exploration needs the policy's noise state: "
                "grlx_evaluate_noisy carries it); it serves agents with a policy/discrete/q", who);
  if (sampler != GRLX_SAMPLER_GREEDY && sampler != GRLX_SAMPLER_EPSILON_GREEDY)
    return fail(GRLX_ERR_INVALID, "%s: unknown sampler %d (GRLX_SAMPLER_GREEDY = 0, GRLX_SAMPLER_EPSILON_GREEDY = 1)", who, sampler);
  if (!std::isfinite(epsilon)) return fail(GRLX_ERR_INVALID, "%s: epsilon is not finite (%g)", who, epsilon);
  if (epsilon != GRLX_EPSILON_OWN && !(epsilon >= 0. && epsilon <= 1.))
    return fail(GRLX_ERR_INVALID, "%s: epsilon = %g is outside [0, 1] and is not GRLX_EPSILON_OWN (-1)", who, epsilon);
  if (streams)
    for (int64_t row = 0; row < (int64_t)n_replicas * n_starts; ++row)
      for (int w = 0; w < 2; ++w)
        if (streams[row * 2 + w] >> 48)
          return fail(GRLX_ERR_INVALID, "%s: stream row %lld (replica %lld, start state %lld), word %d is 0x%llx: a rand48 state is below 2^48", who,
                      (long long)row, (long long)(row / n_starts), (long long)(row % n_starts), w, (unsigned long long)streams[row * 2 + w]);
  return GRLX_OK;
}

// ---- noisy evaluation: the actor-critic's episodes under its exploration, on a stream and a noise state the episodes carry (grlx_evaluate_noisy.hip)
// what both noisy evaluations check beyond evaluate_admit
int noisy_admit(grlx_ctx *ctx, const char *who, int n_replicas, int n_starts, double sigma, double theta, const uint64_t *streams, const double *noise)
{
  if (q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "%s serves the actor-critic only (Gaussian / Ornstein-Uhlenbeck noise on a continuous action); the samplers of an agent with a "
                "policy/discrete/q are grlx_evaluate_sampled's", who);
  if (!std::isfinite(sigma)) return fail(GRLX_ERR_INVALID, "%s: sigma is not finite (%g)", who, sigma);
  if (sigma != GRLX_SIGMA_OWN && !(sigma >= 0.)) return fail(GRLX_ERR_INVALID, "%s: sigma = %g is negative and is not GRLX_SIGMA_OWN (-1)", who, sigma);
  if (!std::isfinite(theta)) return fail(GRLX_ERR_INVALID, "%s: theta is not finite (%g)", who, theta);
  if (theta != GRLX_THETA_OWN && !(theta >= 0. && theta <= 1.))
    return fail(GRLX_ERR_INVALID, "%s: theta = %g is outside [0, 1] and is not GRLX_THETA_OWN (-1)", who, theta);
  for (int64_t row = 0; row < (int64_t)n_replicas * n_starts; ++row)
  {
    if (streams && streams[row] >> 48)
      return fail(GRLX_ERR_INVALID, "%s: stream row %lld (replica %lld, start state %lld) is 0x%llx: a rand48 state is below 2^48", who, (long long)row,
                  (long long)(row / n_starts), (long long)(row % n_starts), (unsigned long long)streams[row]);
    if (noise && !std::isfinite(noise[row]))
      return fail(GRLX_ERR_INVALID, "%s: noise row %lld (replica %lld, start state %lld) is not finite (%g)", who, (long long)row, (long long)(row / n_starts),
                  (long long)(row % n_starts), noise[row]);
  }
  return GRLX_OK;
}

// ---- actor-critic ensembles: episodes on the members' combined action (grlx_evaluate_actor_ensemble.hip) -------------------------------------
// what both calls check beyond evaluate_admit
int actor_ensemble_admit(grlx_ctx *ctx, const char *who, int n_replicas, int group_size, int rule, int bins, double r)
{
  if (q_agent(ctx->cfg.agent))
    return fail(GRLX_ERR_INVALID, "%s serves the actor-critic only (it combines continuous actions, mapping/policy/multi); the vote and the mean Q of agents "
                "with a policy/discrete/q are grlx_evaluate_ensemble's", who);
  if (group_size < 1) return fail(GRLX_ERR_INVALID, "%s: group_size = %d is below 1", who, group_size);
  if (n_replicas % group_size != 0) return fail(GRLX_ERR_INVALID, "%s: group_size %d does not divide the %d replicas", who, group_size, n_replicas);
  if (group_size > GRLX_ACTOR_ENSEMBLE_MAX)
    return fail(GRLX_ERR_INVALID, "%s: group_size = %d exceeds GRLX_ACTOR_ENSEMBLE_MAX (%d)", who, group_size, GRLX_ACTOR_ENSEMBLE_MAX);
  switch (rule)
  {
    case GRLX_ACTOR_ENSEMBLE_MEAN: break;
    case GRLX_ACTOR_ENSEMBLE_BINNING:
      if (bins < 1 || bins > 64) return fail(GRLX_ERR_INVALID, "%s: bins = %d is outside 1 ... 64 (GRLX_ACTOR_ENSEMBLE_BINNING)", who, bins);
      break;
    case GRLX_ACTOR_ENSEMBLE_DATA_CENTER:
      if (bins < 1) return fail(GRLX_ERR_INVALID, "%s: bins = %d, the members kept, is below 1 (GRLX_ACTOR_ENSEMBLE_DATA_CENTER)", who, bins);
      break;
    case GRLX_ACTOR_ENSEMBLE_DENSITY:
      if (!std::isfinite(r)) return fail(GRLX_ERR_INVALID, "%s: r is not finite (%g) (GRLX_ACTOR_ENSEMBLE_DENSITY)", who, r);
      if (!(r > 0.)) return fail(GRLX_ERR_INVALID, "%s: r = %g is not above 0 (GRLX_ACTOR_ENSEMBLE_DENSITY)", who, r);
      break;
    default:
      return fail(GRLX_ERR_INVALID, "%s: unknown rule %d (GRLX_ACTOR_ENSEMBLE_MEAN = 0, _BINNING = 1, _DATA_CENTER = 2, _DENSITY = 3)", who, rule);
  }
  return GRLX_OK;
}

// ---- one description of an episode call: what the evaluation entry points share around their launch -----------------------------------------
// Every variant has the six base outputs -- ret, disc, steps, terminal, ties (the noisy variant: clipped) and final_state -- for `rows`
// replicas or groups, up to two outputs of its own, and, as a trajectory, the records.  An entry point fills this in and keeps its admit
// and its launch.
struct EpisodeCall {
  const char   *who;
  int           first_replica, n_replicas;
  int           group_size;                 // 0: an episode per replica; else per group of this many (one block per pair: the grid's bound)
  const double *states;
  int           n_starts, max_steps;
  double       *ret, *disc;
  int32_t      *steps, *terminal, *ties;
  double       *final_state;
  ReadOut       extra[2];                   // the variant's own outputs: host and elem; the rows are filled in here
  int           n_extra;
  size_t        extra_bytes;                // per pair, what the variant stages beyond the six outputs: part of what cuts the chunks
  const ReadIn *in;                         // the variant's second input, or null
  // trajectory calls only: the call that gives the sums alone (named in a refusal), the caller's records, R of an environment's record
  const char   *sibling;
  double       *records;
  int         (*record_words)(int env);
};
constexpr int kBaseOuts = 6;

// the ReadOut rows of a call: the six, the variant's own, the records (rec_elem bytes per pair; 0: none)
int episode_outs(const EpisodeCall &c, int rows, int S, size_t rec_elem, ReadOut *outs)
{
  const ReadOut base[kBaseOuts] = {{c.ret, sizeof(double), rows, true}, {c.disc, sizeof(double), rows, true}, {c.steps, sizeof(int32_t), rows, true},
                                   {c.terminal, sizeof(int32_t), rows, true}, {c.ties, sizeof(int32_t), rows, true},
                                   {c.final_state, sizeof(double) * (size_t)S, rows, true}};
  int n = 0;
  for (const ReadOut &o : base) outs[n++] = o;
  for (int k = 0; k < c.n_extra; ++k) outs[n++] = {c.extra[k].host, c.extra[k].elem, rows, true};
  if (rec_elem) outs[n++] = {c.records, rec_elem, rows, true};
  return n;
}

// the base fields of a chunk's argument block (EvaluateArgs, EnsembleArgs: the same member names) for nc start states at dst
template <class Args>
void episode_args(Args &A, grlx_ctx *ctx, const EpisodeCall &c, int max_steps, int nc, const double *dst, const DevBuf *d)
{
  A.first_replica = c.first_replica; A.n_replicas = c.n_replicas; A.n_starts = nc; A.max_steps = max_steps;
  A.states = dst; A.sweep = ctx->sweep ? ctx->sweep_dev.get() : nullptr;
  A.ret = d[0].as<double>(); A.disc = d[1].as<double>(); A.steps = d[2].as<int32_t>(); A.terminal = d[3].as<int32_t>(); A.ties = d[4].as<int32_t>();
  A.final_state = d[5].as<double>();
}

// The path of every evaluation call.  admit(): the variant's checks, after evaluate_admit's.  launch(A, extra, records): the variant's
// kernels on a chunk -- A with its base fields filled, the device arrays of c.extra, the chunk's zero-filled records (null: no trajectory).
template <class Args, class Admit, class Launch>
int episode_read(grlx_ctx *ctx, const EpisodeCall &c, Admit admit, Launch launch)
{
  int max_steps = c.max_steps;
  if (int rc = evaluate_admit(ctx, c.who, c.first_replica, c.n_replicas, c.states, c.n_starts, max_steps)) return rc;
  if (int rc = admit()) return rc;
  const int S = ctx->S, rows = c.group_size ? c.n_replicas / c.group_size : c.n_replicas, R = c.sibling ? c.record_words(ctx->cfg.env) : 0;
  const size_t per_pair = 2 * sizeof(double) + 3 * sizeof(int32_t) + sizeof(double) * (size_t)S + c.extra_bytes;
  const size_t in_and_sums = sizeof(double) * (size_t)S + per_pair * (size_t)rows;
  int chunk = 0;
  if (c.sibling)
  {
    if (int rc = trajectory_admit(c.who, c.sibling, c.records, max_steps, rows, c.n_starts, R, in_and_sums, &chunk)) return rc;
  }
  else chunk = query_chunk(c.n_starts, in_and_sums);
  if (max_steps == 0) max_steps = GRLX_MAX_EPISODE_STEPS;
  if (c.n_starts == 0 || c.n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  if (c.group_size && (int64_t)chunk * rows > 0x7fffffff) chunk = 0x7fffffff / rows;
  const size_t rec_elem = sizeof(double) * (size_t)R * (size_t)max_steps;
  ReadOut outs[kMaxReadOuts];
  const int n_outs = episode_outs(c, rows, S, rec_elem, outs);
  return chunked_read(ctx, outs, n_outs, c.n_starts, c.states, S, chunk, true, [&](int nc, const double *dst, const DevBuf *d) -> int {
    Args A{};
    episode_args(A, ctx, c, max_steps, nc, dst, d);
    double *records = rec_elem ? d[n_outs - 1].as<double>() : nullptr;
    if (records) HIP_TRY(hipMemsetAsync(records, 0, rec_elem * (size_t)rows * (size_t)nc, nullptr));     // records behind an episode's end are +0.0
    HIP_TRY(launch(A, d + kBaseOuts, records));
    return GRLX_OK;
  }, c.in);
}

// what the *_record_words calls check; wrong_agent(ctx): the variant does not serve the context's agent, `why` says so
int record_words_admit(grlx_ctx *ctx, const char *who, bool (*wrong_agent)(grlx_ctx *), const char *why)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "bad argument");
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL || !evaluate_built(ctx->cfg.agent, ctx->cfg.env, ctx->P.A))
    return fail(GRLX_ERR_INVALID, "%s: no evaluation episodes are built for this context (environment %d)", who, ctx->cfg.env);
  if (wrong_agent && wrong_agent(ctx)) return fail(GRLX_ERR_INVALID, "%s: %s", who, why);
  return GRLX_OK;
}
bool is_ac(grlx_ctx *ctx) { return !q_agent(ctx->cfg.agent); }
bool is_q(grlx_ctx *ctx) { return q_agent(ctx->cfg.agent); }
int greedy_words(int env) { return trajectory_words(env, false); }
int ensemble_words(int env) { return trajectory_words(env, true); }

// ---- streamed trajectories: grlx_evaluate_trajectory's chunks handed to a sink while the next one runs (grlx_evaluate_stream.hip) ----------
// The outputs of a chunk of nc start states, on the device and in pinned memory alike: the records, ret, disc, final_state, steps, terminal,
// ties, one behind the other -- every array [rows][nc]..., the 8-byte ones first -- so that ONE contiguous copy brings a chunk back.
// bytes = nc * stream_out_bytes (grlx_host_rules.h).
struct StreamLayout {
  size_t records, ret, disc, final_state, steps, terminal, ties, bytes;
  StreamLayout(size_t rows, size_t nc, size_t max_steps, size_t R, size_t S)
  {
    const size_t pairs = rows * nc;
    records = 0;
    ret = records + pairs * max_steps * R * sizeof(double);
    disc = ret + pairs * sizeof(double);
    final_state = disc + pairs * sizeof(double);
    steps = final_state + pairs * S * sizeof(double);
    terminal = steps + pairs * sizeof(int32_t);
    ties = terminal + pairs * sizeof(int32_t);
    bytes = ties + pairs * sizeof(int32_t);
  }
};

// the context's slots with room for a chunk -- both, or the first alone for a call of one chunk: made at the first call that needs them,
// grown when a call needs more (idle then: every call leaves them so)
int stream_slots_ready(grlx_ctx *ctx, const char *who, int n_slots, size_t dev_bytes, size_t pinned_bytes)
{
  for (int k = 0; k < n_slots; ++k)
  {
    StreamSlot &s = ctx->stream_slot[k];
    if (!s.stream)
    {
      HIP_TRY(s.stream.create(hipStreamNonBlocking));
      HIP_TRY(s.done.create(hipEventDisableTiming));
      HIP_TRY(s.k0.create(hipEventDefault));
      HIP_TRY(s.k1.create(hipEventDefault));
    }
    if (s.dev_bytes < dev_bytes)
    {
      s.dev_bytes = 0;
      if (s.dev.alloc(dev_bytes) != hipSuccess)
      {
        (void)hipGetLastError();
        return fail(GRLX_ERR_OOM, "%s: no device memory for a staging slot of %zu bytes (lower the bound with grlx_set_query_chunk_bytes)", who, dev_bytes);
      }
      s.dev_bytes = dev_bytes;
    }
    if (s.pinned_bytes < pinned_bytes)
    {
      s.pinned_bytes = 0;
      if (s.pinned.alloc(pinned_bytes) != hipSuccess)
      {
        (void)hipGetLastError();
        return fail(GRLX_ERR_OOM, "%s: no page-locked host memory for a staging slot of %zu bytes (lower the bound with grlx_set_query_chunk_bytes)", who, pinned_bytes);
      }
      s.pinned_bytes = pinned_bytes;
    }
  }
  return GRLX_OK;
}

// The pipeline.  Chunk k runs on slot k & 1, on the slot's stream: its start states in, (the poison kernel,) its kernel, ONE copy of its
// outputs to the slot's pinned memory, the slot's event.  Then the host waits for chunk k - 1's event and hands that chunk to the sink:
// the kernel of chunk k overlaps the copy of chunk k - 1, and the sink overlaps both.
// Ordering.  Device side: chunk k + 2 is enqueued on the stream chunk k ran on, so its kernel writes the slot's device arrays after chunk
// k's copy has read them.  Pinned side: chunk k + 2 is enqueued in the iteration after the one that retired chunk k, so its copy writes
// the pinned arrays after the sink has returned from reading them.  The two streams share nothing but the tables, which both only read.
// A HIP error or a sink's nonzero return ends the enqueueing; both streams are waited for before the call returns, whatever happened.
int stream_pipeline(grlx_ctx *ctx, const char *who, int first_replica, int rows, const double *states, int n_starts, int max_steps, int R, int chunk,
                    grlx_trajectory_sink sink, void *user)
{
  const size_t S = (size_t)ctx->S, states_cap = sizeof(double) * S * (size_t)chunk;
  const int n_chunks = (int)(((int64_t)n_starts + chunk - 1) / chunk);
  const size_t out_cap = StreamLayout((size_t)rows, (size_t)chunk, (size_t)max_steps, (size_t)R, S).bytes;
  if (int rc = stream_slots_ready(ctx, who, n_chunks > 1 ? 2 : 1, states_cap + out_cap, out_cap)) return rc;
  const bool timing = g_read_timing;
  struct Flag { bool &b; Flag(bool &f) : b(f) { b = true; } ~Flag() { b = false; } } in_progress(ctx->streaming);
  auto first_of = [&](int k) { return (int)((int64_t)k * chunk); };
  auto count_of = [&](int k) { return n_starts - first_of(k) < chunk ? n_starts - first_of(k) : chunk; };

  auto enqueue = [&](int k) -> int {
    StreamSlot &s = ctx->stream_slot[k & 1];
    hipStream_t q = s.stream.get();
    const int c0 = first_of(k), nc = count_of(k);
    const StreamLayout L((size_t)rows, (size_t)nc, (size_t)max_steps, (size_t)R, S);
    char *out = s.dev.as<char>() + states_cap;
    HIP_TRY(hipMemcpyAsync(s.dev.get(), states + (size_t)c0 * S, sizeof(double) * (size_t)nc * S, hipMemcpyHostToDevice, q));
    if (ctx->poison) HIP_TRY(launch_poison_registers(ctx->poison_pattern, q));
    TrajectoryArgs T{};
    T.e.first_replica = first_replica; T.e.n_replicas = rows; T.e.n_starts = nc; T.e.max_steps = max_steps;
    T.e.states = s.dev.as<double>(); T.e.sweep = ctx->sweep ? ctx->sweep_dev.get() : nullptr;
    T.records = (double *)(out + L.records);
    T.e.ret = (double *)(out + L.ret); T.e.disc = (double *)(out + L.disc); T.e.final_state = (double *)(out + L.final_state);
    T.e.steps = (int32_t *)(out + L.steps); T.e.terminal = (int32_t *)(out + L.terminal); T.e.ties = (int32_t *)(out + L.ties);
    if (timing) HIP_TRY(hipEventRecord(s.k0.get(), q));       // grlx_read_kernel_timing: around the chunk's kernel, read when it is retired
    HIP_TRY(launch_trajectory_stream(ctx->P, T, q));
    if (timing) HIP_TRY(hipEventRecord(s.k1.get(), q));
    HIP_TRY(hipMemcpyAsync(s.pinned.get(), out, L.bytes, hipMemcpyDeviceToHost, q));
    HIP_TRY(hipEventRecord(s.done.get(), q));
    return GRLX_OK;
  };
  auto retire = [&](int k) -> int {
    StreamSlot &s = ctx->stream_slot[k & 1];
    const int c0 = first_of(k), nc = count_of(k);
    const StreamLayout L((size_t)rows, (size_t)nc, (size_t)max_steps, (size_t)R, S);
    HIP_TRY(hipEventSynchronize(s.done.get()));
    if (timing)
    {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, s.k0.get(), s.k1.get()));
      g_read_ms += ms;
      g_read_chunks++;
    }
    const char *in = s.pinned.get();
    grlx_trajectory_chunk c;
    c.struct_size = (int32_t)sizeof(c);
    c.first_start = c0; c.n_starts = nc; c.rows = rows; c.max_steps = max_steps; c.record_words = R; c.state_dims = (int32_t)S;
    c.ret = (const double *)(in + L.ret); c.disc = (const double *)(in + L.disc);
    c.steps = (const int32_t *)(in + L.steps); c.terminal = (const int32_t *)(in + L.terminal); c.ties = (const int32_t *)(in + L.ties);
    c.final_state = (const double *)(in + L.final_state); c.records = (const double *)(in + L.records);
    if (const int v = sink(user, &c))
      return fail(GRLX_ERR_STOPPED, "%s: the sink returned %d at chunk %d (start states %d ... %d): nothing further is delivered", who, v, k, c0, c0 + nc - 1);
    return GRLX_OK;
  };

  int rc = GRLX_OK;
  for (int k = 0; k <= n_chunks && rc == GRLX_OK; ++k)
  {
    if (k < n_chunks) rc = enqueue(k);
    if (rc == GRLX_OK && k > 0) rc = retire(k - 1);
  }
  for (StreamSlot &s : ctx->stream_slot)
  {
    if (!s.stream) continue;                           // a context that has only ever streamed single chunks has one slot
    const hipError_t e = hipStreamSynchronize(s.stream.get());
    if (e != hipSuccess && rc == GRLX_OK) rc = fail(GRLX_ERR_HIP, "%s: hipStreamSynchronize failed: %s", who, hipGetErrorString(e));
  }
  return rc;
}

} // namespace
extern "C" {

int grlx_set_query_chunk_bytes(uint64_t bytes)
{
  g_query_chunk_bytes = bytes ? bytes : kQueryChunkDefault;
  set_fqi_query_chunk_bytes(bytes);
  return GRLX_OK;
}

int grlx_read_kernel_timing(int enable, double *ms, int *chunks)
{
  if (ms) *ms = g_read_ms;
  if (chunks) *chunks = g_read_chunks;
  g_read_timing = enable != 0;
  if (enable) { g_read_ms = 0; g_read_chunks = 0; }
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
  const ReadOut outs[1] = {{out, sizeof(double), n_replicas, true}};
  return chunked_read(ctx, outs, 1, n_obs, obs, D, chunk, false, [&](int nc, const double *dobs, const DevBuf *d) -> int {
    QueryArgs A;
    A.first_replica = first_replica; A.n_replicas = n_replicas; A.n_obs = nc;
    A.obs = dobs; A.q = nullptr; A.value = d[0].as<double>(); A.greedy = nullptr; A.n_max = nullptr;
    HIP_TRY(launch_query_state(ctx->P, table, A, nullptr));
    return GRLX_OK;
  });
}

// ---- policy evaluation: greedy episodes, per replica or per group of replicas on their vote or mean Q, with or without a record per step ---
// (grlx_evaluate.hip); records null: the sums alone
static int evaluate_impl(grlx_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                         int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  EpisodeCall c{who, first_replica, n_replicas, 0, states, n_starts, max_steps, ret, disc, steps, terminal, ties, final_state};
  c.sibling = sibling; c.records = records; c.record_words = greedy_words;
  return episode_read<EvaluateArgs>(ctx, c, [] { return GRLX_OK; }, [&](EvaluateArgs &A, const DevBuf *, double *rec) {
    return rec ? launch_trajectory(ctx->P, TrajectoryArgs{A, rec}, nullptr) : launch_evaluate(ctx->P, A, nullptr);
  });
}

static int evaluate_ensemble_impl(grlx_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size, int rule,
                                  const double *states, int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                                  int32_t *ties, int64_t *member_ties, int64_t *agreement, double *final_state, double *records)
{
  EpisodeCall c{who, first_replica, n_replicas, group_size, states, n_starts, max_steps, ret, disc, steps, terminal, ties, final_state};
  c.extra[0] = {member_ties, sizeof(int64_t)}; c.extra[1] = {agreement, sizeof(int64_t)}; c.n_extra = 2;
  c.extra_bytes = 2 * sizeof(int64_t);
  c.sibling = sibling; c.records = records; c.record_words = ensemble_words;
  return episode_read<EnsembleArgs>(ctx, c, [&] { return ensemble_admit(ctx, who, n_replicas, group_size, rule); },
                                    [&](EnsembleArgs &A, const DevBuf *extra, double *rec) {
    A.group_size = group_size; A.rule = rule;
    A.member_ties = extra[0].as<int64_t>(); A.agreement = extra[1].as<int64_t>();
    return rec ? launch_trajectory_ensemble(ctx->P, EnsembleTrajectoryArgs{A, rec}, nullptr) : launch_evaluate_ensemble(ctx->P, A, nullptr);
  });
}

int grlx_evaluate(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret, double *disc,
                  int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state)
{
  return evaluate_impl(ctx, "grlx_evaluate", nullptr, first_replica, n_replicas, states, n_starts, max_steps, ret, disc, steps, terminal, ties, final_state,
                       nullptr);
}

int grlx_evaluate_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                           int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                           int64_t *agreement, double *final_state)
{
  return evaluate_ensemble_impl(ctx, "grlx_evaluate_ensemble", nullptr, first_replica, n_replicas, group_size, rule, states, n_starts, max_steps, ret, disc,
                                steps, terminal, ties, member_ties, agreement, final_state, nullptr);
}

int grlx_trajectory_record_words(grlx_ctx *ctx, int ensemble)
{
  if (int rc = record_words_admit(ctx, "grlx_trajectory_record_words", ensemble ? is_ac : nullptr, "the ensemble evaluation is not built for the actor-critic agent"))
    return rc;
  return trajectory_words(ctx->cfg.env, ensemble != 0);
}

int grlx_evaluate_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double *ret,
                             double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, double *records)
{
  return evaluate_impl(ctx, "grlx_evaluate_trajectory", "grlx_evaluate", first_replica, n_replicas, states, n_starts, max_steps, ret, disc, steps, terminal,
                       ties, final_state, records);
}

// grlx_evaluate_trajectory's result chunk by chunk (stream_pipeline above); every refusal comes before anything is allocated or launched
int grlx_evaluate_trajectory_stream(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps,
                                    grlx_trajectory_sink sink, void *user)
{
  const char *who = "grlx_evaluate_trajectory_stream";
  if (int rc = evaluate_admit(ctx, who, first_replica, n_replicas, states, n_starts, max_steps)) return rc;
  STREAM_REFUSES(ctx, "grlx_evaluate_trajectory_stream");
  if (!sink) return fail(GRLX_ERR_INVALID, "%s: sink is null (for the whole result in one array call grlx_evaluate_trajectory)", who);
  if (max_steps == 0)
    return fail(GRLX_ERR_INVALID, "%s: max_steps = 0: the records are sized by max_steps, so there is no default here (1 ... GRLX_MAX_EPISODE_STEPS = %d)", who,
                GRLX_MAX_EPISODE_STEPS);
  const int S = ctx->S, R = trajectory_words(ctx->cfg.env, false);
  const int chunk = stream_chunk(g_query_chunk_bytes, n_replicas, max_steps, R, S, n_starts);
  if (chunk < 0)
  {
    const uint64_t column = (uint64_t)n_replicas * (uint64_t)max_steps * (uint64_t)R * sizeof(double);
    return fail(GRLX_ERR_INVALID, "%s: one start state's column of records is %llu bytes (%d rows x %d steps x %d words x 8; %llu with its sums) and exceeds "
                "half the staging bound, %llu of %llu bytes (two chunks are staged at a time): ask for fewer replicas per call, a smaller max_steps, or raise the "
                "bound with grlx_set_query_chunk_bytes", who, (unsigned long long)column, n_replicas, max_steps, R,
                (unsigned long long)stream_start_bytes(n_replicas, max_steps, R, S), (unsigned long long)(g_query_chunk_bytes / 2),
                (unsigned long long)g_query_chunk_bytes);
  }
  if (n_starts == 0 || n_replicas == 0) return GRLX_OK;
  DRAIN(ctx);
  return stream_pipeline(ctx, who, first_replica, n_replicas, states, n_starts, max_steps, R, chunk, sink, user);
}

int grlx_evaluate_ensemble_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, const double *states, int n_starts,
                                      int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *member_ties,
                                      int64_t *agreement, double *final_state, double *records)
{
  return evaluate_ensemble_impl(ctx, "grlx_evaluate_ensemble_trajectory", "grlx_evaluate_ensemble", first_replica, n_replicas, group_size, rule, states,
                                n_starts, max_steps, ret, disc, steps, terminal, ties, member_ties, agreement, final_state, records);
}

// ---- sampled evaluation (grlx_evaluate_sampled.hip); sibling null: the sums alone
static int evaluate_sampled_impl(grlx_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                                 int max_steps, int sampler, double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps,
                                 int32_t *terminal, int32_t *ties, int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  DevBuf dstreams;
  const ReadIn in_streams = {streams, 2 * sizeof(uint64_t), n_replicas, &dstreams};     // [replica][start][2]: a chunk is strided, not contiguous
  EpisodeCall c{who, first_replica, n_replicas, 0, states, n_starts, max_steps, ret, disc, steps, terminal, ties, final_state};
  c.extra[0] = {explored, sizeof(int32_t)}; c.extra[1] = {streams_out, 2 * sizeof(uint64_t)}; c.n_extra = 2;
  c.extra_bytes = sizeof(int32_t) + 4 * sizeof(uint64_t);     // explored, both streams in and out
  c.in = &in_streams;
  c.sibling = sibling; c.records = records; c.record_words = sampled_trajectory_words;
  return episode_read<EvaluateArgs>(ctx, c, [&] { return sampled_admit(ctx, who, n_replicas, n_starts, sampler, epsilon, streams); },
                                    [&](EvaluateArgs &A, const DevBuf *extra, double *rec) {
    SampledArgs T;
    T.e = A; T.sampler = sampler; T.epsilon = epsilon;
    T.streams = streams ? dstreams.as<uint64_t>() : nullptr;
    T.explored = extra[0].as<int32_t>(); T.streams_out = extra[1].as<uint64_t>();
    T.records = rec;
    return rec ? launch_trajectory_sampled(ctx->P, T, nullptr) : launch_evaluate_sampled(ctx->P, T, nullptr);
  });
}

int grlx_evaluate_sampled(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler, double epsilon,
                          const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int32_t *explored,
                          double *final_state, uint64_t *streams_out)
{
  return evaluate_sampled_impl(ctx, "grlx_evaluate_sampled", nullptr, first_replica, n_replicas, states, n_starts, max_steps, sampler, epsilon, streams, ret,
                               disc, steps, terminal, ties, explored, final_state, streams_out, nullptr);
}

int grlx_sampled_trajectory_record_words(grlx_ctx *ctx)
{
  if (int rc = record_words_admit(ctx, "grlx_sampled_trajectory_record_words", is_ac, "the sampled evaluation is not built for the actor-critic agent")) return rc;
  return sampled_trajectory_words(ctx->cfg.env);
}

int grlx_evaluate_sampled_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, int sampler,
                                     double epsilon, const uint64_t *streams, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties,
                                     int32_t *explored, double *final_state, uint64_t *streams_out, double *records)
{
  return evaluate_sampled_impl(ctx, "grlx_evaluate_sampled_trajectory", "grlx_evaluate_sampled", first_replica, n_replicas, states, n_starts, max_steps,
                               sampler, epsilon, streams, ret, disc, steps, terminal, ties, explored, final_state, streams_out, records);
}

// ---- noisy evaluation (grlx_evaluate_noisy.hip); sibling null: the sums alone
static int evaluate_noisy_impl(grlx_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, const double *states, int n_starts,
                               int max_steps, double sigma, double theta, const uint64_t *streams, const double *noise, double *ret, double *disc,
                               int32_t *steps, int32_t *terminal, int32_t *clipped, double *final_state, uint64_t *streams_out, double *noise_out,
                               double *records)
{
  // the two 8-byte inputs of a pair travel as one 16-byte column of the staging skeleton: [replica][start]{stream, bits of the noise};
  // an absent array is filled with what the kernel takes as its default (kNoisyOwnStream: the replica's own stream; +0.0)
  std::vector<uint64_t> packed;
  DevBuf dinputs;
  ReadIn in_pairs = {nullptr, 2 * sizeof(uint64_t), n_replicas, &dinputs};
  EpisodeCall c{who, first_replica, n_replicas, 0, states, n_starts, max_steps, ret, disc, steps, terminal, clipped, final_state};
  c.extra[0] = {streams_out, sizeof(uint64_t)}; c.extra[1] = {noise_out, sizeof(double)}; c.n_extra = 2;
  c.extra_bytes = 4 * sizeof(uint64_t);     // stream and noise in and out
  c.in = &in_pairs;
  c.sibling = sibling; c.records = records; c.record_words = noisy_trajectory_words;
  return episode_read<EvaluateArgs>(ctx, c, [&]() -> int {
    if (int rc = noisy_admit(ctx, who, n_replicas, n_starts, sigma, theta, streams, noise)) return rc;
    if (theta == GRLX_THETA_OWN) theta = ctx->P.theta;
    if (streams || noise)
    {
      const size_t rows = (size_t)n_replicas * (size_t)n_starts;
      packed.resize(rows * 2);
      for (size_t row = 0; row < rows; ++row)
      {
        packed[row * 2] = streams ? streams[row] : kNoisyOwnStream;
        uint64_t bits = 0;
        if (noise) memcpy(&bits, &noise[row], sizeof bits);
        packed[row * 2 + 1] = bits;
      }
    }
    in_pairs.host = packed.empty() ? nullptr : packed.data();
    return GRLX_OK;
  }, [&](EvaluateArgs &A, const DevBuf *extra, double *rec) {
    NoisyArgs T;
    T.e = A; T.sigma = sigma; T.theta = theta;
    T.inputs = packed.empty() ? nullptr : dinputs.as<uint64_t>();
    T.streams_out = extra[0].as<uint64_t>(); T.noise_out = extra[1].as<double>();
    T.records = rec;
    return rec ? launch_trajectory_noisy(ctx->P, T, nullptr) : launch_evaluate_noisy(ctx->P, T, nullptr);
  });
}

int grlx_evaluate_noisy(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double sigma, double theta,
                        const uint64_t *streams, const double *noise, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *clipped,
                        double *final_state, uint64_t *streams_out, double *noise_out)
{
  return evaluate_noisy_impl(ctx, "grlx_evaluate_noisy", nullptr, first_replica, n_replicas, states, n_starts, max_steps, sigma, theta, streams, noise, ret,
                             disc, steps, terminal, clipped, final_state, streams_out, noise_out, nullptr);
}

int grlx_noisy_trajectory_record_words(grlx_ctx *ctx)
{
  if (int rc = record_words_admit(ctx, "grlx_noisy_trajectory_record_words", is_q, "the noisy evaluation serves the actor-critic only")) return rc;
  return noisy_trajectory_words(ctx->cfg.env);
}

int grlx_evaluate_noisy_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps, double sigma,
                                   double theta, const uint64_t *streams, const double *noise, double *ret, double *disc, int32_t *steps,
                                   int32_t *terminal, int32_t *clipped, double *final_state, uint64_t *streams_out, double *noise_out, double *records)
{
  return evaluate_noisy_impl(ctx, "grlx_evaluate_noisy_trajectory", "grlx_evaluate_noisy", first_replica, n_replicas, states, n_starts, max_steps, sigma,
                             theta, streams, noise, ret, disc, steps, terminal, clipped, final_state, streams_out, noise_out, records);
}

// ---- actor-critic ensembles (grlx_evaluate_actor_ensemble.hip); sibling null: the sums alone
static int evaluate_actor_ensemble_impl(grlx_ctx *ctx, const char *who, const char *sibling, int first_replica, int n_replicas, int group_size, int rule,
                                        int bins, double r, const double *states, int n_starts, int max_steps, double *ret, double *disc, int32_t *steps,
                                        int32_t *terminal, int32_t *ties, int64_t *kept, double *spread, double *final_state, double *records)
{
  EpisodeCall c{who, first_replica, n_replicas, group_size, states, n_starts, max_steps, ret, disc, steps, terminal, ties, final_state};
  c.extra[0] = {kept, sizeof(int64_t)}; c.extra[1] = {spread, sizeof(double)}; c.n_extra = 2;
  c.extra_bytes = sizeof(int64_t) + sizeof(double);
  c.sibling = sibling; c.records = records; c.record_words = actor_ensemble_trajectory_words;
  return episode_read<ActorEnsembleArgs>(ctx, c, [&] { return actor_ensemble_admit(ctx, who, n_replicas, group_size, rule, bins, r); },
                                         [&](ActorEnsembleArgs &A, const DevBuf *extra, double *rec) {
    A.group_size = group_size; A.rule = rule; A.bins = bins; A.r = r;
    A.kept = extra[0].as<int64_t>(); A.spread = extra[1].as<double>();
    A.records = rec;
    return rec ? launch_trajectory_actor_ensemble(ctx->P, A, nullptr) : launch_evaluate_actor_ensemble(ctx->P, A, nullptr);
  });
}

int grlx_evaluate_actor_ensemble(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, int bins, double r, const double *states,
                                 int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal, int32_t *ties, int64_t *kept,
                                 double *spread, double *final_state)
{
  return evaluate_actor_ensemble_impl(ctx, "grlx_evaluate_actor_ensemble", nullptr, first_replica, n_replicas, group_size, rule, bins, r, states, n_starts,
                                      max_steps, ret, disc, steps, terminal, ties, kept, spread, final_state, nullptr);
}

int grlx_actor_ensemble_trajectory_record_words(grlx_ctx *ctx)
{
  if (int rc = record_words_admit(ctx, "grlx_actor_ensemble_trajectory_record_words", is_q, "the actor ensemble serves the actor-critic only")) return rc;
  return actor_ensemble_trajectory_words(ctx->cfg.env);
}

int grlx_evaluate_actor_ensemble_trajectory(grlx_ctx *ctx, int first_replica, int n_replicas, int group_size, int rule, int bins, double r,
                                            const double *states, int n_starts, int max_steps, double *ret, double *disc, int32_t *steps, int32_t *terminal,
                                            int32_t *ties, int64_t *kept, double *spread, double *final_state, double *records)
{
  return evaluate_actor_ensemble_impl(ctx, "grlx_evaluate_actor_ensemble_trajectory", "grlx_evaluate_actor_ensemble", first_replica, n_replicas, group_size,
                                      rule, bins, r, states, n_starts, max_steps, ret, disc, steps, terminal, ties, kept, spread, final_state, records);
}

// host only: stream k = srand48(seed) advanced by k * 2^20 draws, k = 2 * pair + which
void grlx_episode_streams(long seed, int64_t first_pair, int64_t n_pairs, uint64_t *out)
{
  if (!out || n_pairs <= 0 || first_pair < 0) return;
  constexpr uint64_t kA = 0x5DEECE66DULL, kC = 0xBULL, kMask = (1ULL << 48) - 1;
  uint64_t ja = kA, jc = kC;                            // the affine map of 2^20 draws, by 20 squarings
  for (int i = 0; i < 20; ++i) { jc = ((ja + 1) * jc) & kMask; ja = (ja * ja) & kMask; }
  // ... and of first_pair * 2 such jumps: x -> A^n x + C_n by repeated squaring over the bits of n
  uint64_t x = h_seed(seed), a = ja, c = jc;
  for (uint64_t n = (uint64_t)first_pair * 2; n; n >>= 1)
  {
    if (n & 1) x = (a * x + c) & kMask;
    c = ((a + 1) * c) & kMask;
    a = (a * a) & kMask;
  }
  for (int64_t k = 0; k < 2 * n_pairs; ++k)
  {
    out[k] = x;
    x = (ja * x + jc) & kMask;
  }
}

// host only: the even streams of grlx_episode_streams, one per pair
void grlx_episode_stream_words(long seed, int64_t first_pair, int64_t n_pairs, uint64_t *out)
{
  if (!out || n_pairs <= 0 || first_pair < 0) return;
  std::vector<uint64_t> both((size_t)n_pairs * 2);
  grlx_episode_streams(seed, first_pair, n_pairs, both.data());
  for (int64_t k = 0; k < n_pairs; ++k) out[k] = both[(size_t)k * 2];
}

} // extern "C"
