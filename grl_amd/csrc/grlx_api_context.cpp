// grlx_api_context.cpp -- the C ABI declared in include/grlx.h: context lifetime -- the error message, create / destroy, diagnostics, table growth and the reset between two runs.
#include "grlx_host.h"

namespace grlx {
static thread_local std::string g_err;      // the library's one message per thread

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

void set_last_error(const char *msg) { g_err = msg; }     // other translation units of the library (grlx_fqi.hip)

bool have_device() { return grlx_device_count() > 0; }

// Read-back and fine-grained entry points run on the NULL stream or copy synchronously: wait for the rollouts
// of the last grlx_run first (its stream may be non-blocking with respect to the NULL stream).
int drain(grlx_ctx *ctx)
{
  // from inside the sink of grlx_evaluate_trajectory_stream: the chunks in flight read the tables, and a copy on the null stream would
  // wait for them one way or the other -- no call on this context is served until the streamed call has returned
  if (ctx->streaming)
    return fail(GRLX_ERR_INVALID, "a streamed call is in progress on this context (grlx_evaluate_trajectory_stream has not returned): no other call on it is served from inside the sink");
  if (ctx->run_pending)
  {
    HIP_TRY(hipStreamSynchronize(ctx->run_stream));
    ctx->run_pending = false;
  }
  return GRLX_OK;
}

// Re-hash every table of the context into tables of 2^new_logC entries per replica.  Positions are internal to the tables,
// to the persisted actor-critic trace and to the target values (both translated); nothing else refers to them.
int grow_tables(grlx_ctx *ctx, uint32_t new_logC)
{
  if (new_logC <= ctx->P.logC) return GRLX_OK;
  if (new_logC > 26) return fail(GRLX_ERR_INVALID, "tables cannot grow beyond 2^26 entries");
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)ctx->P.n_replicas;
  const size_t new_bytes = table_bytes(ctx, new_logC);
  Dev<Entry> nt;                            // freed on every early return; ownership moves to the context at the end
  Dev<uint32_t> remap;
  Dev<double> ntv;
  if (nt.alloc(new_bytes) != hipSuccess ||
      ((ctx->trace_state || ctx->tvals) && remap.alloc((N * sizeof(uint32_t)) << ctx->P.logC) != hipSuccess) ||
      (ctx->tvals && ntv.alloc(tval_bytes(N, new_logC)) != hipSuccess))
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "no device memory to grow the sparse tables to 2^%u entries per replica (%.1f GiB)", new_logC,
                (double)new_bytes / 1073741824.);
  }
  HIP_TRY(hipMemset(nt.get(), 0, new_bytes));
  if (ntv) HIP_TRY(hipMemset(ntv.get(), 0xFF, tval_bytes(N, new_logC)));
  HIP_TRY(launch_rehash(ctx->P, ctx->n_tables, nt.get(), new_logC, remap.get(), nullptr));
  if (remap) HIP_TRY(launch_remap_positions(ctx->P, remap.get(), new_logC, ntv.get(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  ctx->tables = std::move(nt);
  ctx->tvals = std::move(ntv);
  bind_params(ctx, new_logC, &ctx->P);
  return GRLX_OK;
}

// The growth rule applied (growth_target, grlx_host_rules.h) to `used`, the slots of the fullest table; every site has its own way of
// obtaining it.  Growing needs the old and the new tables at once: when that does not fit, the run goes on in the tables it has (a quarter
// full is not an overflow; a real one is still reported as GRLX_ERR_TABLE_FULL) and does not try again.
int grow_if_loaded(grlx_ctx *ctx, uint32_t used)
{
  const int rc = grow_tables(ctx, growth_target(used, ctx->P.logC, ctx->logC_max));
  if (rc != GRLX_ERR_OOM) return rc;
  g_err.clear();
  ctx->logC_max = ctx->P.logC;
  return GRLX_OK;
}

// The one place the context's device pointers (and the tables' size, which goes with them) enter a parameter block: the context's own
// after create, a growth, a snapshot load and the first per-step agent call; the launch copy of grlx_run after a growth between launches.
void bind_params(const grlx_ctx *ctx, uint32_t logC, DevParams *P)
{
  P->tables = ctx->tables.get(); P->logC = logC; P->tvals = ctx->tvals.get(); P->states = ctx->states.get();
  P->row_reward = ctx->row_reward.get(); P->row_time = ctx->row_time.get(); P->row_steps = ctx->row_steps.get(); P->row_trial = ctx->row_trial.get();
  P->taps = ctx->taps.get(); P->tap_count = ctx->tap_count.get(); P->trace_state = ctx->trace_state.get();
  P->queue = ctx->queue.get(); P->park = ctx->park.get(); P->agent_rep = ctx->agent_rep.get(); P->agent_lane = ctx->agent_lane.get();
}

// a persisted trace ([replica][16 lanes][kMaxTrace][2]: position, count | weight) with every entry invalid
hipError_t upload_empty_trace(uint32_t *dst, size_t N)
{
  std::vector<uint32_t> init(trace_words(N), 0u);
  for (size_t i = 0; i < init.size(); i += 2) init[i] = kInvalidPos;
  return hipMemcpy(dst, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
}

} // namespace grlx

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
  const size_t tbytes = table_bytes((size_t)N, n_tables, logC), row_cells = (size_t)N * (size_t)cfg->max_rows;
#define CTX_TRY(expr)   /* a half-built context goes with its owners */                                                                       \
  do { const hipError_t e__ = (expr); if (e__ != hipSuccess) { delete ctx; return fail(e__ == hipErrorOutOfMemory ? GRLX_ERR_OOM : GRLX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); } } while (0)
  CTX_TRY(ctx->tables.alloc(tbytes));
  CTX_TRY(hipMemset(ctx->tables.get(), 0, tbytes));
  CTX_TRY(ctx->states.alloc(sizeof(ReplicaState) * (size_t)N));
  CTX_TRY(ctx->row_reward.alloc(sizeof(double) * row_cells));
  CTX_TRY(ctx->row_steps.alloc(sizeof(int64_t) * row_cells));
  CTX_TRY(ctx->row_trial.alloc(sizeof(int64_t) * row_cells));
  CTX_TRY(hipMemset(ctx->row_reward.get(), 0, sizeof(double) * row_cells));
  CTX_TRY(hipMemset(ctx->row_steps.get(), 0, sizeof(int64_t) * row_cells));
  CTX_TRY(hipMemset(ctx->row_trial.get(), 0, sizeof(int64_t) * row_cells));
  CTX_TRY(ctx->row_time.alloc(sizeof(double) * row_cells));
  CTX_TRY(hipMemset(ctx->row_time.get(), 0, sizeof(double) * row_cells));
  CTX_TRY(ctx->scratch.alloc(sizeof(uint64_t) * 8));
  CTX_TRY(ctx->queue.alloc(sizeof(uint32_t)));
  // (the sub-batches beyond the second of a 12- / 16-replica wave park their lane state in registers since round 4: no buffer)
  if (P.replicas_per_wave == 32)      // ... five of the eight sub-batches of a 32-replica wave here (grlx_rollout_wide.h: MEMP)
    CTX_TRY(ctx->park.alloc(kAcParkBytes * 5 * (((size_t)N + 31) / 32)));
  CTX_TRY(ctx->max_load.alloc(sizeof(uint32_t)));
  CTX_TRY(hipMemset(ctx->max_load.get(), 0, sizeof(uint32_t)));
  CTX_TRY(ctx->tap_count.alloc(sizeof(uint32_t)));
  CTX_TRY(hipMemset(ctx->tap_count.get(), 0, sizeof(uint32_t)));
  if (cfg->agent == GRLX_AGENT_AC)
  { // the critic's trace survives launches: positions live here, all entries invalid at first
    CTX_TRY(ctx->trace_state.alloc(trace_words((size_t)N) * sizeof(uint32_t)));
    CTX_TRY(upload_empty_trace(ctx->trace_state.get(), (size_t)N));
  }
  if (P.target_interval > 0)
  {
    CTX_TRY(ctx->tvals.alloc(tval_bytes((size_t)N, logC)));
    CTX_TRY(hipMemset(ctx->tvals.get(), 0xFF, tval_bytes((size_t)N, logC)));      // all ones = not materialised
  }
  if (ctx->no_trace_td)
  { // the records of the sweep kernels, every replica with the configuration's values (grlx_set_replica_params overwrites them)
    SweepParams w;
    w.alpha = P.alpha; w.gamma = P.gamma; w.gl = P.gl; w.epsilon = P.epsilon;
    std::vector<SweepParams> rec((size_t)N, w);
    CTX_TRY(ctx->sweep_dev.alloc(sizeof(SweepParams) * (size_t)N));
    CTX_TRY(hipMemcpy(ctx->sweep_dev.get(), rec.data(), sizeof(SweepParams) * (size_t)N, hipMemcpyHostToDevice));
  }
  if (P.tap_capacity > 0)
  {
    CTX_TRY(ctx->taps.alloc(sizeof(grlx_tap) * (size_t)P.tap_capacity));
    CTX_TRY(hipMemset(ctx->taps.get(), 0, sizeof(grlx_tap) * (size_t)P.tap_capacity));
  }

  // Seed every replica exactly as `grld -s seed` instantiates the yaml
  // (deployer.cpp:70-74; configurable.cpp:627-654 instantiate order):
  //   srand48(seed) -> representation reset: thread-local Rand seeded by global lrand48 #1,
  //   memory*outputs uniforms drawn -> learning sampler Rand (global #2) -> test sampler Rand (global #3).
  std::vector<ReplicaState> hs((size_t)N);
  const uint64_t draws = table_draws(*cfg);
  for (int r = 0; r < N; ++r)
  {
    ReplicaState &s = hs[(size_t)r];
    memset(&s, 0, sizeof(s));
    uint64_t G = h_seed((long)seeds[r]);
    G = h_next(G);
    s.TL0 = h_seed((long)(G >> 17));
    s.TL = h_jump(s.TL0, draws);
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
  CTX_TRY(hipMemcpy(ctx->states.get(), hs.data(), sizeof(ReplicaState) * (size_t)N, hipMemcpyHostToDevice));
#undef CTX_TRY

  ctx->P = P;
  bind_params(ctx, logC, &ctx->P);
  *out = ctx;
  return GRLX_OK;
}

int grlx_destroy(grlx_ctx *ctx)
{
  STREAM_REFUSES(ctx, "grlx_destroy");
  delete ctx;     // (null: nothing to do) every device allocation, stream and event of the context goes with its owner
  return GRLX_OK;
}

int grlx_set_diag(grlx_ctx *ctx, int enable)
{
  if (!ctx) return fail(GRLX_ERR_INVALID, "null ctx");
  STREAM_REFUSES(ctx, "grlx_set_diag");
  if (enable && ctx->sweep) return fail(GRLX_ERR_INVALID, "diagnostics are not built for a sweep context (grlx_set_replica_params)");
  if (enable == 2 && ctx->cfg.trace == GRLX_TRACE_NONE)
    return fail(GRLX_ERR_INVALID, "stamps of the production ordering (grlx_set_diag 2) are not built for a context without a trace "
                                  "(trace = GRLX_TRACE_NONE): use the in-place stamps (grlx_set_diag 1)");
  const size_t waves = ((size_t)ctx->P.n_replicas + kReplicasPerWave - 1) / kReplicasPerWave;
  if (enable && !ctx->diag.get())
  {
    Dev<unsigned long long> diag;
    HIP_TRY(diag.alloc(waves * 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(diag.get(), 0, waves * 8 * sizeof(unsigned long long)));
    ctx->diag = std::move(diag);
  }
  ctx->P.diag_out = enable ? ctx->diag.get() : nullptr;
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
  HIP_TRY(hipMemcpy(out, ctx->diag.get(), (size_t)waves * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  *n_waves = waves;
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
  STREAM_REFUSES(ctx, "grlx_reset_run");
  DRAIN(ctx);
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)ctx->P.n_replicas;
  std::vector<ReplicaState> hs(N);
  HIP_TRY(hipMemcpy(hs.data(), ctx->states.get(), sizeof(ReplicaState) * N, hipMemcpyDeviceToHost));
  const uint64_t draws = table_draws(ctx->cfg);      // the walk reaches what construction drew for, in its order
  for (ReplicaState &s : hs)
  {
    s.sync_count = 0;
    s.syncs = 0;
    s.TL0 = s.TL;                         // the re-draw starts where the stream stands
    s.TL = h_jump(s.TL, draws);
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
  HIP_TRY(hipMemcpy(ctx->states.get(), hs.data(), sizeof(ReplicaState) * N, hipMemcpyHostToDevice));
  // (emptying the tables drops the claims of projector/tile_coding:safe with them: tile_coding.cpp:82-89)
  HIP_TRY(hipMemset(ctx->tables.get(), 0, table_bytes(ctx, ctx->P.logC)));
  if (ctx->tvals) HIP_TRY(hipMemset(ctx->tvals.get(), 0xFF, tval_bytes(N, ctx->P.logC)));      // kTvalUnset: not materialised
  HIP_TRY(hipMemset(ctx->max_load.get(), 0, sizeof(uint32_t)));
  if (ctx->trace_state) HIP_TRY(upload_empty_trace(ctx->trace_state.get(), N));
  if (ctx->tap_count) HIP_TRY(hipMemset(ctx->tap_count.get(), 0, sizeof(uint32_t)));
  if (ctx->agent_rep) HIP_TRY(hipMemset(ctx->agent_rep.get(), 0, sizeof(AgentRep) * N));
  if (ctx->agent_lane) HIP_TRY(hipMemset(ctx->agent_lane.get(), 0, sizeof(uint32_t) * N * 16 * 2));
  for (Dev<double> &timg : ctx->target_images) timg.reset();
  ctx->trials_run = 0;
  return GRLX_OK;
}

} // extern "C"
