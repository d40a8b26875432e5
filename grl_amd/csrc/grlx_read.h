// grlx_read.h -- what the read calls of both contexts share (grlx_api_read.cpp: grlx_ctx, grlx_api_fqi.cpp: grlx_fqi_ctx) and that needs
// neither: the staging bound, the skeleton that takes a call's columns through the device a chunk at a time, and the rules both sides
// state about replica ranges, start states and records.  Host code only.
#pragma once
#include <initializer_list>
#include "grlx_host.h"

namespace grlx {

// device staging one read holds at most (grlx_set_query_chunk_bytes)
constexpr uint64_t kQueryChunkDefault = 256ull << 20;
inline uint64_t g_query_chunk_bytes = kQueryChunkDefault;

// columns (observations or start states) per chunk so that one chunk's device arrays stay within the bound; at least one
inline int query_chunk(int n, size_t bytes_per_column) { return query_chunk(g_query_chunk_bytes, n, bytes_per_column); }

// rows [n_replicas] of `elem` bytes per observation: device [r][chunk] -> host [r][n_obs] at observation o0
inline hipError_t query_copy_out(void *host, const void *dev, size_t elem, int n_replicas, int n_obs, int o0, int nc)
{
  return hipMemcpy2D((char *)host + (size_t)o0 * elem, (size_t)n_obs * elem, dev, (size_t)nc * elem, (size_t)nc * elem, (size_t)n_replicas,
                     hipMemcpyDeviceToHost);
}

// grlx_read_kernel_timing (include/grlx_diag.h): the device time of the chunks' launches, summed since timing was enabled
inline bool g_read_timing = false;
inline double g_read_ms = 0;
inline int g_read_chunks = 0;

struct ReadTimer {
  DevEvent e0, e1;
  hipError_t start()
  {
    if (hipError_t err = e0.create(hipEventDefault)) return err;
    if (hipError_t err = e1.create(hipEventDefault)) return err;
    return hipEventRecord(e0.get(), nullptr);
  }
  hipError_t stop()
  {
    if (hipError_t err = hipEventRecord(e1.get(), nullptr)) return err;
    if (hipError_t err = hipEventSynchronize(e1.get())) return err;
    float ms = 0;
    if (hipError_t err = hipEventElapsedTime(&ms, e0.get(), e1.get())) return err;
    g_read_ms += ms;
    g_read_chunks++;
    return hipSuccess;
  }
};

// One output of a chunked read: `rows` rows of `elem` bytes per column, copied to `host` when that is not null; `on_device`: the kernels
// write it (or a reduction reads it) whether the caller asked for it or not.
struct ReadOut { void *host; size_t elem; int rows; bool on_device; };
constexpr int kMaxReadOuts = 11;
// A second per-column input of a chunked read, laid out like an output: host [rows][cols] of `elem` bytes -> `dev` [rows][chunk], so that
// a chunk's rows begin at its first column for EVERY row (a strided copy, not a contiguous one).  host null: nothing is staged.  `dev`:
// where the skeleton put it, for the launch to read.
struct ReadIn { const void *host; size_t elem; int rows; void *dev; };
// a chunk's device array as the launch sees it; null: neither asked for nor needed
struct DevPtr {
  void *p = nullptr;
  void *get() const { return p; }
  template <typename U> U *as() const { return (U *)p; }
};
// What the caller's context adds around a chunk's kernels: the poison launch before them (GRLX_POISON_REGISTERS) and their device time
// in grlx_read_kernel_timing's sum.  The batch path's reads have neither (kPlainRead).
struct ReadHooks { bool poison; uint32_t poison_pattern; bool timed; };
constexpr ReadHooks kPlainRead = {false, 0, false};

// The skeleton of every read: the columns of `in` (observations or start states, `in_dims` doubles each) go through the device `chunk` at a
// time.  Per chunk: the input in, launch(nc, input, outputs) -- device pointers, null for an output neither asked for nor needed -- and out
// what the caller asked for.  `sync_each`: every output may be null, so the next chunk's copy-in must not overtake the launch.
// `extra`: a second input staged beside the first (ReadIn), or null.  The chunk's arrays share ONE allocation, each at a multiple of 256
// bytes; when the device has no room for it the call is refused with GRLX_ERR_OOM.
template <typename Launch>
int chunked_read(const ReadHooks &hooks, const ReadOut *outs, int n_outs, int cols, const double *in, int in_dims, int chunk, bool sync_each,
                 Launch launch, ReadIn *extra = nullptr)
{
  size_t bytes = 0;
  auto place = [&](size_t b) { const size_t at = bytes; bytes += (b + 255) & ~(size_t)255; return at; };
  const size_t at_in = place(sizeof(double) * (size_t)chunk * in_dims);
  const size_t at_extra = extra && extra->host ? place(extra->elem * (size_t)extra->rows * (size_t)chunk) : 0;
  size_t at_out[kMaxReadOuts] = {};
  for (int k = 0; k < n_outs; ++k)
    if (outs[k].host || outs[k].on_device) at_out[k] = place(outs[k].elem * (size_t)outs[k].rows * (size_t)chunk);
  DevBuf stage;
  if (stage.alloc(bytes) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "out of device memory (%zu bytes of staging; lower the bound with grlx_set_query_chunk_bytes)", bytes);
  }
  const double *din = (const double *)(stage.as<char>() + at_in);
  if (extra) extra->dev = extra->host ? stage.as<char>() + at_extra : nullptr;
  DevPtr dout[kMaxReadOuts];
  for (int k = 0; k < n_outs; ++k)
    if (outs[k].host || outs[k].on_device) dout[k].p = stage.as<char>() + at_out[k];
  for (int c0 = 0; c0 < cols; c0 += chunk)
  {
    const int nc = cols - c0 < chunk ? cols - c0 : chunk;
    HIP_TRY(hipMemcpy((void *)din, in + (size_t)c0 * in_dims, sizeof(double) * (size_t)nc * in_dims, hipMemcpyHostToDevice));
    if (extra && extra->host)
      HIP_TRY(hipMemcpy2D(extra->dev, (size_t)nc * extra->elem, (const char *)extra->host + (size_t)c0 * extra->elem, (size_t)cols * extra->elem,
                          (size_t)nc * extra->elem, (size_t)extra->rows, hipMemcpyHostToDevice));
    if (hooks.poison) HIP_TRY(launch_poison_registers(hooks.poison_pattern, nullptr));
    if (hooks.timed && g_read_timing)
    { // grlx_read_kernel_timing: events around the chunk's launches, waited for here
      ReadTimer timer;
      HIP_TRY(timer.start());
      if (int rc = launch(nc, din, dout)) return rc;
      HIP_TRY(timer.stop());
    }
    else if (int rc = launch(nc, din, dout)) return rc;
    for (int k = 0; k < n_outs; ++k)
      if (outs[k].host) HIP_TRY(query_copy_out(outs[k].host, dout[k].get(), outs[k].elem, outs[k].rows, cols, c0, nc));
    if (sync_each) HIP_TRY(hipDeviceSynchronize());
  }
  return GRLX_OK;
}

// ---- the rules both contexts state, each once; R: the context's replicas, S: the doubles of a model state
// the replica range every read names: [first_replica, first_replica + n_replicas) inside the context
inline int replica_range_ok(const char *who, int R, int first_replica, int n_replicas)
{
  if (first_replica < 0 || n_replicas < 0 || (int64_t)first_replica + n_replicas > R)
    return fail(GRLX_ERR_INVALID, "%s: replica range [%d, %lld) is outside the context's %d replicas", who, first_replica,
                (long long)first_replica + n_replicas, R);
  return GRLX_OK;
}

// what every evaluation says about its pairs: the count of start states, the replica range, the start states, the bounds of max_steps
inline int episode_pairs_ok(const char *who, int R, int S, int first_replica, int n_replicas, const double *states, int n_starts, int max_steps)
{
  if (n_starts < 0) return fail(GRLX_ERR_INVALID, "%s: n_starts = %d", who, n_starts);
  if (int rc = replica_range_ok(who, R, first_replica, n_replicas)) return rc;
  if (!states) return fail(GRLX_ERR_INVALID, "%s: states is null", who);
  if (max_steps < 0 || max_steps > GRLX_MAX_EPISODE_STEPS)
    return fail(GRLX_ERR_INVALID, "%s: max_steps = %d is outside 1 ... GRLX_MAX_EPISODE_STEPS (%d; 0 = that cap)", who, max_steps, GRLX_MAX_EPISODE_STEPS);
  for (int s = 0; s < n_starts; ++s)
    for (int i = 0; i < S; ++i)
    { // below 2^17 the RK4 stages of one step stay inside the branch-free sine's domain (the cart-pole's case)
      const double v = states[(size_t)s * S + i];
      if (!std::isfinite(v)) return fail(GRLX_ERR_INVALID, "%s: state row %d, component %d is not finite (%g)", who, s, i, v);
      if (!(fabs(v) < 0x1p17)) return fail(GRLX_ERR_INVALID, "%s: state row %d, component %d (%g) is out of range: its magnitude reaches 2^17", who, s, i, v);
    }
  return GRLX_OK;
}

inline int group_size_ok(const char *who, int group_size)
{
  if (group_size < 1) return fail(GRLX_ERR_INVALID, "%s: group_size = %d is below 1", who, group_size);
  return GRLX_OK;
}

// What a trajectory call checks beyond its sibling, after the sibling's own checks; gives the start states per chunk.  `rows`: replicas or
// groups; `in_and_sums`: a start state's other staged bytes (episode_start_bytes).  Unlike the other reads a chunk never exceeds the
// bound: the records are what the bound is for, so a column that does not fit is refused instead of staged as "at least one".
inline int trajectory_admit(const char *who, const char *sibling, const void *records, int max_steps, int rows, int n_starts, int R, size_t in_and_sums,
                            int *chunk)
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

// ---- what the two batch contexts' episode calls (grlx_fqi_evaluate*, grlx_lspi_evaluate*) share
// what their grouped calls check after their single-policy sibling's rules
inline int batch_ensemble_admit(const char *who, int n_replicas, int group_size)
{
  if (int rc = group_size_ok(who, group_size)) return rc;
  if (n_replicas % group_size != 0)
    return fail(GRLX_ERR_INVALID, "%s: n_replicas = %d is not a multiple of group_size = %d", who, n_replicas, group_size);
  return GRLX_OK;
}

// ---- their sampled episodes: the samplers of one policy, the draw from a group's majority or rank votes.  What they check beyond their
// greedy siblings follows grlx_api_read.cpp's sampled_admit / ensemble_sampled_admit; a batch context has no sampler stream and no epsilon
// of its own, so what would read them is refused by name.
inline int batch_epsilon_ok(const char *who, double e, const char *of)
{
  if (!std::isfinite(e)) return fail(GRLX_ERR_INVALID, "%s: epsilon is not finite (%g)%s", who, e, of);
  if (e == GRLX_EPSILON_OWN)
    return fail(GRLX_ERR_INVALID, "%s: GRLX_EPSILON_OWN (-1) is refused: a batch context has no epsilon of its own; name a number in [0, 1]%s", who, of);
  if (!(e >= 0. && e <= 1.)) return fail(GRLX_ERR_INVALID, "%s: epsilon = %g is outside [0, 1]%s", who, e, of);
  return GRLX_OK;
}

inline int batch_sampled_admit(const char *who, int n_replicas, int n_starts, int sampler, double epsilon, const uint64_t *streams)
{
  if (sampler != GRLX_SAMPLER_GREEDY && sampler != GRLX_SAMPLER_EPSILON_GREEDY)
    return fail(GRLX_ERR_INVALID, "%s: unknown sampler %d (GRLX_SAMPLER_GREEDY = 0, GRLX_SAMPLER_EPSILON_GREEDY = 1)", who, sampler);
  if (int rc = batch_epsilon_ok(who, epsilon, "")) return rc;
  if (!streams && sampler == GRLX_SAMPLER_EPSILON_GREEDY)
    return fail(GRLX_ERR_INVALID, "%s: streams is null under GRLX_SAMPLER_EPSILON_GREEDY: a batch context has no sampler stream of its own to copy "
                "(grlx_episode_streams makes them)", who);
  if (streams)
    for (int64_t row = 0; row < (int64_t)n_replicas * n_starts; ++row)
      for (int w = 0; w < 2; ++w)
        if (streams[row * 2 + w] >> 48)
          return fail(GRLX_ERR_INVALID, "%s: stream row %lld (replica %lld, start state %lld), word %d is 0x%llx: a rand48 state is below 2^48", who,
                      (long long)row, (long long)(row / n_starts), (long long)(row % n_starts), w, (unsigned long long)streams[row * 2 + w]);
  return GRLX_OK;
}

inline int batch_ensemble_sampled_admit(const char *who, int n_replicas, int group_size, int n_starts, int strategy, double tau, int member, double member_param,
                                        const uint64_t *streams)
{
  if (int rc = batch_ensemble_admit(who, n_replicas, group_size)) return rc;
  if (strategy != GRLX_ENSEMBLE_MAJORITY && strategy != GRLX_ENSEMBLE_RANK)
    return fail(GRLX_ERR_INVALID, "%s: unknown strategy %d (GRLX_ENSEMBLE_MAJORITY = 0, GRLX_ENSEMBLE_RANK = 1)", who, strategy);
  if (!std::isfinite(tau) || !(tau > 0.)) return fail(GRLX_ERR_INVALID, "%s: tau = %g is not a finite temperature above 0", who, tau);
  switch (member)
  {
    case GRLX_MEMBER_GREEDY: break;
    case GRLX_MEMBER_EPSILON:
      if (int rc = batch_epsilon_ok(who, member_param, " (GRLX_MEMBER_EPSILON)")) return rc;
      break;
    case GRLX_MEMBER_SOFTMAX:
      if (!std::isfinite(member_param) || !(member_param > 0.))
        return fail(GRLX_ERR_INVALID, "%s: tau_m = %g is not a finite temperature above 0 (GRLX_MEMBER_SOFTMAX)", who, member_param);
      break;
    default:
      return fail(GRLX_ERR_INVALID, "%s: unknown member sampler %d (GRLX_MEMBER_GREEDY = 0, GRLX_MEMBER_EPSILON = 1, GRLX_MEMBER_SOFTMAX = 2)", who, member);
  }
  if (streams)
    for (int64_t row = 0; row < (int64_t)(n_replicas / group_size) * n_starts; ++row)
      if (streams[row] >> 48)
        return fail(GRLX_ERR_INVALID, "%s: stream row %lld (group %lld, start state %lld) is 0x%llx: a rand48 state is below 2^48", who, (long long)row,
                    (long long)(row / n_starts), (long long)(row % n_starts), (unsigned long long)streams[row]);
  return GRLX_OK;
}

// An admitted episode call over `rows` replicas or groups of a batch context whose model state has S components, as the skeleton takes
// it: the start states per chunk and the outputs -- the six every call has, `own` (the ensemble's two), `more` (the sampled calls':
// explored, the streams after), the records of `words` doubles per step.  sibling null: the sums alone, max_steps = 0 is the cap; else
// trajectory_admit's checks come first.  in_bytes: what a pair stages beside its start state (the streams that go in).
struct BatchEpisodes {
  int     chunk = 0, n_outs = 0;
  ReadOut outs[kMaxReadOuts];
};
inline int batch_episodes(BatchEpisodes &e, const char *who, const char *sibling, int S, int rows, int n_starts, int *max_steps, double *ret, double *disc,
                          int32_t *steps, int32_t *terminal, int32_t *ties, double *final_state, std::initializer_list<int64_t *> own, double *records,
                          int words, std::initializer_list<ReadOut> more = {}, size_t in_bytes = 0)
{
  size_t extra = own.size() * sizeof(int64_t) + in_bytes;
  for (const ReadOut &o : more) extra += o.elem;
  const size_t in_and_sums = episode_start_bytes(S, rows, extra);
  // the launches read d[6 + own + more] for the records whether they were asked for or not: that slot exists in the skeleton's arrays
  if (6 + own.size() + more.size() + 1 > (size_t)kMaxReadOuts)
    return fail(GRLX_ERR_INVALID, "%s: %zu outputs exceed the read skeleton's kMaxReadOuts = %d", who, 6 + own.size() + more.size() + 1, kMaxReadOuts);
  if (sibling)
  {
    if (int rc = trajectory_admit(who, sibling, records, *max_steps, rows, n_starts, words, in_and_sums, &e.chunk)) return rc;
  }
  else
  {
    if (*max_steps == 0) *max_steps = GRLX_MAX_EPISODE_STEPS;
    e.chunk = query_chunk(n_starts, in_and_sums);
  }
  for (const ReadOut &o : {ReadOut{ret, sizeof(double), rows, true}, ReadOut{disc, sizeof(double), rows, true}, ReadOut{steps, sizeof(int32_t), rows, true},
                           ReadOut{terminal, sizeof(int32_t), rows, true}, ReadOut{ties, sizeof(int32_t), rows, true},
                           ReadOut{final_state, sizeof(double) * (size_t)S, rows, true}})
    e.outs[e.n_outs++] = o;
  for (int64_t *p : own) e.outs[e.n_outs++] = {p, sizeof(int64_t), rows, true};
  for (const ReadOut &o : more) e.outs[e.n_outs++] = o;
  if (sibling) e.outs[e.n_outs++] = {records, sizeof(double) * (size_t)words * (size_t)*max_steps, rows, true};
  return GRLX_OK;
}

} // namespace grlx
