// grlx_api_tables.cpp -- the C ABI declared in include/grlx.h: a context's state, weights and table operations -- environment state, streams, table load, target weights, taps, reading / exporting / loading weights, and grlx_read / _write / _update.
#include <algorithm>
#include "grlx_host.h"

extern "C" {

int grlx_get_env_state(grlx_ctx *ctx, int replica, double *state)
{
  if (!ctx || !state || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(read_state(ctx, replica, &s));
  memcpy(state, s.x, sizeof(double) * GRLX_MAX_STATE);
  return GRLX_OK;
}

int grlx_get_rng(grlx_ctx *ctx, int replica, uint64_t out[4])
{
  if (!ctx || !out || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(read_state(ctx, replica, &s));
  out[0] = s.G; out[1] = s.TL; out[2] = s.S1; out[3] = s.S2;
  return GRLX_OK;
}

int grlx_table_load(grlx_ctx *ctx, int table, int replica, uint32_t *n_slots_used)
{
  if (!ctx || !n_slots_used || table < 0 || table >= ctx->n_tables || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  ReplicaState s;
  DRAIN(ctx);
  HIP_TRY(read_state(ctx, replica, &s));
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
    HIP_TRY(read_state(ctx, replica, &s));
    *n_syncs = s.syncs;
  }
  if (n == 0) return GRLX_OK;
  DevBuf ds, dout;
  HIP_TRY(ds.upload(slots, sizeof(uint32_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(launch_get_target_weights(ctx->P, replica, ds.as<uint32_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_read_taps(grlx_ctx *ctx, grlx_tap *out, int cap, int *n)
{
  if (!ctx || !out || !n) return fail(GRLX_ERR_INVALID, "bad argument");
  uint32_t cnt = 0;
  DRAIN(ctx);
  HIP_TRY(hipMemcpy(&cnt, ctx->tap_count.get(), sizeof(cnt), hipMemcpyDeviceToHost));
  int m = (int)cnt < cap ? (int)cnt : cap;
  if (m > ctx->P.tap_capacity) m = ctx->P.tap_capacity;
  if (m > 0) HIP_TRY(hipMemcpy(out, ctx->taps.get(), sizeof(grlx_tap) * (size_t)m, hipMemcpyDeviceToHost));
  *n = m;
  return GRLX_OK;
}

int grlx_get_weights(grlx_ctx *ctx, int table, int replica, const uint32_t *slots, int n, double *out)
{
  if (!ctx || !slots || !out || n < 0 || table < 0 || table >= ctx->n_tables || replica < 0 || replica >= ctx->P.n_replicas) return fail(GRLX_ERR_INVALID, "bad argument");
  if (n == 0) return GRLX_OK;
  DRAIN(ctx);
  DevBuf ds, dout;
  HIP_TRY(ds.upload(slots, sizeof(uint32_t) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(launch_get_weights(ctx->P, table, replica, ds.as<uint32_t>(), n, dout.as<double>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * memory, hipMemcpyDeviceToHost));
  return GRLX_OK;
}

int grlx_load_weights(grlx_ctx *ctx, int table, int first_replica, int n_replicas, const double *dense, uint64_t count)
{
  if (!ctx || !dense || table < 0 || table >= ctx->n_tables) return fail(GRLX_ERR_INVALID, "bad argument");
  STREAM_REFUSES(ctx, "grlx_load_weights");
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
  Dev<double> image;
  if (image.alloc(sizeof(double) * memory) != hipSuccess) return fail(GRLX_ERR_OOM, "no device memory for a %zu-weight policy image", memory);
  // (a target network with tau != 0: one new dense vector per replica, allocated before anything is touched -- a failure leaves the context as it was)
  std::vector<Dev<double>> fresh((size_t)n_replicas);
  if (target_images)
    for (int k = 0; k < n_replicas; ++k)
      if (fresh[(size_t)k].alloc(sizeof(double) * memory) != hipSuccess)
      {
        (void)hipGetLastError();
        return fail(GRLX_ERR_OOM, "no device memory for the target vector of replica %d", first_replica + k);
      }
  double *const img = image.get();
  ctx->images.push_back(std::move(image));
  {
    std::vector<int> &of = ctx->image_of[table];
    if (of.empty()) of.assign((size_t)N, -1);
    const int mine = (int)ctx->images.size() - 1;
    for (int r = first_replica; r < first_replica + n_replicas; ++r) of[(size_t)r] = mine;
  }
  HIP_TRY(hipMemcpy(img, dense, sizeof(double) * memory, hipMemcpyHostToDevice));
  if (with_target)
  { // the target's new values, from its values NOW (entries and lazily defined ones alike), BEFORE the tables are emptied
    if (ctx->target_images.empty()) ctx->target_images.resize((size_t)N);
    std::vector<ReplicaState> hs((size_t)n_replicas);
    HIP_TRY(hipMemcpy(hs.data(), ctx->states.get() + first_replica, sizeof(ReplicaState) * (size_t)n_replicas, hipMemcpyDeviceToHost));
    if (target_images)
      for (int k = 0; k < n_replicas; ++k) HIP_TRY(launch_target_after_load(ctx->P, first_replica + k, img, fresh[(size_t)k].get(), nullptr));
    HIP_TRY(hipDeviceSynchronize());          // (the kernels read the vectors of an earlier load for the last time)
    for (int k = 0; k < n_replicas; ++k)
    {
      const int r = first_replica + k;
      ctx->target_images[(size_t)r] = std::move(fresh[(size_t)k]);
      hs[(size_t)k].target_base = ctx->target_images[(size_t)r].get();
      hs[(size_t)k].syncs += 1;                     // the load's synchronize() (count_ = 0, representation.h:284-296)
      hs[(size_t)k].syncs_base = hs[(size_t)k].syncs;
      hs[(size_t)k].sync_count = 0;
    }
    HIP_TRY(hipMemcpy(ctx->states.get() + first_replica, hs.data(), sizeof(ReplicaState) * (size_t)n_replicas, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(ctx->tvals.get() + ((size_t)first_replica << ctx->P.logC), 0xFF, tval_bytes((size_t)n_replicas, ctx->P.logC)));      // kTvalUnset
  }
  // setParams() overwrites every weight: forget the sparse tables of these replicas; every slot is
  // re-created on first touch from the image
  const size_t per_replica = sizeof(Entry) << ctx->P.logC;
  Entry *base = ctx->tables.get() + (((size_t)table * (size_t)N + (size_t)first_replica) << ctx->P.logC);
  if (ctx->P.twin_tables)      // twin tables keep their common key layout: the entries stay and take their values from the image
    HIP_TRY(launch_reload_entries(ctx->P, table, first_replica, n_replicas, img, nullptr));
  else
    HIP_TRY(hipMemset(base, 0, per_replica * (size_t)n_replicas));
  HIP_TRY(launch_set_lazy_base(ctx->P, table, first_replica, n_replicas, img, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  // an earlier image that no replica of any table refers to any more goes now (repeated loads do not accumulate)
  for (size_t k = 0; k + 1 < ctx->images.size(); ++k)
  {
    bool used = false;
    for (const std::vector<int> &of : ctx->image_of) used = used || std::count(of.begin(), of.end(), (int)k) != 0;
    if (!used) ctx->images[k].reset();
  }
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
  HIP_TRY(dr.upload(replica, sizeof(int32_t) * (size_t)n));
  HIP_TRY(di.upload(idx, sizeof(uint32_t) * (size_t)n * T));
  HIP_TRY(da.alloc(sizeof(double) * (size_t)n));
  HIP_TRY(dout.alloc(sizeof(double) * (size_t)n));
  if (arg) HIP_TRY(hipMemcpy(da.get(), arg, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIP_TRY(launch_table_op(ctx->P, table, op, dr.as<int32_t>(), di.as<uint32_t>(), n, da.as<double>(), alpha, dout.as<double>(), nullptr));
  if (out) HIP_TRY(hipMemcpy(out, dout.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
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

} // extern "C"
