// grlx_api_snapshot.cpp -- the C ABI declared in include/grlx.h: exact resume -- snapshot info / size / save / load and their diagnostics.
#include "grlx_host.h"
#include "grlx_snapshot.h"

// ------------------------------------------------------------------------------------------------ exact resume ---
// A snapshot (layout: grlx_snapshot_format.h) is assembled in the caller's buffer section by section; the tables go through the
// compacting kernels of grlx_snapshot.hip.  A load validates and allocates everything first, unpacks into NEW tables, and only then
// touches the context.
namespace {

static_assert(sizeof(ReplicaState) == snap::kStateBytes, "grlx_snapshot_format.h: kStateBytes");
static_assert(offsetof(ReplicaState, lazy_base) == snap::kStatePointerOffsets[0] && offsetof(ReplicaState, lazy_base) + 8 == snap::kStatePointerOffsets[1] &&
              offsetof(ReplicaState, target_base) == snap::kStatePointerOffsets[2], "grlx_snapshot_format.h: kStatePointerOffsets");
static_assert(offsetof(ReplicaState, n_slots) == snap::kStateSlotsOffset && offsetof(ReplicaState, rows) == snap::kStateRowsOffset, "grlx_snapshot_format.h: state offsets");
static_assert(snap::kTraceWordsPerReplica == kRuleTraceWords, "grlx_snapshot_format.h: kTraceWordsPerReplica");

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
  for (const Dev<double> &t : ctx->target_images) target_image = target_image || t;
  if (!ctx->images.empty() || target_image)
    return fail(GRLX_ERR_INVALID, "%s: not built for a context that holds a loaded policy (grlx_load_weights): a snapshot carries no dense parameter vectors", who);
  if (ctx->agent_rep) return fail(GRLX_ERR_INVALID, "%s: not built for a context on which a per-step entry point has run (agent state in mid-episode)", who);
  if (ctx->cfg.env == GRLX_ENV_EXTERNAL) return fail(GRLX_ERR_INVALID, "%s: not built for GRLX_ENV_EXTERNAL", who);
  if (ctx->P.tap_capacity > 0 || ctx->P.diag_out || ctx->diag.get()) return fail(GRLX_ERR_INVALID, "%s: not built for a context with taps or diagnostics (grlx_set_diag)", who);
  return GRLX_OK;
}

// launch one of the two snapshot kernels on the null stream between two events: *ms = its device time (diagnostic, grlx_snapshot_timing)
int timed_snapshot_launch(hipError_t (*launch)(const SnapshotArgs &, hipStream_t), const SnapshotArgs &a, double *ms)
{
  DevEvent t0, t1;
  const bool timed = t0.create(hipEventDefault) == hipSuccess && t1.create(hipEventDefault) == hipSuccess;
  if (!timed) (void)hipGetLastError();
  if (timed) (void)hipEventRecord(t0.get(), nullptr);
  const hipError_t e = launch(a, nullptr);
  if (timed) (void)hipEventRecord(t1.get(), nullptr);
  float f = -1.f;
  if (e == hipSuccess && timed && hipEventSynchronize(t1.get()) == hipSuccess) (void)hipEventElapsedTime(&f, t0.get(), t1.get());
  *ms = f;
  if (e != hipSuccess) return fail(GRLX_ERR_HIP, "snapshot kernel launch failed: %s", hipGetErrorString(e));
  return GRLX_OK;
}

// The record streams of a snapshot, one per (table, replica) at index table * N + replica, in that order: counts[i] records starting at
// record offsets[i].  Returns their total.
uint64_t snapshot_streams(const std::vector<ReplicaState> &hs, size_t N, size_t T, std::vector<uint32_t> *counts, std::vector<uint64_t> *offsets)
{
  counts->assign(T * N, 0u);
  offsets->assign(T * N, 0ull);
  uint64_t n_records = 0;
  for (size_t t = 0; t < T; ++t)
    for (size_t r = 0; r < N; ++r)
    {
      (*counts)[t * N + r] = hs[r].n_slots[t];
      (*offsets)[t * N + r] = n_records;
      n_records += hs[r].n_slots[t];
    }
  return n_records;
}

// what the two snapshot kernels take: the tables (and target values) packed from or unpacked into, and the staged record stream
SnapshotArgs snapshot_args(const grlx_ctx *ctx, Entry *tables, double *tvals, const snap::Header &h, const DevBuf &off, const DevBuf &cnt, const DevBuf &rec,
                           const DevBuf &err)
{
  SnapshotArgs a;
  a.tables = tables; a.tvals = tvals; a.logC = h.logC; a.n_replicas = ctx->P.n_replicas; a.n_tables = ctx->n_tables;
  a.offsets = off.as<uint64_t>(); a.counts = cnt.as<uint32_t>(); a.records = rec.as<uint8_t>(); a.record_bytes = h.record_bytes; a.err = err.as<uint32_t>();
  return a;
}

// the header of a snapshot of the context as it stands (drained), its replica states with the device pointers zeroed, and the
// record count / first record of every stream (table * n_replicas + replica)
int snapshot_plan(grlx_ctx *ctx, snap::Header *h, std::vector<ReplicaState> *hs, std::vector<uint32_t> *counts, std::vector<uint64_t> *offsets)
{
  const size_t N = (size_t)ctx->P.n_replicas, T = (size_t)ctx->n_tables;
  hs->resize(N);
  HIP_TRY(hipMemcpy(hs->data(), ctx->states.get(), sizeof(ReplicaState) * N, hipMemcpyDeviceToHost));
  memset(h, 0, sizeof(*h));
  h->cfg = ctx->cfg;
  h->n_replicas = (uint32_t)N;
  h->n_tables = (uint32_t)T;
  h->logC = ctx->P.logC;
  h->trials_run = ctx->trials_run;
  h->flags = (ctx->sweep ? snap::kFlagSweep : 0u) | (ctx->trace_state.get() ? snap::kFlagTrace : 0u) | (ctx->tvals.get() ? snap::kFlagTarget : 0u) |
             (ctx->P.twin_tables ? snap::kFlagTwin : 0u);
  for (ReplicaState &s : *hs)
  {
    s.lazy_base[0] = s.lazy_base[1] = nullptr;
    s.target_base = nullptr;
    if (s.rows > h->rows) h->rows = s.rows;
  }
  h->n_records = snapshot_streams(*hs, N, T, counts, offsets);
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
    const void *src[4] = {ctx->row_reward.get(), ctx->row_time.get(), ctx->row_steps.get(), ctx->row_trial.get()};
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
    HIP_TRY(hipMemcpy(out, ctx->trace_state.get(), h.section_bytes[snap::SEC_TRACE], hipMemcpyDeviceToHost));
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
    HIP_TRY(hipMemcpy(off.get(), offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cnt.get(), counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.get(), 0, 4));
    const SnapshotArgs a = snapshot_args(ctx, ctx->tables.get(), ctx->tvals.get(), h, off, cnt, rec, err);
    if ((rc = timed_snapshot_launch(launch_snapshot_pack, a, &ctx->snap_pack_ms)) != GRLX_OK) return rc;
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, err.get(), 4, hipMemcpyDeviceToHost));
    if (e != 0) return fail(GRLX_ERR_INVALID, "grlx_snapshot_save: table occupancy and slot count disagree");
    HIP_TRY(hipMemcpy(out, rec.get(), h.section_bytes[snap::SEC_RECORDS], hipMemcpyDeviceToHost));
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
  STREAM_REFUSES(ctx, "grlx_snapshot_load");
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
  const uint32_t want_flags = (ctx->trace_state.get() ? snap::kFlagTrace : 0u) | (ctx->P.target_interval > 0 ? snap::kFlagTarget : 0u) | (ctx->P.twin_tables ? snap::kFlagTwin : 0u);
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
  for (size_t t = 0; t < T; ++t)
    for (size_t r = 0; r < N; ++r)
      if (hs[r].n_slots[t] > (1u << h.logC)) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: replica %zu, table %zu: %u records exceed the capacity 2^%u", r, t, hs[r].n_slots[t], h.logC);
  std::vector<uint32_t> counts;
  std::vector<uint64_t> offsets;
  const uint64_t n_records = snapshot_streams(hs, N, T, &counts, &offsets);
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
  const size_t tbytes = table_bytes(N, T, h.logC), tvbytes = tval_bytes(N, h.logC);
  Dev<Entry> nt;
  Dev<double> ntv;
  Dev<SweepParams> nsw;
  DevBuf rec, off, cnt, err;
  if (nt.alloc(tbytes) != hipSuccess || (ctx->tvals && ntv.alloc(tvbytes) != hipSuccess) || rec.alloc(h.section_bytes[snap::SEC_RECORDS]) != hipSuccess ||
      off.alloc(offsets.size() * 8) != hipSuccess || cnt.alloc(counts.size() * 4) != hipSuccess || err.alloc(4) != hipSuccess ||
      (!sweep_rec.empty() && !ctx->sweep_dev && nsw.alloc(sizeof(SweepParams) * N) != hipSuccess))
  {
    (void)hipGetLastError();
    return fail(GRLX_ERR_OOM, "grlx_snapshot_load: no device memory for tables of 2^%u entries per replica (%.1f GiB) and the record stream", h.logC, (double)tbytes / 1073741824.);
  }
  HIP_TRY(hipMemset(nt.get(), 0, tbytes));
  if (ntv) HIP_TRY(hipMemset(ntv.get(), 0xFF, tvbytes));
  if (h.n_records != 0)
  {
    HIP_TRY(hipMemcpy(rec.get(), records_in, h.section_bytes[snap::SEC_RECORDS], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(off.get(), offsets.data(), offsets.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cnt.get(), counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(err.get(), 0, 4));
    const SnapshotArgs a = snapshot_args(ctx, nt.get(), ntv.get(), h, off, cnt, rec, err);
    if ((rc = timed_snapshot_launch(launch_snapshot_unpack, a, &ctx->snap_unpack_ms)) != GRLX_OK) return rc;
    uint32_t e = 0;
    HIP_TRY(hipMemcpy(&e, err.get(), 4, hipMemcpyDeviceToHost));
    if (e != 0) return fail(GRLX_ERR_INVALID, "grlx_snapshot_load: a table record has an empty key, a position beyond the capacity, or is out of order");
  }
  // --- commit
  HIP_TRY(hipMemcpy(ctx->states.get(), hs.data(), sizeof(ReplicaState) * N, hipMemcpyHostToDevice));
  {
    const size_t part = 8 * (size_t)h.rows * N;
    void *dst[4] = {ctx->row_reward.get(), ctx->row_time.get(), ctx->row_steps.get(), ctx->row_trial.get()};
    for (int k = 0; k < 4 && part != 0; ++k) HIP_TRY(hipMemcpy(dst[k], rows_in + (size_t)k * part, part, hipMemcpyHostToDevice));
  }
  if (ctx->trace_state) HIP_TRY(hipMemcpy(ctx->trace_state.get(), trace_in, h.section_bytes[snap::SEC_TRACE], hipMemcpyHostToDevice));
  if (!sweep_rec.empty())
  {
    if (!ctx->sweep_dev) ctx->sweep_dev = std::move(nsw);
    HIP_TRY(hipMemcpy(ctx->sweep_dev.get(), sweep_rec.data(), sizeof(SweepParams) * N, hipMemcpyHostToDevice));
    for (int k = 0; k < 4; ++k) ctx->sweep_host[k].assign(sweep_in + (size_t)k * N, sweep_in + (size_t)(k + 1) * N);
    ctx->sweep = true;
    sweep_limits_layout(ctx->P);
  }
  ctx->tables = std::move(nt);
  ctx->tvals = std::move(ntv);
  bind_params(ctx, h.logC, &ctx->P);
  HIP_TRY(launch_max_load(ctx->P, ctx->n_tables, ctx->max_load.get(), nullptr));      // what the run before the snapshot left there
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
    {ctx->tables.get(), table_bytes(ctx, ctx->P.logC)}, {ctx->tvals.get(), ctx->tvals ? tval_bytes(N, ctx->P.logC) : 0},
    {ctx->states.get(), sizeof(ReplicaState) * N}, {ctx->row_reward.get(), rows}, {ctx->row_time.get(), rows}, {ctx->row_steps.get(), rows}, {ctx->row_trial.get(), rows},
    {ctx->trace_state.get(), ctx->trace_state ? trace_words(N) * sizeof(uint32_t) : 0}};
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
