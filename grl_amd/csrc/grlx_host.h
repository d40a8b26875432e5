// grlx_host.h -- what the units of the C ABI (grlx_api_*.cpp) share: the context, the error and device-memory helpers, and the
// declarations of the helpers that cross unit boundaries.  Host code only: no .hip file includes it.
//
// Ownership: every device pointer, stream and event of the context is an owner (Dev, DevStream, DevEvent below) and is released with the
// context; nothing frees by hand.  The parameter block the kernels read (grlx_ctx::P) gets the context's pointers from bind_params alone.
// Validation (grl's bad_param conditions become GRLX_ERR_INVALID with a message), the reference's instantiate-order RNG seeding, device
// memory management and kernel launches.  No compute happens on the host: without a HIP device every compute entry point fails.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>
#include "grlx_internal.h"
#include "grlx_host_rules.h"
#include "../../include/grlx_diag.h"

using namespace grlx;

namespace grlx {
int fail(int code, const char *fmt, ...);                  // sets the thread's message (grlx_last_error), returns `code`
void set_last_error(const char *msg);                      // other translation units of the library (grlx_fqi.hip)
void set_fqi_query_chunk_bytes(uint64_t bytes);            // grlx_fqi.hip: the staging bound of grlx_fqi_query
bool have_device();
static_assert(sizeof(Entry) == kRuleEntryBytes && 16 * kMaxTrace * 2 == kRuleTraceWords, "grlx_host_rules.h: kRuleEntryBytes, kRuleTraceWords");
}
#define HIP_TRY(expr)                                                                   \
  do { const hipError_t e__ = (expr); if (e__ != hipSuccess) return fail(GRLX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); } while (0)

namespace grlx {
// Move-only owners: of a stream or an event, and (Dev) of one device allocation.  Moving in releases what was held before.
template <typename H, hipError_t (*Release)(H)>
struct Owner {
  Owner() = default;
  Owner(Owner &&o) noexcept : h(o.h) { o.h = nullptr; }
  Owner &operator=(Owner &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
  ~Owner() { reset(); }
  void reset() { if (h) (void)Release(h); h = nullptr; }
  explicit operator bool() const { return h != nullptr; }
protected:
  H h = nullptr;
};
template <typename T>
struct Dev : Owner<void *, hipFree> {
  hipError_t alloc(size_t bytes) { reset(); return hipMalloc(&h, bytes ? bytes : 8); }
  hipError_t upload(const void *src, size_t bytes) { const hipError_t e = alloc(bytes); return e != hipSuccess ? e : hipMemcpy(h, src, bytes, hipMemcpyHostToDevice); }
  T *get() const { return (T *)h; }
  template <typename U> U *as() const { return (U *)h; }
};
using DevBuf = Dev<void>;          // the staging arrays of the copy-in / copy-out entry points
struct DevStream : Owner<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&h, flags); }
  hipStream_t get() const { return h; }
};
struct DevEvent : Owner<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&h, flags); }
  hipEvent_t get() const { return h; }
};
struct PinnedBuf : Owner<void *, hipHostFree> {      // page-locked host memory: the target of an asynchronous copy
  hipError_t alloc(size_t bytes) { reset(); return hipHostMalloc(&h, bytes ? bytes : 8, hipHostMallocDefault); }
  char *get() const { return (char *)h; }
};

// One of the two staging slots of grlx_evaluate_trajectory_stream (grlx_api_read.cpp): a chunk's device arrays (the start states in, then
// the outputs in the chunk's layout), the pinned copy of the outputs, the stream the chunk runs on, the event behind its last copy, and
// the two events around its kernel (grlx_read_kernel_timing).  Made at the first streamed call, grown when a call needs more, released
// with the context.
struct StreamSlot {
  DevBuf    dev;
  PinnedBuf pinned;
  size_t    dev_bytes = 0, pinned_bytes = 0;
  DevStream stream;
  DevEvent  done, k0, k1;
};
} // namespace grlx

struct grlx_ctx {
  grlx_config cfg;
  DevParams   P;
  int         S, D;
  Dev<Entry>        tables;
  Dev<ReplicaState> states;
  Dev<double>       row_reward, row_time;
  Dev<int64_t>      row_steps, row_trial;
  Dev<grlx_tap>     taps;
  Dev<uint32_t>     tap_count;
  Dev<uint64_t>     scratch;     // 8 x u64
  Dev<uint32_t>     queue;       // work queue of the wide actor-critic kernel: next unstarted replica
  Dev<uint32_t>     max_load;    // fullest table of the context after the last grlx_run (max_load_kernel)
  uint32_t     logC_max = 26;             // growth bound of the sparse tables
  Dev<unsigned long long> diag;
  Dev<uint32_t>     trace_state;
  Dev<double>       tvals;       // target network values per table position (target_interval > 0)
  // loaded policy images (grlx_load_weights): image k serves the replicas r with image_of[table][r] == k;
  // an image no replica refers to any more is freed at the next load, the rest with the context
  std::vector<Dev<double>> images;
  std::vector<int>      image_of[2];
  std::vector<Dev<double>> target_images;    // per replica: the target network's dense vector after a load with tau != 0 (ReplicaState::target_base)
  hipStream_t  run_stream = nullptr;      // stream of the last grlx_run / grlx_curve_stats: the caller's, not owned
  bool         run_pending = false;       // ... with work possibly still in flight on it
  int          n_tables = 1;
  int64_t      trials_run = 0;
  const KernelRow *last_row = nullptr;    // the row of the kernel table launched last
  bool         poison = false;            // GRLX_POISON_REGISTERS=<pattern>: diagnostic, see launch_poison_registers
  uint32_t     poison_pattern = 0;
  // the environment server of the pendulum rollout kernels (grlx_env_server.h): mailboxes, its stream, and the fork / join events
  int          env_server = 1;            // GRLX_ENV_SERVER=0 turns it off
  Dev<void>    park;                      // 32-replica waves of the compass walker: parked lane state of the sub-batches beyond the third, per wave
  Dev<EnvMail> env_mail;
  size_t       env_mail_bytes = 0;        // per replica: kEnvMailBytes (pendulum kernels) or kWideMailBytes (wide kernels)
  DevStream    srv_stream;
  DevEvent     srv_go, srv_done;
  // per-step entry points (grlx_env_start / _advance, grlx_agent_start / _step / _end): agent state between calls and the staging
  // buffers of their host arguments, created at the first such call
  Dev<AgentRep> agent_rep;
  Dev<uint32_t> agent_lane;
  Dev<double>  stage_f64;                 // [N][GRLX_MAX_DIMS] obs | [N] reward | [N] action
  Dev<int32_t> stage_i32;                 // [N] active | [N] terminal
  uint64_t     step_calls = 0;            // agent calls since the last look at the tables' load
  // hyper-parameter sweep (grlx_set_replica_params): the per-replica values as given ([GRLX_PARAM_*][replica]; empty = none set: not a
  // sweep context) and their device records, handed to the SpecSweep rows once the context is a sweep context
  std::vector<double> sweep_host[4];
  Dev<SweepParams> sweep_dev;
  bool         sweep = false;
  // A context WITHOUT a trace (GRLX_TRACE_NONE).  The deferred update stores p's weight straight into the table, behind the loads of the
  // next step's weights that are already in flight, and no trace entry forwards it to them (p of consecutive steps is often the same
  // slot); only the instantiations that load again after such an update, or that update in place, equal the reference there:
  //   no_trace_td: SARSA / Q / Expected SARSA without target network and claim table run the sweep kernels on records that all hold the
  //                configuration's values (sweep_dev, made at create): at most 8 replicas per wave, no environment server
  //   no_trace_ac: the actor-critic runs the instantiation that updates the critic in place: 4 replicas per wave
  // (QV, advantage learning, target networks, the claim table and the per-step entries update in place anyway.)
  bool         no_trace_td = false, no_trace_ac = false;
  double       snap_pack_ms = -1, snap_unpack_ms = -1;   // diagnostic: device time of the snapshot kernels in the last save / load
  bool         launched = false;          // a rollout or per-step kernel has run in this context: its replicas' parameters are fixed
  // grlx_evaluate_trajectory_stream: its two slots, and whether a call is between its first launch and its return -- that is, whether the
  // caller's sink may be running (STREAM_REFUSES, drain)
  StreamSlot   stream_slot[2];
  bool         streaming = false;
};

// Wait for the rollouts of the last grlx_run (grlx_api_context.cpp).  Every entry point that reads or writes the context's device memory
// outside a rollout passes here, so this is also where a call made from inside a streamed call's sink is refused.
namespace grlx { int drain(grlx_ctx *ctx); }
#define DRAIN(ctx) do { int rc__ = drain(ctx); if (rc__ != GRLX_OK) return rc__; } while (0)
// ... and the entry points that change the context without (or before) passing DRAIN say it themselves
#define STREAM_REFUSES(ctx, who)                                                                                                  \
  do { if ((ctx) && (ctx)->streaming) return fail(GRLX_ERR_INVALID, who ": a streamed call is in progress on this context (grlx_evaluate_trajectory_stream has not returned)"); } while (0)
#define SWEEP_REFUSES(ctx, what)                                                                                                  \
  do { if ((ctx) && (ctx)->sweep) return fail(GRLX_ERR_INVALID, what " is not built for a sweep context (grlx_set_replica_params): it would run on the shared values"); } while (0)

namespace grlx {
// grlx_api_config.cpp
int env_dims(int env, int *S, int *D);
int make_tile_params(const grlx_tile_spec &ts, TileParams *tp);
int make_params(const grlx_config &c, DevParams *P);
int admit(const grlx_config *cfg, DevParams *P);
// grlx_api_context.cpp
void bind_params(const grlx_ctx *ctx, uint32_t logC, DevParams *P);
int grow_tables(grlx_ctx *ctx, uint32_t new_logC);
int grow_if_loaded(grlx_ctx *ctx, uint32_t used);
hipError_t upload_empty_trace(uint32_t *dst, size_t N);
// grlx_api_run.cpp
int status_to_error(uint64_t st);
int sweep_record(const grlx_config &c, size_t r, double alpha, double gamma, double lambda, double epsilon, int param, SweepParams *w);
int sweep_admits(const grlx_config &c, const DevParams &P);
void sweep_limits_layout(DevParams &P);

inline size_t table_bytes(const grlx_ctx *ctx, uint32_t logC) { return table_bytes((size_t)ctx->P.n_replicas, (size_t)ctx->n_tables, logC); }
// one replica's state as the device holds it (the caller has drained)
inline hipError_t read_state(const grlx_ctx *ctx, int replica, ReplicaState *s)
{
  return hipMemcpy(s, ctx->states.get() + replica, sizeof(*s), hipMemcpyDeviceToHost);
}
}
