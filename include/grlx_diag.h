/* grlx_diag.h -- diagnostic exports of libgrlx.so: not part of the drop-in boundary (include/grlx.h), kept stable only for the
 * repository's own tools, tests and bench.py.  Every symbol the library exports is declared in one of the two headers
 * (tests/test_capi_symbols.py checks exported == declared). */
#ifndef GRLX_DIAG_H_
#define GRLX_DIAG_H_

#include "grlx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The environment server of the pendulum rollout kernels (grl_amd/csrc/grlx_env_server.h): in the last launch of the context that had
 * it, how many replicas took every environment step from it and how many gave up waiting and integrated themselves; both 0 when no
 * launch of this context had it. */
int grlx_env_server_counts(grlx_ctx *ctx, int *served, int *fell_back);
/* The wave-uniform pass of rollout_served_kernel (grl_amd/csrc/grlx_rollout.h): out[r], r < min(count, replicas), = the passes the wave of
 * replica r took in that loop in the last launch of the context that had the environment server (the four replicas of a wave report the
 * same number; a ragged wave, a wave without the server and the wide kernels report 0); the rest of out, and all of it when no launch of
 * this context had the server, is 0. */
int grlx_uniform_pass_counts(grlx_ctx *ctx, unsigned long long *out, int count);
/* Which replicas grlx_env_server_counts counted: out[r], r < min(count, replicas), = 1 when replica r was served to the end of the last
 * launch of the context that had the environment server, 2 when it fell back to integrating itself; the rest of out, and all of it when
 * no launch of this context had the server, is 0. */
int grlx_env_server_flags(grlx_ctx *ctx, int32_t *out, int count);
/* The raw mailboxes of the environment server after the last launch (1 KB per replica; GRLX_ENV_SERVER_STATS builds leave cycle counts
 * in them): at most `bytes` bytes to `out`. */
int grlx_env_server_debug(grlx_ctx *ctx, void *out, size_t bytes);
/* Shader-clock stamps of the LAST fqi_epochs_kernel launch (GRLX_FQI_STAMPS=1 at grlx_fqi_create): count = n_replicas * 16 * 4 * 8. */
int grlx_fqi_debug_stamps(grlx_fqi_ctx *ctx, unsigned long long *out, int count);

/* Which kernel runs.  Every rollout instantiation is one row of the kernel table (grl_amd/csrc/grlx_kernel_table.h); a row's name is the
 * instantiation as spelled there, e.g. "rollout_wide_kernel<GRLX_ENV_ACROBOT, 3, 4, SpecAcrobotQ>".
 * grlx_last_kernel_name: the row the context launched last ("" before the first launch).
 * grlx_kernel_plan: what a context of this configuration would launch on a device of `simds` SIMDs, WITHOUT a device: the validation of
 * grlx_create (its error codes and messages), the layout choice and the plan of one launch.  Out (each optional): the replicas per wave,
 * the GRLX_KERNEL_* variant, the grid, the rollout row's name and the server row's name ("" when the launch has no environment server),
 * each name truncated to name_cap bytes. */
#define GRLX_PLAN_STAMPS_IN_PLACE 1   /* as after grlx_set_diag(ctx, 1) */
#define GRLX_PLAN_STAMPS_DEFERRED 2   /* as after grlx_set_diag(ctx, 2) */
#define GRLX_PLAN_SWEEP           4   /* as after grlx_set_replica_params */
#define GRLX_PLAN_SERVER_OFF      8   /* GRLX_ENV_SERVER=0 */
#define GRLX_PLAN_WALKER_SERVER  16   /* GRLX_ENV_SERVER_WALKER=1 */
#define GRLX_PLAN_FITS_YES       32   /* a rollout wave and its server wave fit one SIMD: yes / no; neither flag: ask the runtime */
#define GRLX_PLAN_FITS_NO        64
const char *grlx_last_kernel_name(grlx_ctx *ctx);
int grlx_kernel_plan(const grlx_config *cfg, int simds, int flags, int *replicas_per_wave, int *variant, int *grid, char *rollout_name,
                     char *server_name, size_t name_cap);


/* Snapshots (grlx_snapshot_save / _load), for tools/snapshot_throughput.py.
 * grlx_snapshot_timing: milliseconds (events on the device) that snapshot_pack_kernel took in the context's last grlx_snapshot_save and
 * snapshot_unpack_kernel in its grlx_snapshot_load; negative where none has run.
 * grlx_snapshot_naive_copy: the naive snapshot as a baseline -- hipMemcpy of the context's OWN raw arrays (tables, target values, states,
 * rows, trace) to one freshly allocated pageable host buffer of their total size and back again (the context is left as it was): the
 * bytes and the milliseconds of both directions.  GRLX_ERR_OOM when the host has no such buffer. */
int grlx_snapshot_timing(grlx_ctx *ctx, double *pack_ms, double *unpack_ms);
int grlx_snapshot_naive_copy(grlx_ctx *ctx, uint64_t *bytes, double *out_ms, double *back_ms);

/* Policy queries (grlx_query_q / _state / _ensemble, grlx_fqi_query): the bound on the device scratch one call holds, process-wide; 0 = the default,
 * 256 MiB.  A chunk never has less than one observation.  For tests: a small value forces several chunks at a small shape. */
int grlx_set_query_chunk_bytes(uint64_t bytes);
/* The device time of the reads' kernels, for tools/trajectory_throughput.py.  enable != 0: from now on every chunk of every query,
 * evaluation and trajectory call is timed by events around its launches (a trajectory chunk: the zero fill of its records and the kernel),
 * each waited for before the chunk's outputs are copied; the sums start at zero.  enable == 0: timing off.  Either way *ms (may be NULL)
 * receives the milliseconds and *chunks (may be NULL) the number of chunks timed since the last enabling call.  Process-wide, off by default. */
int grlx_read_kernel_timing(int enable, double *ms, int *chunks);

#ifdef __cplusplus
}
#endif
#endif /* GRLX_DIAG_H_ */
