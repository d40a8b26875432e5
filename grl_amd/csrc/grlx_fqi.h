// grlx_fqi.h -- the batch path (grlx_fqi_*): what grlx_api_fqi.cpp hands to the kernels of grlx_fqi.hip.  Included by those two only.
#pragma once
#include "grlx_internal.h"

namespace grlx {

constexpr int kFqiNIn = 3;                 // task/pendulum/swingup: observation (2) ++ action (1)
constexpr int kFqiD = 2;
constexpr int kFqiS = 3;

struct FqiRep {                            // per-replica state between launches
  uint64_t G, TL;                          // global / thread-local streams (fqi.c: orc_fqi_create)
  int64_t  n;                              // transitions stored
  int64_t  batches_done;
  unsigned long long maxdelta_bits;        // max |target - previous target| of the running iteration (non-negative double)
  double   maxdelta_last;
  int32_t  done;                           // the rebuild's iteration loop has ended (maxdelta <= 0.001)
  int32_t  iterations;                     // iterations executed by the last rebuild
  uint32_t status;
  uint32_t rows;
  double   last_error;
};

struct FqiParams {
  DevParams env;                           // h, integration_steps, timeout, randomization of the pendulum
  int32_t  R, H, P, A, batch_size, cap, chunks_cap;
  double   actions[kMaxActions];
  double   in_min[kFqiNIn], in_scale[kFqiNIn], obs_min[kFqiD], obs_range[kFqiD];
  double   action_min, action_range;
  double   gamma_tau;
  double   eta;                                     // representation/parameterized/ann:eta (0: RPROP, > 0: gradient descent, < 0: RMSprop)
  FqiRep  *rep;
  double  *in, *next_obs, *reward, *targets;        // [R][cap][...]
  int32_t *absorbing;
  double  *net;                                     // [R][4][P]: params, eta, Delta (unused), prev_Delta
  double  *vL;                                      // [2][R][P + 1][64]: the 64 partial sums of level 2 per parameter, double-buffered by epoch parity
  unsigned long long *stamps;                       // diagnostic (GRLX_FQI_STAMPS=1): [R][16][4 epochs][8] shader-clock stamps, else null
  unsigned int *sync;                               // [R][4]: arrival counter of the replica's blocks (16-byte slots), zeroed per launch
  double  *row_reward;                              // [R][max_rows]
  int64_t *row_batch, *row_transitions;
  int32_t  max_rows;
};

constexpr uint32_t ST_SYNC_TIMEOUT = 32u;
constexpr int kFqiStampBlocks = 16;

constexpr int kFqiTrajWords = GRLX_TRAJ_OBS + kFqiD + kFqiS;
constexpr int kFqiEvalDomain = 3;          // terminal code of a step that ended outside Env<PENDULUM>::in_domain (grlx_evaluate's)

struct FqiEvalArgs {
  int32_t first_replica, n_starts, max_steps;      // n_starts: of this chunk; max_steps: 1 ... GRLX_MAX_EPISODE_STEPS
  const double *states;                            // [n_starts][3]
  double  *ret, *disc;                             // [n_replicas][n_starts], as are steps, terminal and ties
  int32_t *steps, *terminal, *ties;
  double  *final_state;                            // [n_replicas][n_starts][3]
  double  *records;                                // RECORD: [n_replicas][n_starts][max_steps][kFqiTrajWords]
};

constexpr int kFqiEnsTrajWords = GRLX_TRAJ_ENS_OBS + kFqiD + kFqiS;

struct FqiEnsArgs {
  int32_t first_replica, group_size, rule, n_starts, max_steps;      // n_starts: of this chunk; max_steps: 1 ... GRLX_MAX_EPISODE_STEPS
  const double *states;                            // [n_starts][3]
  double  *ret, *disc;                             // [groups][n_starts], as are steps, terminal, ties, member_ties and agreement
  int32_t *steps, *terminal, *ties;
  int64_t *member_ties, *agreement;
  double  *final_state;                            // [groups][n_starts][3]
  double  *records;                                // RECORD: [groups][n_starts][max_steps][kFqiEnsTrajWords]
};

// ---- the sampled episodes (grlx_fqi_evaluate_sampled, grlx_fqi_evaluate_ensemble_sampled): the greedy calls' arguments, the sampler,
// and the rand48 words every episode carries in and out
constexpr int kFqiSampledTrajWords = kFqiTrajWords + 1;              // ... then `explored`
constexpr int kFqiEnsSampledTrajWords = kFqiEnsTrajWords + 2;        // ... then `explored`, `prob`

struct FqiSampledArgs {
  FqiEvalArgs e;                                   // e.records: [n_replicas][n_starts][max_steps][kFqiSampledTrajWords]
  int32_t sampler;                                 // GRLX_SAMPLER_*
  double  epsilon;                                 // [0, 1]
  const uint64_t *streams;                         // [n_replicas][n_starts][2]: {sampler's, global}; null: {0, the replica's G}
  int32_t  *explored;                              // [n_replicas][n_starts]
  uint64_t *streams_out;                           // [n_replicas][n_starts][2]
};

struct FqiEnsSampledArgs {
  FqiEnsArgs e;                                    // e.rule: GRLX_ENSEMBLE_MAJORITY / _RANK; e.records: [...][kFqiEnsSampledTrajWords]
  double  tau;                                     // the combined softmax's temperature, > 0
  int32_t member;                                  // GRLX_MEMBER_*
  double  member_param;                            // e in [0, 1] (EPSILON), tau_m > 0 (SOFTMAX)
  const uint64_t *streams;                         // [groups][n_starts]; null: G of the group's first replica
  int32_t  *explored;                              // [groups][n_starts]
  uint64_t *streams_out;                           // [groups][n_starts]
};

// How a context launches the epochs kernel: FqiShape<hidden>'s blocks per replica and threads per block, how many replicas' blocks are
// resident at once, and whether the launch is plain -- GRLX_FQI_NO_COOP=1 (diagnostic), or the runtime refused the cooperative launch
// because another process holds the device's cooperative queue (launch_fqi_batch sets it then)
struct FqiLaunchPlan {
  int  replicas_per_launch = 1;
  int  blocks_per_replica = 16, block_threads = 256;
  bool plain_launch = false;
};

// the launchers of grlx_fqi.hip; every pointer is a device pointer.  A hidden width that is not built is hipErrorInvalidValue.
bool fqi_width_built(int H);             // the instantiated widths of the hidden layer (representation/parameterized/ann:hiddens = [H])
// the plan's shape, and how many blocks of the epochs kernel one CU holds
hipError_t fqi_epochs_shape(int H, FqiLaunchPlan *plan, int *blocks_per_cu);
hipError_t launch_fqi_init(const FqiParams &F, const uint64_t *r0, hipStream_t stream);
// one batch: generate, rebuild (iterations x (targets + epochs)), the test trial; batches_run: those before this one
hipError_t launch_fqi_batch(const FqiParams &F, FqiLaunchPlan &plan, int batches_run, int iterations, int epochs, hipStream_t stream);
hipError_t launch_fqi_query(const FqiParams &F, int first_replica, int n_replicas, const double *obs, int n_obs, double *q, hipStream_t stream);
// the episodes of a chunk for `rows` replicas (groups); A.records null: the sums alone
hipError_t launch_fqi_evaluate(const FqiParams &F, const FqiEvalArgs &A, int rows, hipStream_t stream);
hipError_t launch_fqi_evaluate_ensemble(const FqiParams &F, const FqiEnsArgs &A, int rows, hipStream_t stream);
// the sampled episodes; every output pointer is written without a test
hipError_t launch_fqi_evaluate_sampled(const FqiParams &F, const FqiSampledArgs &A, int rows, hipStream_t stream);
hipError_t launch_fqi_evaluate_ensemble_sampled(const FqiParams &F, const FqiEnsSampledArgs &A, int rows, hipStream_t stream);
hipError_t launch_fqi_query_ensemble(const FqiParams &F, int first_replica, int groups, int group_size, const double *obs, int n_obs, double *out,
                                     hipStream_t stream);

} // namespace grlx
