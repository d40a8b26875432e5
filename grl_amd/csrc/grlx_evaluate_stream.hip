// grlx_evaluate_stream.hip -- the kernels of grlx_evaluate_trajectory_stream: trajectory_q_kernel and trajectory_ac_kernel
// (grlx_evaluate.hip) with the zero fill of the records done by the kernel itself, so that the host stages chunk after chunk through
// buffers it never clears.  A unit of its own beside grlx_evaluate.hip, whose kernels stay what they are: the loop is restated here, not
// shared through a template flag (a flag on trajectory_q_kernel would make it another kernel for the compiler).
//
// The episodes, the record words and the sums are the sibling's, bit for bit: the same probe (member_probe / actor_probe), the same
// findmax, env_step, episode_account and record_store16 (grlx_episode.h), in the same order, in the same layout -- a 16-lane group per
// (replica, start state) pair, four groups per wave, kQueryWaves waves per block, no wave waits for another.  trajectory_ac_kernel
// carries actor_probe's and read_actor's lines itself for the sake of its own machine code; a new kernel has none to keep and calls them:
// the same operations in the same order.
//
// The new part is the tail.  After the loop every live group writes +0.0 to the words [steps * R, max_steps * R) of its own episode,
// lane j the words j, j + 16, ... behind the end: 16 lanes on 16 consecutive doubles, one 128-byte run per group and store.  The groups
// of a wave end at different steps, so this loop is divergent by design: a wave runs it as often as its longest tail needs.  An episode
// that ran to max_steps has no tail, a dead group stores nothing.  Every word of a live pair's column is therefore written exactly once
// per launch -- by record_store16 up to the episode's end, by the tail behind it -- and what the buffer held before does not matter.
// Indices are 64-bit, as in the sibling: pairs * max_steps * R * 8 bytes pass 2^32 at a million pairs of 100 steps.
//
// Compiled with -ffp-contract=off like every unit.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate_stream.h"
#include "grlx_episode.h"
#include "grlx_host_rules.h"

namespace grlx {

static_assert(4 * kQueryWaves == kRulePairsPerBlock, "grlx_host_rules.h: kRulePairsPerBlock is pair_blocks' pairs per block");

// +0.0 behind the end of the group's episode: words [steps * R, max_steps * R) of rec, lane j every 16th from steps * R + j
template <int R>
__device__ __forceinline__ void tail_zero16(double *rec, int j, int steps, int max_steps)
{
  const size_t end = (size_t)max_steps * R;
  for (size_t w = (size_t)steps * R + (size_t)j; w < end; w += 16) rec[w] = 0.;
}

// trajectory_q_kernel's loop, then the tail
template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_stream_q_kernel(DevParams P, TrajectoryArgs T)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, R = GRLX_TRAJ_OBS + D + S;
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_q[kQueryWaves][4 * 8];
  const EvaluateArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;                    // dead groups of the last wave neither load nor store
  double *W = sh_w[wave], *Q = sh_q[wave];

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 0, r);
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  double *rec = T.records + (live ? (size_t)pair * (size_t)A.max_steps * R : 0);
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active) member_probe<ENV, NA>(P, tab, rs, obs, j, lane, W);
    wave_sync();
    if (active && j < NA) Q[g * 8 + j] = member_q(P, W, g, j);
    wave_sync();
    if (active)
    {
      double q[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) q[a] = Q[g * 8 + a];
      int mai, man;
      findmax<NA>(q, mai, man);
      const double action = action_of<NA>(P, mai);
      double value = q[0];
#pragma unroll
      for (int a = 1; a < NA; ++a) value = (mai == a) ? q[a] : value;
      double before[D];
#pragma unroll
      for (int i = 0; i < D; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, gamma, terminal, status, man > 1);
      record_store16<D, S>(rec + (size_t)(e.steps - 1) * R, j, action, reward, value, mai, man, e.code, before, x);
    }
  }
  if (live) tail_zero16<R>(rec, j, e.steps, A.max_steps);
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// trajectory_ac_kernel's loop, then the tail
template <int ENV>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_stream_ac_kernel(DevParams P, TrajectoryArgs T)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, R = GRLX_TRAJ_OBS + D + S;
  __shared__ double sh_w[kQueryWaves][64];
  const EvaluateArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;
  double *W = sh_w[wave];

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 1, r);                 // twin tables: each holds its own keys
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  double *rec = T.records + (live ? (size_t)pair * (size_t)A.max_steps * R : 0);
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;
    if (active) actor_probe<ENV>(P, tab, rs, obs, j, lane, W);
    wave_sync();
    if (active)
    { // ActionPolicy::read (action.cpp:99-112) over LinearRepresentation::read, then the clip of act; every lane sums for itself
      const double value = read_actor(P, W, g);
      const double action = query_clamp(value, P.action_min, P.action_max);
      double before[D];
#pragma unroll
      for (int i = 0; i < D; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, gamma, terminal, status, false);
      record_store16<D, S>(rec + (size_t)(e.steps - 1) * R, j, action, reward, value, -1, 1, e.code, before, x);
    }
    wave_sync();                                       // the sums above are read before the next step's weights are written
  }
  if (live) tail_zero16<R>(rec, j, e.steps, A.max_steps);
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// launch_trajectory's grid and checks; the records are written whole by the kernel
hipError_t launch_trajectory_stream(const DevParams &P, const TrajectoryArgs &A, hipStream_t stream)
{
  const unsigned blocks = pair_blocks(A.e);
  if (blocks == 0) return hipSuccess;
  if (!evaluate_built(P.agent, P.env, P.A) || A.e.max_steps < 1 || !A.records) return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kQueryWaves * 64);
  if (P.agent == GRLX_AGENT_AC)
    with_ac_instance(P, [&](auto env) { hipLaunchKernelGGL(trajectory_stream_ac_kernel<decltype(env)::value>, grid, block, 0, stream, P, A); });
  else
    with_q_instance(P, [&](auto env, auto na) {
      hipLaunchKernelGGL((trajectory_stream_q_kernel<decltype(env)::value, decltype(na)::value>), grid, block, 0, stream, P, A);
    });
  return hipGetLastError();
}

} // namespace grlx
