// grlx_evaluate_noisy.hip -- noisy evaluation episodes of the actor-critic (grlx_evaluate_noisy, grlx_evaluate_noisy_trajectory):
// grlx_evaluate's episode for every (replica, start state) pair, acted by the policy that collects the data -- ActionPolicy::act(time, in,
// out) (action.cpp:127-158): the actor's read plus Gaussian or Ornstein-Uhlenbeck noise drawn by Box-Muller from a rand48 stream
// (Rand::getNormal, utils.h:120-125), clipped to the action range -- instead of the noise-free actor.  Every episode carries one rand48
// state (the role of the thread-local stream) and one double (the noise state, ActionPolicy::n_) in and out.
//
// A unit of its own beside grlx_evaluate.hip.  The actor's probe and read, the bookkeeping and the head of a record are
// grlx_episode.h's, which every evaluation unit shares; what is below is this unit's alone: the policy's state, its draw (the
// expression of grlx_rollout_ac.h / grlx_step.h), the store and the record's two last words.
//
// Layout: evaluate_ac_kernel's.  A 16-lane group serves one pair, lane = tiling, four pairs per wave, kQueryWaves waves per block, no wave
// waits for another.  The episode loop is wave-uniform on __ballot(active), bounded by max_steps; finished and dead groups skip loads, LDS
// stores, the draws, the environment step and the sums under ONE predicate; every lane reaches every wave_sync.
//
// Who draws.  evaluate_noisy_kernel: lane 0 of a group ALONE carries the stream, the noise state and the clip counter.  It already forms
// the action alone (the serial sum of the 16 weights) and hands it back through LDS, so the draw -- two logarithm / cosine polynomials and
// a square root -- runs in one lane of sixteen between the two wave_syncs that are there anyway, and the other lanes hold no copy that
// could disagree.  trajectory_noisy_kernel: every lane sums the weights itself, as trajectory_ac_kernel's
// do, because every lane needs the step's words for its part of the record; so every lane carries identical copies of the stream and the
// noise and draws itself, as trajectory_sampled_kernel's lanes do: the same bits in every lane, nothing handed back through LDS.
// `active` is per lane and equal within a group by construction, so no lane draws for a group that another lane thinks finished.
//
// Compiled with -ffp-contract=off like every unit: (1 - theta) * noise + nrm is a product and a sum, ac_decay * sigma a plain product.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate_noisy.h"
#include "grlx_episode.h"

namespace grlx {
namespace noisy {

// what the drawing lane(s) of a group carry through the loop besides the sums
struct Policy {
  uint64_t TL;                  // the episode's rand48 state
  double   noise;               // ActionPolicy::n_
  double   sg, theta;           // the standard deviation of a draw, the Ornstein-Uhlenbeck pull
  int      clipped;
};

// ActionPolicy::act(time, in, out) (action.cpp:127-158) on the actor's read u at model time `time`, in the rollout kernels' order: the
// noise state is reset at time 0; sg != 0: two draws (Rand::getNormal, utils.h:120-125), the noise state moves, out = u + noise; the
// clip.  `clip`: out lay outside the action range.
__device__ __forceinline__ double act(const DevParams &P, Policy &p, double u, double time, bool &clip)
{
  if (time == 0) p.noise = 0;
  double out = u;
  if (p.sg != 0)
  {
    p.TL = lcg_next(p.TL);
    const double U1 = lcg_double(p.TL);
    p.TL = lcg_next(p.TL);
    const double U2 = lcg_double(p.TL);
    const double nrm = __builtin_sqrt(-2 * plog(U1)) * pcos(2 * GRLX_PI * U2) * p.sg + 0.;
    p.noise = (1 - p.theta) * p.noise + nrm;
    out = u + p.noise;
  }
  clip = out < P.action_min || out > P.action_max;
  p.clipped += clip ? 1 : 0;
  return fmin(fmax(out, P.action_min), P.action_max);
}

// the pair's policy state at its episode's start
__device__ __forceinline__ void policy_init(const DevParams &P, const NoisyArgs &T, const ReplicaState &rs, long long pair, bool holds, Policy &p)
{
  p.TL = 0; p.noise = 0; p.clipped = 0;
  // GRLX_SIGMA_OWN: the product the rollout kernels form, on the decay as it stands (never advanced here)
  p.sg = T.sigma < 0. ? rs.ac_decay * P.sigma : T.sigma;
  p.theta = T.theta;
  if (holds)
  {
    uint64_t tl = T.inputs ? T.inputs[(size_t)pair * 2] : kNoisyOwnStream;
    p.TL = (tl >> 48) ? rs.TL : tl;
    p.noise = T.inputs ? __longlong_as_double((long long)T.inputs[(size_t)pair * 2 + 1]) : 0.;
  }
}

template <int S>
__device__ __forceinline__ void store(const NoisyArgs &T, long long pair, const EpisodeSums &e, const Policy &p, const double (&x)[S])
{
  const EvaluateArgs &A = T.e;
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = p.clipped;
  T.streams_out[pair] = p.TL;
  T.noise_out[pair] = p.noise;
#pragma unroll
  for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
}

// Word w of a step's record: record_head's words for the actor-critic -- action index -1, one maximum --, then the noise state after the
// step and the clip flag
template <int D, int S>
__device__ __forceinline__ double record_word(int w, double action, double reward, double value, int code, double noise, bool clip,
                                              const double (&obs)[D], const double (&x)[S])
{
  double out = record_head<D, S>(w, action, reward, value, -1, 1, code, obs, x);
  out = (w == GRLX_TRAJ_OBS + D + S) ? noise : out;
  out = (w == GRLX_TRAJ_OBS + D + S + 1) ? (clip ? 1.0 : 0.0) : out;
  return out;
}

} // namespace noisy

// evaluate_ac_kernel under the exploring policy: lane 0 of a group carries the stream and the noise state and draws between the two
// wave_syncs of the sibling
template <int ENV>
__global__ __launch_bounds__(kQueryWaves * 64) void evaluate_noisy_kernel(DevParams P, NoisyArgs T)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D;
  __shared__ double sh_w[kQueryWaves][64];
  __shared__ double sh_act[kQueryWaves][4];
  const EvaluateArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;                    // dead groups of the last wave neither load nor store nor draw
  double *W = sh_w[wave], *ACT = sh_act[wave];

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 1, r);                 // twin tables: each holds its own keys
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  EpisodeSums e;                                       // ties stays 0: the steps that clipped are the policy's count
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  noisy::Policy p;
  noisy::policy_init(P, T, rs, pair, live && j == 0, p);
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active) actor_probe<ENV>(P, tab, rs, obs, j, lane, W);
    wave_sync();
    if (active && j == 0)
    { // the draws sit under the step's predicate: a finished group's stream and noise stand where its last step left them
      bool clip;
      ACT[g] = noisy::act(P, p, read_actor(P, W, g), x[S - 1], clip);
    }
    wave_sync();
    if (active)
    {
      const double action = ACT[g];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, gamma, terminal, status, false);
    }
  }
  if (live && j == 0) noisy::store<S>(T, pair, e, p, x);
}

// trajectory_ac_kernel under the exploring policy: every lane sums the weights, carries the stream and the noise state and draws itself;
// lane j stores word j of the step's record, and word j + 16 where the record has one
template <int ENV>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_noisy_kernel(DevParams P, NoisyArgs T)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, R = GRLX_TRAJ_OBS + D + S + 2;
  static_assert(R <= 32, "a record is stored by 16 lanes in two rounds");
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
  const Table tab = table_of(P, 1, r);
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  double *rec = T.records + (live ? (size_t)pair * (size_t)A.max_steps * R : 0);     // 64-bit: see trajectory_q_kernel
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);

  EpisodeSums e;                                       // ties stays 0: the steps that clipped are the policy's count
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  noisy::Policy p;
  noisy::policy_init(P, T, rs, pair, live, p);
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active) actor_probe<ENV>(P, tab, rs, obs, j, lane, W);
    wave_sync();
    if (active)
    {
      const double value = read_actor(P, W, g);
      bool clip;
      const double action = noisy::act(P, p, value, x[S - 1], clip);
      double before[D];
#pragma unroll
      for (int i = 0; i < D; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, gamma, terminal, status, false);
      double *at = rec + (size_t)(e.steps - 1) * R;
      if (j < R) at[j] = noisy::record_word<D, S>(j, action, reward, value, e.code, p.noise, clip, before, x);
      if constexpr (R > 16)
        if (j + 16 < R) at[j + 16] = noisy::record_word<D, S>(j + 16, action, reward, value, e.code, p.noise, clip, before, x);
    }
    wave_sync();                                       // the sums above are read before the next step's weights are written
  }
  if (live && j == 0) noisy::store<S>(T, pair, e, p, x);
}

int noisy_trajectory_words(int env)
{
  const int words = trajectory_words(env, false);
  return words ? words + 2 : 0;
}

// launch_evaluate's grid.  Every output pointer of the kernels is written without a test, so all of them are required here.
static hipError_t launch_noisy(const DevParams &P, const NoisyArgs &A, bool rec, hipStream_t stream)
{
  const unsigned blocks = pair_blocks(A.e);
  if (blocks == 0) return hipSuccess;
  if (P.agent != GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.e.max_steps < 1 || (rec && !A.records) ||
      !A.streams_out || !A.noise_out || !A.e.ret || !A.e.disc || !A.e.steps || !A.e.terminal || !A.e.ties || !A.e.final_state || !A.e.states)
    return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kQueryWaves * 64);
  with_ac_instance(P, [&](auto env) {
    constexpr int ENV = decltype(env)::value;
    if (rec) hipLaunchKernelGGL(trajectory_noisy_kernel<ENV>, grid, block, 0, stream, P, A);
    else hipLaunchKernelGGL(evaluate_noisy_kernel<ENV>, grid, block, 0, stream, P, A);
  });
  return hipGetLastError();
}

hipError_t launch_evaluate_noisy(const DevParams &P, const NoisyArgs &A, hipStream_t stream) { return launch_noisy(P, A, false, stream); }
hipError_t launch_trajectory_noisy(const DevParams &P, const NoisyArgs &A, hipStream_t stream) { return launch_noisy(P, A, true, stream); }

} // namespace grlx
