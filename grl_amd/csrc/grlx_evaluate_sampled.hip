// grlx_evaluate_sampled.hip -- sampled evaluation episodes (grlx_evaluate_sampled, grlx_evaluate_sampled_trajectory): grlx_evaluate's
// episode for every (replica, start state) pair, acted by the reference's SAMPLERS instead of the first maximum -- the greedy sampler with
// its drawn tie break (GreedySampler::sample, greedy.cpp:63-86) or the epsilon-greedy one (EpsilonGreedySampler::sample, greedy.cpp:144-218)
// -- on two rand48 streams that every episode carries.  The order of draws is eps_greedy_act's (grlx_policy.h), which only the rollout
// kernels call: the epsilon draw from the sampler's stream, then the global stream for the random action or for the tie break.
//
// A unit of its own beside grlx_evaluate.hip.  The probe, the read and the head of a record are grlx_episode.h's, which every evaluation
// unit shares; what is below is this unit's alone: the sampler, the record's last word, and what an episode carries and stores -- the
// bookkeeping mirrors episode_account inline, see Sums.
//
// Layout: evaluate_q_kernel's.  A 16-lane group serves one pair, lane = tiling, four pairs per wave, kQueryWaves waves per block, no wave
// waits for another.  The episode loop is wave-uniform on __ballot(active), bounded by max_steps; finished and dead groups skip loads, LDS
// stores, the draws, the environment step and the sums under ONE predicate; every lane reaches every wave_sync.
//
// Who carries the streams: ALL 16 lanes of a group, in identical copies (two 64-bit registers each).  After the Q-values are in LDS every
// lane reads them (broadcast), runs findmax and the sampler itself, as trajectory_q_kernel's lanes run findmax: the same bits in every
// lane, nothing is handed back through LDS, and no lane can draw for a group that another lane thinks finished -- `active` is per lane and
// equal within a group by construction.  A draw is a 64-bit multiply-add masked to 48 bits (lcg_next); the integers come from lcg_long
// (an unsigned 31-bit value, unsigned modulo), epsilon's comparison from lcg_double.  Lane 0 writes the pair's outputs and both streams
// once, after the loop.
//
// The tie-break walk and Q of the action taken are selects over the NA Q-values (registers): no dynamically indexed array, no scratch.
//
// Compiled with -ffp-contract=off like every unit: eps_decay * epsilon is the plain product the rollout kernels form.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate_sampled.h"
#include "grlx_episode.h"

namespace grlx {
namespace sampled {

// what a group carries through the loop besides the model state: EpisodeSums' fields (grlx_episode.h), the random actions taken and both
// streams, in a struct of this unit's.  Deriving it from EpisodeSums, or carrying the extras in a struct beside one, so that the loop
// could call episode_account and the end episode_store, changed the machine code (the first: two moves of the walker's kernel swap
// places; the second: every kernel of the unit), so the loop keeps the bookkeeping inline and the end its own store.
struct Sums {
  double ret, disc, g;
  int steps, code, ties, explored;
  uint64_t S, G;                // the sampler's private stream, the global stream
};

// One action of the sampler over q (eps_greedy_act's order of draws, grlx_policy.h); returns the index that acts.
//   epsilon-greedy: S advances, rnd = drand48; rnd < e: G advances, lrand48 % NA acts, `explored`.
//   otherwise, and the greedy sampler: man > 1: G advances, the (lrand48 % man + 1)-th maximal entry acts, `tie`; else mai, no draw.
template <int NA>
__device__ __forceinline__ int sample(const double (&q)[NA], int sampler, double e, uint64_t &S, uint64_t &G, int &man, bool &tie, bool &explored)
{
  int mai = 0;
  man = 1;
  double best = q[0];
#pragma unroll
  for (int a = 1; a < NA; ++a)
  { // greedy.cpp:47-61
    if (q[a] > best) { best = q[a]; mai = a; man = 1; }
    else if (q[a] == best) man++;
  }
  tie = false;
  explored = false;
  if (sampler == GRLX_SAMPLER_EPSILON_GREEDY)
  {
    S = lcg_next(S);
    if (lcg_double(S) < e)
    {
      G = lcg_next(G);
      explored = true;
      return (int)(lcg_long(G) % (uint32_t)NA);
    }
  }
  if (man > 1)
  { // greedy.cpp:77-85, by selects: the entry at which the countdown over the maximal entries stands at zero
    G = lcg_next(G);
    int jj = (int)(lcg_long(G) % (uint32_t)man);
    int res = 0;
#pragma unroll
    for (int a = 0; a < NA; ++a)
    {
      const bool m = q[a] == best;
      res = (m && jj == 0) ? a : res;
      jj -= m ? 1 : 0;
    }
    tie = true;
    return res;
  }
  return mai;
}

// Word w of a step's record: record_head's words, then `explored`
template <int D, int S>
__device__ __forceinline__ double record_word(int w, double action, double reward, double value, int idx, int man, int code, bool explored,
                                              const double (&obs)[D], const double (&x)[S])
{
  const double out = record_head<D, S>(w, action, reward, value, idx, man, code, obs, x);
  return (w == GRLX_TRAJ_OBS + D + S) ? (explored ? 1.0 : 0.0) : out;
}

// the episode of one pair by its 16-lane group; REC: with one record per step taken (lane j stores word j, and word j + 16 where R > 16)
template <int ENV, int NA, bool REC>
__device__ __forceinline__ void episode(const DevParams &P, const SampledArgs &T, double *W, double *Q)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, R = GRLX_TRAJ_OBS + D + S + 1;
  static_assert(R <= 32, "a record is stored by 16 lanes in two rounds");
  const EvaluateArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;                    // dead groups of the last wave neither load nor store nor draw

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 0, r);
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  // GRLX_EPSILON_OWN: the product the rollout kernels compare with, on the decay as it stands (never advanced here)
  const double own = A.sweep ? A.sweep[r].epsilon : P.epsilon;
  const double eps = T.epsilon < 0. ? rs.eps_decay * own : T.epsilon;
  double *rec = nullptr;
  if constexpr (REC) rec = T.records + (live ? (size_t)pair * (size_t)A.max_steps * R : 0);
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  Sums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0; e.explored = 0;
  e.S = 0; e.G = 0;
  if (live)
  {
    e.S = T.streams ? T.streams[(size_t)pair * 2] : rs.S1;
    e.G = T.streams ? T.streams[(size_t)pair * 2 + 1] : rs.G;
  }
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active) member_probe<ENV, NA>(P, tab, rs, obs, j, lane, W);
    wave_sync();
    if (active && j < NA) Q[g * 8 + j] = member_q(P, W, g, j);
    wave_sync();
    if (active)
    { // the draws sit under the step's predicate: a finished group's streams stand where its last step left them
      double q[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) q[a] = Q[g * 8 + a];
      int man;
      bool tie, explored;
      const int idx = sample<NA>(q, T.sampler, eps, e.S, e.G, man, tie, explored);
      double action = P.actions[0], value = q[0];      // selects, not indexed reads: no scratch copy of either
#pragma unroll
      for (int a = 1; a < NA; ++a)
      {
        action = (idx == a) ? P.actions[a] : action;
        value = (idx == a) ? q[a] : value;
      }
      double before[D];
      if constexpr (REC)
      {
#pragma unroll
        for (int i = 0; i < D; ++i) before[i] = obs[i];
      }
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      // episode_account (grlx_episode.h) inline, on this unit's Sums: see there why it is not an EpisodeSums
      e.ret += reward;
      e.disc += e.g * reward;
      e.g = e.g * gamma;
      e.steps++;
      e.ties += tie ? 1 : 0;
      e.explored += explored ? 1 : 0;
      e.code = (status & ST_DOMAIN) ? kEvaluateDomain : terminal;
      active = e.code == 0;
      if constexpr (REC)
      {
        double *at = rec + (size_t)(e.steps - 1) * R;
        if (j < R) at[j] = record_word<D, S>(j, action, reward, value, idx, man, e.code, explored, before, x);
        if constexpr (R > 16)
          if (j + 16 < R) at[j + 16] = record_word<D, S>(j + 16, action, reward, value, idx, man, e.code, explored, before, x);
      }
    }
  }
  if (live && j == 0)
  {
    A.ret[pair] = e.ret;
    A.disc[pair] = e.disc;
    A.steps[pair] = e.steps;
    A.terminal[pair] = e.code;
    A.ties[pair] = e.ties;
    T.explored[pair] = e.explored;
    T.streams_out[(size_t)pair * 2] = e.S;
    T.streams_out[(size_t)pair * 2 + 1] = e.G;
#pragma unroll
    for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
  }
}

} // namespace sampled

template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void evaluate_sampled_kernel(DevParams P, SampledArgs A)
{
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_q[kQueryWaves][4 * 8];
  const int wave = threadIdx.x >> 6;
  sampled::episode<ENV, NA, false>(P, A, sh_w[wave], sh_q[wave]);
}

template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_sampled_kernel(DevParams P, SampledArgs A)
{
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_q[kQueryWaves][4 * 8];
  const int wave = threadIdx.x >> 6;
  sampled::episode<ENV, NA, true>(P, A, sh_w[wave], sh_q[wave]);
}

int sampled_trajectory_words(int env)
{
  const int words = trajectory_words(env, false);
  return words ? words + 1 : 0;
}

// launch_evaluate's grid.  Every output pointer of the kernels is written without a test, so all of them are required here.
static hipError_t launch_sampled(const DevParams &P, const SampledArgs &A, bool rec, hipStream_t stream)
{
  const unsigned blocks = pair_blocks(A.e);
  if (blocks == 0) return hipSuccess;
  if (P.agent == GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.e.max_steps < 1 || (rec && !A.records) ||
      (A.sampler != GRLX_SAMPLER_GREEDY && A.sampler != GRLX_SAMPLER_EPSILON_GREEDY) || !A.streams_out || !A.explored ||
      !A.e.ret || !A.e.disc || !A.e.steps || !A.e.terminal || !A.e.ties || !A.e.final_state || !A.e.states)
    return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kQueryWaves * 64);
  with_q_instance(P, [&](auto env, auto na) {
    constexpr int ENV = decltype(env)::value, NA = decltype(na)::value;
    if (rec) hipLaunchKernelGGL((trajectory_sampled_kernel<ENV, NA>), grid, block, 0, stream, P, A);
    else hipLaunchKernelGGL((evaluate_sampled_kernel<ENV, NA>), grid, block, 0, stream, P, A);
  });
  return hipGetLastError();
}

hipError_t launch_evaluate_sampled(const DevParams &P, const SampledArgs &A, hipStream_t stream) { return launch_sampled(P, A, false, stream); }
hipError_t launch_trajectory_sampled(const DevParams &P, const SampledArgs &A, hipStream_t stream) { return launch_sampled(P, A, true, stream); }

} // namespace grlx
