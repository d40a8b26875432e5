// grlx_evaluate.hip -- greedy evaluation episodes (grlx_evaluate): for every (replica, start state) pair one episode of the test agent
// (agent/fixed over the learned tables) from a model state of the caller's choice to its end, in one launch.  Reference: the test
// branch of OnlineLearningExperiment::run (online_learning.cpp:172-213) for one episode with the caller's state in place of Task::start;
// QPolicy::act const under GreedySampler::findmax (q.cpp:129-141, greedy.cpp:47-61), ActionPolicy::act(in, out) const (action.cpp).
//
// An evaluation writes to nothing but its own output arrays.  Every step is the body of query_q_kernel / query_state_kernel
// (grlx_query.hip: peek-only probes through query_weights, slots without an entry contribute initial_weight(); no entry is created, no
// counter, stream, trace, key bit or sticky status is touched) followed by the environment step of the rollout kernels
// (env_step<ENV, false, NoShare>, grlx_envs.h).
//
// Layout: the queries'.  A 16-lane group serves one (replica, start state) pair, lane = tiling, four pairs per wave, four waves per block
// (no wave waits for another: every LDS region belongs to one wave).  Pair = replica * n_starts + start, so the groups of a wave mostly
// probe one replica's table and mostly run episodes of similar length.  All 16 lanes of a group integrate the same state redundantly: the
// bits are identical in every lane and the environment needs no cross-lane traffic.
//
// The episode loop is wave-uniform: it runs while a ballot finds an active group and the step counter is below max_steps -- the bound
// that keeps a caller-made state from becoming a hang.  Finished and dead groups skip loads, LDS stores, the environment step and the
// sums under a predicate; every lane reaches every wave_sync.  Lane 0 of a group writes the pair's outputs once, after the loop.
//
// LDS: the weight tile of grlx_query.hip (rows kRowStride = 66 doubles apart, see the bank argument there), the group's Q-values, and
// two words per group by which lane 0 hands findmax's result (the actor-critic: the action) back to the 16 lanes.
//
// evaluate_ensemble_kernel (grlx_evaluate_ensemble): the same episode for a GROUP of consecutive replicas that share one environment state
// and act on their vote or their summed Q; its layout is described at the kernel.
//
// trajectory_q_kernel, trajectory_ac_kernel, trajectory_ensemble_kernel (grlx_evaluate_trajectory, grlx_evaluate_ensemble_trajectory): the
// same episodes with one record per step taken, in kernels of their own below the three above, which they leave as they are.
//
// The step's helpers (the probes, the reads, findmax, the bookkeeping, the head of a record) and the dispatch over the instantiations
// live in grlx_episode.h, which the units of the evaluation variants share.  evaluate_q_kernel, evaluate_ac_kernel and
// trajectory_ac_kernel mirror some of them inline, each under a comment that says which and why.
//
// Compiled with -ffp-contract=off like every unit: g * reward is a plain product, the sums plain additions.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate.h"
#include "grlx_episode.h"

namespace grlx {

// Q agents: actions[first maximum of Q(obs, .)] at every step.  The probe, the maximum and the action select below mirror member_probe,
// findmax and action_of (grlx_episode.h) inline: calling any of the three from this kernel changed its machine code (instruction counts,
// on the walker the registers).  member_q is called: it leaves the kernel instruction for instruction the same.
template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void evaluate_q_kernel(DevParams P, EvaluateArgs A)
{
  constexpr int T = kLanesPerReplica, S = Env<ENV>::S, D = Env<ENV>::D;
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_q[kQueryWaves][4 * 8];
  __shared__ int32_t sh_a[kQueryWaves][4 * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;                    // dead groups of the last wave neither load nor store
  double *W = sh_w[wave], *Q = sh_q[wave];
  int32_t *M = sh_a[wave];

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 0, r);
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = live ? A.states[(size_t)s * S + i] : 0.;
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active)
    { // project(obs, a_k), k < NA: the hash of the observation once, then the action's coordinate and the tiling (tile_coding.cpp:103-149)
      uint32_t hpre = 449u ^ (uint32_t)(D + 2);
#pragma unroll
      for (int i = 0; i < D; ++i)
        hpre = murmur_mix(hpre, tile_coord<T>(P.tile, i, tile_quant(P.tile, i, obs[i]), j));
      uint32_t slot[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a)
      {
        uint32_t h = murmur_mix(hpre, tile_coord<T>(P.tile, D, tile_quant(P.tile, D, P.actions[a]), j));
        h = murmur_mix(h, j);
        slot[a] = murmur_final(h) % (uint32_t)P.tile.memory;
      }
      double w[NA];
      query_weights<NA>(tab, rs, 0, P.lin, slot, w);
#pragma unroll
      for (int a = 0; a < NA; ++a) W[a * kRowStride + lane] = w[a];
    }
    wave_sync();
    if (active && j < NA) Q[g * 8 + j] = member_q(P, W, g, j);
    wave_sync();
    if (active && j == 0)
    { // greedy.cpp:47-61
      int mai = 0, man = 1;
      double best = Q[g * 8];
#pragma unroll
      for (int a = 1; a < NA; ++a)
      {
        const double q = Q[g * 8 + a];
        if (q > best) { best = q; mai = a; man = 1; }
        else if (q == best) man++;
      }
      M[g * 2] = mai;
      M[g * 2 + 1] = man;
    }
    wave_sync();
    if (active)
    {
      const int mai = M[g * 2], man = M[g * 2 + 1];
      double action = P.actions[0];                    // selects, not an indexed read of the parameter block: no scratch copy of it
#pragma unroll
      for (int a = 1; a < NA; ++a) action = (mai == a) ? P.actions[a] : action;
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, gamma, terminal, status, man > 1);
    }
  }
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// Ensembles of Q agents: one episode per (group of G consecutive replicas, start state); at every step the members' first maxima are
// counted (votes) and their Q-values summed, both over the members in ASCENDING order, and the episode acts on the first maximum of
// the votes (GRLX_ENSEMBLE_VOTE) or of the sums (GRLX_ENSEMBLE_MEAN_Q).  Reference: MultiDiscretePolicy::act (multi_discrete.cpp:
// 120-235) under policy_strategy_majority_voting_prob / _add_prob; see include/grlx.h for what differs.
//
// Layout: one block of kQueryWaves waves serves one episode; its 16 lane groups serve 16 members per round, ceil(G / 16) rounds per step.
// Per round: member_probe, the wave's barrier, member_q by lanes j < NA into the member's slot of sh_m, then the block's barrier, after
// which EVERY thread continues the same votes / sumq accumulators over the round's slots in ascending member order -- broadcast LDS
// reads, identical bits in every thread, so no result is handed back.  All 256 threads integrate the same state redundantly: the
// episode's end is block-uniform by construction, and every thread reaches every barrier.
//
// sh_m is double-buffered by the parity of a round counter that runs through the episode.  A thread that writes buffer p in round k + 2
// has passed the block barrier of round k + 1, which every thread reaches only after its reads of round k (buffer p) are done.  The
// wave's tile W is written again only after that block barrier too, which orders it after the wave's own reads of the round before.
// Dead member slots (member >= G) skip loads and stores; nobody reads their slots.
// thread 0 of the block writes the pair's outputs once, after the loop
template <int S>
__device__ __forceinline__ void ensemble_store(const EnsembleArgs &A, const EpisodeSums &e, long long member_ties, long long agreement, const double (&x)[S])
{
  const long long pair = blockIdx.x;                   // group * n_starts + start
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
  A.member_ties[pair] = member_ties;
  A.agreement[pair] = agreement;
#pragma unroll
  for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
}

template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void evaluate_ensemble_kernel(DevParams P, EnsembleArgs A)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, kSlots = kQueryWaves * 4;
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_m[2][kSlots][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int slot = wave * 4 + g;                       // the member of a round this lane group serves
  const int G = A.group_size;
  const int grp = (int)(blockIdx.x / (unsigned)A.n_starts), s = (int)(blockIdx.x - (unsigned)grp * (unsigned)A.n_starts);
  const int r0 = A.first_replica + grp * G;
  double *W = sh_w[wave];

  const double gamma = A.sweep ? A.sweep[r0].gamma : P.gamma;      // the group's first replica's
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = A.states[(size_t)s * S + i];
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  long long member_ties = 0, agreement = 0;
  unsigned round = 0;
  bool active = true;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // block-uniform: every thread holds the same state
    int votes[NA];
    double sumq[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) { votes[a] = 0; sumq[a] = 0.; }
    for (int m0 = 0; m0 < G; m0 += kSlots, ++round)
    {
      double (*MQ)[8] = sh_m[round & 1u];
      const bool member = m0 + slot < G;
      const int r = r0 + (member ? m0 + slot : 0);
      if (member) member_probe<ENV, NA>(P, table_of(P, 0, r), P.states[r], obs, j, lane, W);
      wave_sync();
      if (member && j < NA) MQ[slot][j] = member_q(P, W, g, j);
      __syncthreads();
      const int n = G - m0 < kSlots ? G - m0 : kSlots;
      for (int m = 0; m < n; ++m)
      {
        double q[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) q[a] = MQ[m][a];
        int mai, man;
        findmax<NA>(q, mai, man);
#pragma unroll
        for (int a = 0; a < NA; ++a)
        {
          votes[a] += (mai == a) ? 1 : 0;
          sumq[a] += q[a];
        }
        member_ties += man > 1 ? 1 : 0;
      }
    }
    int mai, man;
    if (A.rule == GRLX_ENSEMBLE_VOTE) findmax<NA>(votes, mai, man);
    else findmax<NA>(sumq, mai, man);
    int agree = votes[0];
#pragma unroll
    for (int a = 1; a < NA; ++a) agree = (mai == a) ? votes[a] : agree;
    agreement += agree;
    const double action = action_of<NA>(P, mai);
    double reward = 0;
    int terminal = 0;
    uint32_t status = 0;
    env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
    active = episode_account(e, reward, gamma, terminal, status, man > 1);
  }
  if (threadIdx.x == 0) ensemble_store<S>(A, e, member_ties, agreement, x);
}

// actor-critic: the noise-free actor, fmin(fmax(read(actor table, obs), action_min), action_max) (ActionPolicy::act(in, out) const).
// The projection and the read mirror actor_probe and read_actor (grlx_episode.h) inline: calling them changes this kernel's machine code.
template <int ENV>
__global__ __launch_bounds__(kQueryWaves * 64) void evaluate_ac_kernel(DevParams P, EvaluateArgs A)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D;
  __shared__ double sh_w[kQueryWaves][64];
  __shared__ double sh_act[kQueryWaves][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_starts;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;
  double *W = sh_w[wave], *ACT = sh_act[wave];

  const int rl = live ? (int)(pair / A.n_starts) : 0, s = live ? (int)(pair - (long long)rl * A.n_starts) : 0;
  const int r = A.first_replica + rl;
  const Table tab = table_of(P, 1, r);                 // twin tables: each holds its own keys
  const ReplicaState &rs = P.states[r];
  const double gamma = A.sweep ? A.sweep[r].gamma : P.gamma;
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
    if (active)
    {
      // project(obs) of the actor's projector (tile_coding.cpp:103-149), unrolled over the observation: tile_slot_generic's loop
      // indexes obs by a run-time counter, which puts obs into scratch
      uint32_t h = 449u ^ (uint32_t)(D + 1);
#pragma unroll
      for (int i = 0; i < D; ++i)
        h = murmur_mix(h, tile_coord<kLanesPerReplica>(P.tile_actor, i, tile_quant(P.tile_actor, i, obs[i]), j));
      h = murmur_mix(h, j);
      uint32_t slot[1] = {murmur_final(h) % (uint32_t)P.tile_actor.memory};
      double w[1];
      query_weights<1>(tab, rs, 1, P.lin_actor, slot, w);
      W[lane] = w[0];
    }
    wave_sync();
    if (active && j == 0)
    { // ActionPolicy::read (action.cpp:99-112) over LinearRepresentation::read, then the clip of act
      double sum = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) sum += W[g * 16 + k];
      sum /= 16;
      sum = query_clamp(sum, P.lin_actor.out_min, P.lin_actor.out_max);
      ACT[g] = query_clamp(sum, P.action_min, P.action_max);
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
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// ---- per-step trajectories (grlx_evaluate_trajectory, grlx_evaluate_ensemble_trajectory) ------------------------------------------------
// The episodes above with one record of R doubles per step taken (include/grlx.h: GRLX_TRAJ_*), in kernels of their own: the evaluation
// kernels are not touched and share nothing new with these.  Same layouts.  The one new thing in the loop is the store.  Every lane of a
// group (the ensemble: every thread of the block) holds the step's R values, bit for bit the same, so lane j stores word j -- and word
// j + 16 where R > 16 --: one store instruction per wave and step (two for the walker), each group writing one contiguous run of 8 R
// bytes, an episode's records one after the other.  The word is picked by selects unrolled at compile time; indexing the values by the
// lane number would put them into scratch.  The store comes after episode_account, at index steps - 1, so that the terminal word is the
// code after the step; finished and dead groups store nothing, and nothing is written behind an episode's end (the caller zero-fills).

// Word w of a step's record of the ensemble, whose two words more sit before the observation: record_head's selects (grlx_episode.h) in
// the record's own order.  Any w outside the record gives the action.
template <int D, int S>
__device__ __forceinline__ double ensemble_record_word(int w, double action, double reward, double value, int mai, int man, int code, int agree,
                                                       int member_ties, const double (&obs)[D], const double (&x)[S])
{
  double out = action;
  out = (w == GRLX_TRAJ_REWARD) ? reward : out;
  out = (w == GRLX_TRAJ_VALUE) ? value : out;
  out = (w == GRLX_TRAJ_ACTION_INDEX) ? (double)mai : out;
  out = (w == GRLX_TRAJ_N_MAX) ? (double)man : out;
  out = (w == GRLX_TRAJ_TERMINAL) ? (double)code : out;
  out = (w == GRLX_TRAJ_ENS_AGREEMENT) ? (double)agree : out;
  out = (w == GRLX_TRAJ_ENS_MEMBER_TIES) ? (double)member_ties : out;
#pragma unroll
  for (int i = 0; i < D; ++i) out = (w == GRLX_TRAJ_ENS_OBS + i) ? obs[i] : out;
#pragma unroll
  for (int i = 0; i < S; ++i) out = (w == GRLX_TRAJ_ENS_OBS + D + i) ? x[i] : out;
  return out;
}

// evaluate_q_kernel with records.  After the Q-values are in LDS every lane of the group reads them (broadcast) and runs findmax itself,
// as the ensemble kernel's threads do: the same bits in every lane, and no word is handed back through LDS.
template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_q_kernel(DevParams P, TrajectoryArgs T)
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
  double *rec = T.records + (live ? (size_t)pair * (size_t)A.max_steps * R : 0);     // 64-bit: pairs * max_steps * R * 8 bytes pass 2^32 at a million pairs of 100 steps
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
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// evaluate_ac_kernel with records.  Every lane of the group sums the 16 weights itself (broadcast reads): the value word, the actor's
// read before the action clip, is then in every lane, and nothing is handed back through LDS.  The projection and the read mirror
// actor_probe and read_actor (grlx_episode.h) inline, as evaluate_ac_kernel's do and for its reason.
template <int ENV>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_ac_kernel(DevParams P, TrajectoryArgs T)
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
    if (active)
    { // project(obs) of the actor's projector, unrolled over the observation as in evaluate_ac_kernel
      uint32_t h = 449u ^ (uint32_t)(D + 1);
#pragma unroll
      for (int i = 0; i < D; ++i)
        h = murmur_mix(h, tile_coord<kLanesPerReplica>(P.tile_actor, i, tile_quant(P.tile_actor, i, obs[i]), j));
      h = murmur_mix(h, j);
      uint32_t slot[1] = {murmur_final(h) % (uint32_t)P.tile_actor.memory};
      double w[1];
      query_weights<1>(tab, rs, 1, P.lin_actor, slot, w);
      W[lane] = w[0];
    }
    wave_sync();
    if (active)
    { // ActionPolicy::read (action.cpp:99-112) over LinearRepresentation::read, then the clip of act
      double sum = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) sum += W[g * 16 + k];
      sum /= 16;
      const double value = query_clamp(sum, P.lin_actor.out_min, P.lin_actor.out_max);
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
  if (live && j == 0) episode_store<S>(A, pair, e, x);
}

// evaluate_ensemble_kernel with records: two more words, the step's votes[mai] and its members with a tie; threads 0 .. R - 1 of the
// block (all of wave 0: R <= 24) store one word each.
template <int ENV, int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void trajectory_ensemble_kernel(DevParams P, EnsembleTrajectoryArgs T)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, kSlots = kQueryWaves * 4, R = GRLX_TRAJ_ENS_OBS + D + S;
  static_assert(R <= 64, "the record is stored by one wave");
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_m[2][kSlots][8];
  const EnsembleArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int slot = wave * 4 + g;                       // the member of a round this lane group serves
  const int G = A.group_size;
  const int grp = (int)(blockIdx.x / (unsigned)A.n_starts), s = (int)(blockIdx.x - (unsigned)grp * (unsigned)A.n_starts);
  const int r0 = A.first_replica + grp * G;
  double *W = sh_w[wave];
  double *rec = T.records + (size_t)blockIdx.x * (size_t)A.max_steps * R + threadIdx.x;      // the thread's word of the episode's first record

  const double gamma = A.sweep ? A.sweep[r0].gamma : P.gamma;      // the group's first replica's
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = A.states[(size_t)s * S + i];
  (void)Env<ENV>::observe(P, x, obs);

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  long long member_ties = 0, agreement = 0;
  unsigned round = 0;
  bool active = true;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // block-uniform: every thread holds the same state
    int votes[NA];
    const long long ties_before = member_ties;
    double sumq[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) { votes[a] = 0; sumq[a] = 0.; }
    for (int m0 = 0; m0 < G; m0 += kSlots, ++round)
    {
      double (*MQ)[8] = sh_m[round & 1u];
      const bool member = m0 + slot < G;
      const int r = r0 + (member ? m0 + slot : 0);
      if (member) member_probe<ENV, NA>(P, table_of(P, 0, r), P.states[r], obs, j, lane, W);
      wave_sync();
      if (member && j < NA) MQ[slot][j] = member_q(P, W, g, j);
      __syncthreads();
      const int n = G - m0 < kSlots ? G - m0 : kSlots;
      for (int m = 0; m < n; ++m)
      {
        double q[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) q[a] = MQ[m][a];
        int mai, man;
        findmax<NA>(q, mai, man);
#pragma unroll
        for (int a = 0; a < NA; ++a)
        {
          votes[a] += (mai == a) ? 1 : 0;
          sumq[a] += q[a];
        }
        member_ties += man > 1 ? 1 : 0;
      }
    }
    int mai, man;
    if (A.rule == GRLX_ENSEMBLE_VOTE) findmax<NA>(votes, mai, man);
    else findmax<NA>(sumq, mai, man);
    int agree = votes[0];
    double score = sumq[0];
#pragma unroll
    for (int a = 1; a < NA; ++a)
    {
      agree = (mai == a) ? votes[a] : agree;
      score = (mai == a) ? sumq[a] : score;
    }
    if (A.rule == GRLX_ENSEMBLE_VOTE) score = (double)agree;
    agreement += agree;
    const int step_ties = (int)(member_ties - ties_before);
    const double action = action_of<NA>(P, mai);
    double before[D];
#pragma unroll
    for (int i = 0; i < D; ++i) before[i] = obs[i];
    double reward = 0;
    int terminal = 0;
    uint32_t status = 0;
    env_step<ENV, false, NoShare>(P, x, action, obs, reward, terminal, status);
    active = episode_account(e, reward, gamma, terminal, status, man > 1);
    if (threadIdx.x < R)
      rec[(size_t)(e.steps - 1) * R] =
          ensemble_record_word<D, S>((int)threadIdx.x, action, reward, score, mai, man, e.code, agree, step_ties, before, x);
  }
  if (threadIdx.x == 0) ensemble_store<S>(A, e, member_ties, agreement, x);
}

// The instantiations: the (environment, action count) pairs grlx_create admits for the Q agents, and the actor-critic's two environments
bool evaluate_built(int agent, int env, int actions)
{
  if (agent == GRLX_AGENT_AC) return env == GRLX_ENV_CART_POLE || env == GRLX_ENV_PENDULUM;
  if (env == GRLX_ENV_PENDULUM) return actions == 3 || actions == 5;
  return (env == GRLX_ENV_ACROBOT || env == GRLX_ENV_CART_POLE || env == GRLX_ENV_COMPASS_WALKER) && actions == 3;
}

hipError_t launch_evaluate(const DevParams &P, const EvaluateArgs &A, hipStream_t stream)
{
  const unsigned blocks = pair_blocks(A);
  if (blocks == 0) return hipSuccess;
  if (!evaluate_built(P.agent, P.env, P.A) || A.max_steps < 1) return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kQueryWaves * 64);
  if (P.agent == GRLX_AGENT_AC)
    with_ac_instance(P, [&](auto env) { hipLaunchKernelGGL(evaluate_ac_kernel<decltype(env)::value>, grid, block, 0, stream, P, A); });
  else
    with_q_instance(P, [&](auto env, auto na) {
      hipLaunchKernelGGL((evaluate_q_kernel<decltype(env)::value, decltype(na)::value>), grid, block, 0, stream, P, A);
    });
  return hipGetLastError();
}

// one block per (group, start state)
hipError_t launch_evaluate_ensemble(const DevParams &P, const EnsembleArgs &A, hipStream_t stream)
{
  if (A.group_size < 1 || A.n_replicas % A.group_size != 0) return hipErrorInvalidValue;
  const long long blocks = (long long)(A.n_replicas / A.group_size) * A.n_starts;
  if (blocks == 0) return hipSuccess;
  if (P.agent == GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.max_steps < 1 || blocks > 0x7fffffffll ||
      (A.rule != GRLX_ENSEMBLE_VOTE && A.rule != GRLX_ENSEMBLE_MEAN_Q))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kQueryWaves * 64);
  with_q_instance(P, [&](auto env, auto na) {
    hipLaunchKernelGGL((evaluate_ensemble_kernel<decltype(env)::value, decltype(na)::value>), grid, block, 0, stream, P, A);
  });
  return hipGetLastError();
}

int trajectory_words(int env, bool ensemble)
{
  const int head = ensemble ? GRLX_TRAJ_ENS_OBS : GRLX_TRAJ_OBS;
  switch (env)
  {
    case GRLX_ENV_PENDULUM: return head + Env<GRLX_ENV_PENDULUM>::D + Env<GRLX_ENV_PENDULUM>::S;
    case GRLX_ENV_ACROBOT: return head + Env<GRLX_ENV_ACROBOT>::D + Env<GRLX_ENV_ACROBOT>::S;
    case GRLX_ENV_CART_POLE: return head + Env<GRLX_ENV_CART_POLE>::D + Env<GRLX_ENV_CART_POLE>::S;
    case GRLX_ENV_COMPASS_WALKER: return head + Env<GRLX_ENV_COMPASS_WALKER>::D + Env<GRLX_ENV_COMPASS_WALKER>::S;
    default: return 0;
  }
}

// launch_evaluate's grid; A.records zero-filled by the caller
hipError_t launch_trajectory(const DevParams &P, const TrajectoryArgs &A, hipStream_t stream)
{
  const unsigned blocks = pair_blocks(A.e);
  if (blocks == 0) return hipSuccess;
  if (!evaluate_built(P.agent, P.env, P.A) || A.e.max_steps < 1 || !A.records) return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kQueryWaves * 64);
  if (P.agent == GRLX_AGENT_AC)
    with_ac_instance(P, [&](auto env) { hipLaunchKernelGGL(trajectory_ac_kernel<decltype(env)::value>, grid, block, 0, stream, P, A); });
  else
    with_q_instance(P, [&](auto env, auto na) {
      hipLaunchKernelGGL((trajectory_q_kernel<decltype(env)::value, decltype(na)::value>), grid, block, 0, stream, P, A);
    });
  return hipGetLastError();
}

// one block per (group, start state); A.records zero-filled by the caller
hipError_t launch_trajectory_ensemble(const DevParams &P, const EnsembleTrajectoryArgs &A, hipStream_t stream)
{
  if (A.e.group_size < 1 || A.e.n_replicas % A.e.group_size != 0) return hipErrorInvalidValue;
  const long long blocks = (long long)(A.e.n_replicas / A.e.group_size) * A.e.n_starts;
  if (blocks == 0) return hipSuccess;
  if (P.agent == GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.e.max_steps < 1 || blocks > 0x7fffffffll || !A.records ||
      (A.e.rule != GRLX_ENSEMBLE_VOTE && A.e.rule != GRLX_ENSEMBLE_MEAN_Q))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kQueryWaves * 64);
  with_q_instance(P, [&](auto env, auto na) {
    hipLaunchKernelGGL((trajectory_ensemble_kernel<decltype(env)::value, decltype(na)::value>), grid, block, 0, stream, P, A);
  });
  return hipGetLastError();
}

} // namespace grlx
