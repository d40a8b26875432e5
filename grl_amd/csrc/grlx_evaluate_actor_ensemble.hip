// grlx_evaluate_actor_ensemble.hip -- episodes of an ensemble of actors (grlx_evaluate_actor_ensemble, grlx_evaluate_actor_ensemble_trajectory):
// one episode per (group of G consecutive actor-critic replicas, start state); the members share ONE environment state and at every step
// their noise-free actions a_0 ... a_{G-1} -- each what grlx_evaluate would hand the environment for that replica -- are combined into the
// action that acts.  Reference: mapping/policy/multi (base/src/policies/multi.cpp) under csMean (:507-523), csBinning (:126-181),
// csDataCenter (:251-336) and csDensityBased (:183-248); include/grlx.h states every rule as a serial loop and what differs (no random
// draw: the first of tied candidates acts and the step is counted).
//
// A unit of its own beside grlx_evaluate.hip.  The actor's probe and read, the bookkeeping and the head of a record are grlx_episode.h's;
// what is below is this unit's alone: the rules, the store and the record's two last words.
//
// Layout: evaluate_ensemble_kernel's.  One block of kQueryWaves waves serves one episode; its 16 lane groups probe 16 members per round
// (actor_probe, the wave's barrier, read_actor and the clip by lane 0 of the group), ceil(G / 16) rounds per step.  Lane 0 of a group
// stores the member's action into sh_a and, where the rule needs it, the member's normalised action (DENSITY) or bin (BINNING) into
// sh_x.  After the step's block barrier EVERY thread runs the same combination over broadcast LDS reads in ascending member order:
// identical bits in every thread, so no result is handed back, all 256 threads integrate the same state redundantly, the episode's end
// is block-uniform by construction and every thread reaches every barrier.
//
// The one shared-out part: under DENSITY thread t < G computes rho_t, the G exponentials of member t (G * G in the block, not in every
// thread), and under BINNING the number of members in member t's bin; both go to sh_r, one more block barrier follows, and then every
// thread scans sh_r.  The rule is a kernel argument, so that barrier is block-uniform too.
//
// LDS hazards.  sh_a and sh_x are double-buffered by the step's parity: a thread that writes buffer p at step k + 2 has passed the block
// barrier of step k + 1, which every thread reaches only after its combination of step k (the reads of buffer p) is done.  sh_r has one
// buffer: it is written after the first block barrier of a step, which every thread reaches only after its scan of the step before.  A
// wave's tile W is read by lane 0 of each group and written again in the next round: a wave barrier stands between.  Dead member slots
// (member >= G: the partial last round) skip loads and stores under one predicate; nobody reads their slots.
//
// Compiled with -ffp-contract=off like every unit: every product, sum and quotient of the rules is a plain one.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate_actor_ensemble.h"
#include "grlx_episode.h"

namespace grlx {
namespace actor_ensemble {

static_assert(GRLX_ACTOR_ENSEMBLE_MAX <= kQueryWaves * 64, "thread t serves member t in the shared-out part of a rule");

// what a rule hands back: the action, GRLX_TRAJ_ACTION_INDEX, GRLX_TRAJ_N_MAX, the members that entered the action, did the selection tie
struct Combined {
  double action;
  int    index, n_max, kept;
  bool   tie;
};

// csBinning's bin of an action (multi.cpp:141): the action is clipped, so the quotient is not negative
__device__ __forceinline__ int bin_of(double a, int B, double lo, double hi)
{
  const int b = (int)__builtin_floor(((double)B * (a - lo)) / (hi - lo));
  return b < B - 1 ? b : B - 1;
}

// csDensityBased's normalised action (multi.cpp:196)
__device__ __forceinline__ double normalised(double a, double lo, double hi) { return -1 + 2 * ((a - lo) / (hi - lo)); }

// thread t's share of BINNING: the members in member t's bin
__device__ __forceinline__ double bin_count(const double *SX, int G, int t)
{
  const double mine = SX[t];
  int n = 0;
  for (int i = 0; i < G; ++i) n += SX[i] == mine ? 1 : 0;
  return (double)n;
}

// thread t's share of DENSITY: rho_t, summed over the members in ascending order from 0.0
__device__ __forceinline__ double density(const double *SX, int G, int t, double r)
{
  const double mine = SX[t];
  double rho = 0.0;
  for (int i = 0; i < G; ++i)
  {
    const double d = mine - SX[i];
    rho += pexp((-1 * (d * d)) / (r * r));
  }
  return rho;
}

// csBinning after the counts: the greatest count, its first bin, and the mean of EVERY member whose bin holds that count -- the members
// of another bin with the same count included, as the reference's test hist[bin(a_i)] == hist[binmax] includes them
__device__ __forceinline__ Combined binning(const double *SA, const double *SX, const double *SR, int G)
{
  double most = 0;
  for (int i = 0; i < G; ++i) most = SR[i] > most ? SR[i] : most;
  double s = 0.0, binmax = 0;
  int n = 0;
  for (int i = 0; i < G; ++i)
    if (SR[i] == most)
    {
      binmax = (n == 0 || SX[i] < binmax) ? SX[i] : binmax;
      s += SA[i];
      ++n;
    }
  Combined c;
  c.action = s / n;
  c.index = (int)binmax;
  c.n_max = n / (int)most;                           // the bins that hold the greatest count
  c.kept = n;
  c.tie = c.n_max > 1;
  return c;
}

// csDensityBased after the densities: the first member of strictly greatest rho, scanning from -inf
__device__ __forceinline__ Combined densest(const double *SA, const double *SR, int G)
{
  double best = -__builtin_inf();
  int at = 0, n = 0;
  for (int i = 0; i < G; ++i)
  {
    const double rho = SR[i];
    if (rho > best) { best = rho; at = i; n = 1; }
    else if (rho == best) n++;
  }
  Combined c;
  c.action = SA[at];
  c.index = at;
  c.n_max = n;
  c.kept = 1;
  c.tie = n > 1;
  return c;
}

// the alive members of csDataCenter as four 64-bit words, indexed by constants only (a run-time index would put them into scratch)
struct Alive {
  unsigned long long w[4];
};

// f(i) for the alive members i in ascending order
template <class F>
__device__ __forceinline__ void for_alive(const Alive &al, F &&f)
{
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (unsigned long long m = al.w[k]; m; m &= m - 1) f(k * 64 + __ffsll((long long)m) - 1);
}

// the serial sum of the alive members, starting from the first one and not from 0.0, over their count
__device__ __forceinline__ double alive_mean(const double *SA, const Alive &al)
{
  double s = 0;
  int n = 0;
  for_alive(al, [&](int i) {
    s = n == 0 ? SA[i] : s + SA[i];
    ++n;
  });
  return s / n;
}

// csDataCenter: while more than K members are alive, the first alive member farthest from the alive members' mean is removed
__device__ __forceinline__ Combined data_center(const double *SA, int G, int K)
{
  Alive al;
#pragma unroll
  for (int k = 0; k < 4; ++k)
  {
    const int n = G - k * 64;
    al.w[k] = n >= 64 ? ~0ull : n > 0 ? (1ull << n) - 1ull : 0ull;
  }
  Combined c;
  c.index = -1;
  c.n_max = 1;
  double mean = alive_mean(SA, al);
  int alive = G;
  while (alive > K)
  {
    double far = 0;
    int at = -1, n = 0;
    for_alive(al, [&](int i) {
      const double d = (SA[i] - mean) * (SA[i] - mean);
      if (at < 0 || d > far) { far = d; at = i; n = 1; }
      else if (d == far) n++;
    });
    c.n_max = n > c.n_max ? n : c.n_max;
#pragma unroll
    for (int k = 0; k < 4; ++k) al.w[k] &= (at >> 6) == k ? ~(1ull << (at & 63)) : ~0ull;
    --alive;
    mean = alive_mean(SA, al);
  }
  c.action = mean;
  c.kept = alive;
  c.tie = c.n_max > 1;
  return c;
}

// thread 0 of the block writes the pair's outputs once, after the loop
template <int S>
__device__ __forceinline__ void store(const ActorEnsembleArgs &A, const EpisodeSums &e, long long kept, double spread, const double (&x)[S])
{
  const long long pair = blockIdx.x;                   // group * n_starts + start
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
  A.kept[pair] = kept;
  A.spread[pair] = spread;
#pragma unroll
  for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
}

} // namespace actor_ensemble

// REC: one record per step taken, record_head's words of the actor-critic and two more, the step's kept and its spread; threads
// 0 ... R - 1 of the block (all of wave 0) store one word each
template <int ENV, bool REC>
__global__ __launch_bounds__(kQueryWaves * 64) void actor_ensemble_kernel(DevParams P, ActorEnsembleArgs A)
{
  using namespace actor_ensemble;
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, kSlots = kQueryWaves * 4, R = GRLX_TRAJ_OBS + D + S + 2;
  static_assert(R <= 64, "the record is stored by one wave");
  __shared__ double sh_w[kQueryWaves][64];
  __shared__ double sh_a[2][GRLX_ACTOR_ENSEMBLE_MAX];
  __shared__ double sh_x[2][GRLX_ACTOR_ENSEMBLE_MAX];
  __shared__ double sh_r[GRLX_ACTOR_ENSEMBLE_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int slot = wave * 4 + g;                       // the member of a round this lane group serves
  const int G = A.group_size, rule = A.rule;
  const int grp = (int)(blockIdx.x / (unsigned)A.n_starts), s = (int)(blockIdx.x - (unsigned)grp * (unsigned)A.n_starts);
  const int r0 = A.first_replica + grp * G;
  const double lo = P.action_min, hi = P.action_max;
  double *W = sh_w[wave];
  double *rec = REC ? A.records + (size_t)blockIdx.x * (size_t)A.max_steps * R + threadIdx.x : nullptr;   // the thread's word of the first record

  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = A.states[(size_t)s * S + i];
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  long long kept = 0;
  double spread = 0;
  bool active = true;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // block-uniform: every thread holds the same state
    double *SA = sh_a[step & 1], *SX = sh_x[step & 1];
    for (int m0 = 0; m0 < G; m0 += kSlots)
    {
      const bool member = m0 + slot < G;
      const int r = r0 + (member ? m0 + slot : 0);
      if (member) actor_probe<ENV>(P, table_of(P, 1, r), P.states[r], obs, j, lane, W);
      wave_sync();
      if (member && j == 0)
      { // ActionPolicy::act(in, out) const: the read, its clamp, the clip
        const double a = query_clamp(read_actor(P, W, g), lo, hi);
        SA[m0 + slot] = a;
        if (rule == GRLX_ACTOR_ENSEMBLE_BINNING) SX[m0 + slot] = (double)bin_of(a, A.bins, lo, hi);
        if (rule == GRLX_ACTOR_ENSEMBLE_DENSITY) SX[m0 + slot] = normalised(a, lo, hi);
      }
      wave_sync();                                     // the reads above come before the next round's weights
    }
    __syncthreads();
    if (rule == GRLX_ACTOR_ENSEMBLE_BINNING || rule == GRLX_ACTOR_ENSEMBLE_DENSITY)
    { // the shared-out part: member t's count or density by thread t
      if ((int)threadIdx.x < G)
        sh_r[threadIdx.x] = rule == GRLX_ACTOR_ENSEMBLE_BINNING ? bin_count(SX, G, (int)threadIdx.x) : density(SX, G, (int)threadIdx.x, A.r);
      __syncthreads();
    }
    // csMean's expression (GRLX_TRAJ_VALUE under every rule) and the step's spread, in one pass
    double m = SA[0], top = SA[0], bottom = SA[0];
    for (int i = 1; i < G; ++i)
    {
      const double a = SA[i];
      m = m + a;
      top = a > top ? a : top;
      bottom = a < bottom ? a : bottom;
    }
    m = m / (double)G;
    Combined c;
    if (rule == GRLX_ACTOR_ENSEMBLE_BINNING) c = binning(SA, SX, sh_r, G);
    else if (rule == GRLX_ACTOR_ENSEMBLE_DENSITY) c = densest(SA, sh_r, G);
    else if (rule == GRLX_ACTOR_ENSEMBLE_DATA_CENTER) c = data_center(SA, G, A.bins);
    else { c.action = m; c.index = -1; c.n_max = 1; c.kept = G; c.tie = false; }
    const double wide = top - bottom;
    kept += c.kept;
    spread += wide;
    double before[D];
    if constexpr (REC)
    {
#pragma unroll
      for (int i = 0; i < D; ++i) before[i] = obs[i];
    }
    double reward = 0;
    int terminal = 0;
    uint32_t status = 0;
    env_step<ENV, false, NoShare>(P, x, c.action, obs, reward, terminal, status);   // no clip after the combination: the task's actuate does its own
    active = episode_account(e, reward, P.gamma, terminal, status, c.tie);
    if constexpr (REC)
    {
      if (threadIdx.x < R)
      {
        const int w = (int)threadIdx.x;
        double out = record_head<D, S>(w, c.action, reward, m, c.index, c.n_max, e.code, before, x);
        out = (w == R - 2) ? (double)c.kept : out;
        out = (w == R - 1) ? wide : out;
        rec[(size_t)(e.steps - 1) * R] = out;
      }
    }
  }
  if (threadIdx.x == 0) store<S>(A, e, kept, spread, x);
}

int actor_ensemble_trajectory_words(int env)
{
  const int words = trajectory_words(env, false);
  return words ? words + 2 : 0;
}

// one block per (group, start state).  Every output pointer of the kernels is written without a test, so all of them are required here.
static hipError_t launch_actor_ensemble(const DevParams &P, const ActorEnsembleArgs &A, bool rec, hipStream_t stream)
{
  if (A.group_size < 1 || A.group_size > GRLX_ACTOR_ENSEMBLE_MAX || A.n_replicas % A.group_size != 0) return hipErrorInvalidValue;
  const long long blocks = (long long)(A.n_replicas / A.group_size) * A.n_starts;
  if (blocks == 0) return hipSuccess;
  const bool rule_ok = A.rule == GRLX_ACTOR_ENSEMBLE_MEAN || (A.rule == GRLX_ACTOR_ENSEMBLE_BINNING && A.bins >= 1 && A.bins <= 64) ||
                       (A.rule == GRLX_ACTOR_ENSEMBLE_DATA_CENTER && A.bins >= 1) || (A.rule == GRLX_ACTOR_ENSEMBLE_DENSITY && A.r > 0 && A.r < __builtin_inf());
  if (P.agent != GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.max_steps < 1 || blocks > 0x7fffffffll || !rule_ok || (rec && !A.records) ||
      !A.states || !A.ret || !A.disc || !A.steps || !A.terminal || !A.ties || !A.kept || !A.spread || !A.final_state)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kQueryWaves * 64);
  with_ac_instance(P, [&](auto env) {
    constexpr int ENV = decltype(env)::value;
    if (rec) hipLaunchKernelGGL((actor_ensemble_kernel<ENV, true>), grid, block, 0, stream, P, A);
    else hipLaunchKernelGGL((actor_ensemble_kernel<ENV, false>), grid, block, 0, stream, P, A);
  });
  return hipGetLastError();
}

hipError_t launch_evaluate_actor_ensemble(const DevParams &P, const ActorEnsembleArgs &A, hipStream_t stream) { return launch_actor_ensemble(P, A, false, stream); }
hipError_t launch_trajectory_actor_ensemble(const DevParams &P, const ActorEnsembleArgs &A, hipStream_t stream) { return launch_actor_ensemble(P, A, true, stream); }

} // namespace grlx
