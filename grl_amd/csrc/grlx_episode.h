// grlx_episode.h -- what the evaluation kernels share: the device helpers of an episode's step (the probe of a 16-lane group, the read,
// findmax, the bookkeeping, the head of a trajectory record) and the host-side dispatch over the instantiations.  Included by
// grlx_evaluate.hip and the units of the evaluation variants beside it, after grlx_envs.h and grlx_query_weights.h; no rollout kernel
// sees it.
//
// Every function here is inlined, and every kernel that calls one is instruction for instruction the kernel that carried the lines
// itself (profiles/evaluate_shared_helpers_isa_diff.txt).  Three kernels do NOT call what they could and keep their own lines, each under
// a comment that names the function mirrored: evaluate_q_kernel (member_probe, findmax, action_of) and evaluate_ac_kernel and
// trajectory_ac_kernel (actor_probe, read_actor) -- calling the helper changes their machine code, and this header
// exists to remove copies, not to change kernels.  For the same reason the episode loop of the unit whose sampler draws the actions keeps
// episode_account's and episode_store's lines on a struct of its own (see there).
#pragma once
#include <type_traits>
#include "grlx_evaluate.h"

namespace grlx {

// what a group carries through the loop besides the model state; ties: the Q agents' (a kernel that never passes a tie carries a constant)
struct EpisodeSums {
  double ret, disc, g;
  int steps, code, ties;
};

// one step's bookkeeping (online_learning.cpp:202; disc += g * reward; g = g * gamma); returns whether the episode goes on
__device__ __forceinline__ bool episode_account(EpisodeSums &e, double reward, double gamma, int terminal, uint32_t status, bool tie)
{
  e.ret += reward;
  e.disc += e.g * reward;
  e.g = e.g * gamma;
  e.steps++;
  e.ties += tie ? 1 : 0;
  e.code = (status & ST_DOMAIN) ? kEvaluateDomain : terminal;
  return e.code == 0;
}

template <int S>
__device__ __forceinline__ void episode_store(const EvaluateArgs &A, long long pair, const EpisodeSums &e, const double (&x)[S])
{
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
#pragma unroll
  for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
}

// The probe of one Q member by its 16-lane group: project(obs, a_k), k < NA -- the hash of the observation once, then the action's
// coordinate and the tiling (tile_coding.cpp:103-149) --, query_weights, the lane's NA weights into its column of the wave's tile.
template <int ENV, int NA>
__device__ __forceinline__ void member_probe(const DevParams &P, const Table &tab, const ReplicaState &rs,
                                             const double (&obs)[Env<ENV>::D], int j, int lane, double *W)
{
  constexpr int T = kLanesPerReplica, D = Env<ENV>::D;
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

// the lane's weight of the actor's read at obs into the wave's tile: project(obs) of the actor's projector (tile_coding.cpp:103-149),
// unrolled over the observation (tile_slot_generic's run-time index would put obs into scratch), and the peek-only probe
template <int ENV>
__device__ __forceinline__ void actor_probe(const DevParams &P, const Table &tab, const ReplicaState &rs, const double (&obs)[Env<ENV>::D], int j, int lane, double *W)
{
  constexpr int D = Env<ENV>::D;
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

// LinearRepresentation::read (linear.cpp:136-184) of the 16 weights that begin at W[first]: serial sum over the tilings, mean
__device__ __forceinline__ double tilings_mean(const double *W, int first)
{
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) sum += W[first + k];
  return sum / 16;
}

// Q(obs, a_j) by lane j < NA of group g: the read and the representation's clamp
__device__ __forceinline__ double member_q(const DevParams &P, const double *W, int g, int j)
{
  return query_clamp(tilings_mean(W, j * kRowStride + g * 16), P.lin.out_min, P.lin.out_max);
}

// ActionPolicy::read (action.cpp:99-112) of group g: the actor's read and its clamp, before the clip of act
__device__ __forceinline__ double read_actor(const DevParams &P, const double *W, int g)
{
  return query_clamp(tilings_mean(W, g * 16), P.lin_actor.out_min, P.lin_actor.out_max);
}

// GreedySampler::findmax (greedy.cpp:47-61): the first maximum and the number of maxima
template <int NA, class V>
__device__ __forceinline__ void findmax(const V *v, int &mai, int &man)
{
  mai = 0; man = 1;
  V best = v[0];
#pragma unroll
  for (int a = 1; a < NA; ++a)
  {
    const V q = v[a];
    if (q > best) { best = q; mai = a; man = 1; }
    else if (q == best) man++;
  }
}

// actions[mai] by selects, not an indexed read of the parameter block: no scratch copy of it
template <int NA>
__device__ __forceinline__ double action_of(const DevParams &P, int mai)
{
  double action = P.actions[0];
#pragma unroll
  for (int a = 1; a < NA; ++a) action = (mai == a) ? P.actions[a] : action;
  return action;
}

// Word w of a step's single-policy record (include/grlx.h: GRLX_TRAJ_*), by selects over the values themselves: no array of the words is
// formed (one that was went to scratch, although only constants indexed it after unrolling).  The head every record begins with: the
// GRLX_TRAJ_OBS + D + S words up to the model state; a unit whose record goes on applies its own selects to the result.  Any w outside
// the head gives the action.
template <int D, int S>
__device__ __forceinline__ double record_head(int w, double action, double reward, double value, int mai, int man, int code,
                                              const double (&obs)[D], const double (&x)[S])
{
  double out = action;
  out = (w == GRLX_TRAJ_REWARD) ? reward : out;
  out = (w == GRLX_TRAJ_VALUE) ? value : out;
  out = (w == GRLX_TRAJ_ACTION_INDEX) ? (double)mai : out;
  out = (w == GRLX_TRAJ_N_MAX) ? (double)man : out;
  out = (w == GRLX_TRAJ_TERMINAL) ? (double)code : out;
#pragma unroll
  for (int i = 0; i < D; ++i) out = (w == GRLX_TRAJ_OBS + i) ? obs[i] : out;
#pragma unroll
  for (int i = 0; i < S; ++i) out = (w == GRLX_TRAJ_OBS + D + i) ? x[i] : out;
  return out;
}

// lane j < 16 of a group writes its words of the single-policy record at rec: word j, and word j + 16 where the record has one
// (trajectory_q_kernel, trajectory_ac_kernel and their streamed twins in grlx_evaluate_stream.hip)
template <int D, int S>
__device__ __forceinline__ void record_store16(double *rec, int j, double action, double reward, double value, int mai, int man, int code,
                                               const double (&obs)[D], const double (&x)[S])
{
  constexpr int R = GRLX_TRAJ_OBS + D + S;
  if (j < R) rec[j] = record_head<D, S>(j, action, reward, value, mai, man, code, obs, x);
  if constexpr (R > 16)
    if (j + 16 < R) rec[j + 16] = record_head<D, S>(j + 16, action, reward, value, mai, man, code, obs, x);
}

// ---- host: the instantiations ------------------------------------------------------------------------------------------------------------
// The grid of the single-policy kernels: a 16-lane group per (replica, start state) pair, four pairs per wave
inline unsigned pair_blocks(const EvaluateArgs &A)
{
  const long long pairs = (long long)A.n_replicas * A.n_starts;
  return (unsigned)((pairs + 4 * kQueryWaves - 1) / (4 * kQueryWaves));
}

// f(environment, action count), both std::integral_constant, for the (ENV, NA) of a Q context that evaluate_built admits -- the one
// statement of which pairs exist; the caller has asked it.  A kernel template named in f is instantiated for exactly these five pairs.
template <class F>
void with_q_instance(const DevParams &P, F &&f)
{
  using std::integral_constant;
  if (P.env == GRLX_ENV_PENDULUM && P.A == 3) f(integral_constant<int, GRLX_ENV_PENDULUM>{}, integral_constant<int, 3>{});
  else if (P.env == GRLX_ENV_PENDULUM) f(integral_constant<int, GRLX_ENV_PENDULUM>{}, integral_constant<int, 5>{});
  else if (P.env == GRLX_ENV_ACROBOT) f(integral_constant<int, GRLX_ENV_ACROBOT>{}, integral_constant<int, 3>{});
  else if (P.env == GRLX_ENV_CART_POLE) f(integral_constant<int, GRLX_ENV_CART_POLE>{}, integral_constant<int, 3>{});
  else f(integral_constant<int, GRLX_ENV_COMPASS_WALKER>{}, integral_constant<int, 3>{});
}

// f(environment) for the actor-critic's two
template <class F>
void with_ac_instance(const DevParams &P, F &&f)
{
  if (P.env == GRLX_ENV_CART_POLE) f(std::integral_constant<int, GRLX_ENV_CART_POLE>{});
  else f(std::integral_constant<int, GRLX_ENV_PENDULUM>{});
}

} // namespace grlx
