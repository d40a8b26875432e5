// grlx_evaluate_ensemble_sampled.hip -- sampled ensemble episodes (grlx_evaluate_ensemble_sampled, grlx_evaluate_ensemble_sampled_trajectory):
// one episode per (group of G consecutive Q replicas, start state); the members share ONE environment state, and at every step the action
// is DRAWN from the distribution the reference's discrete ensemble builds -- softmax(votes / tau) under majority voting, the softmax of
// the members' summed ranks under rank voting -- on one rand48 stream the episode carries.  Reference: DiscreteMultiPolicy::act and
// ::distribution (multi_discrete.cpp:88-105, 201-281), SoftmaxSampler::distribution (softmax.cpp:65-110), GreedySampler:: and
// EpsilonGreedySampler::distribution (greedy.cpp:88-98, 229-236), grl::sample (utils.h:227-250); include/grlx.h states the step as a
// serial loop and what differs.
//
// A unit of its own beside grlx_evaluate.hip.  The probe, the read, findmax, the action select and the bookkeeping are grlx_episode.h's;
// what is below is this unit's alone: the members' distributions, the reduction of the scores, the draw, the store and the record.
//
// Layout: evaluate_ensemble_kernel's frame.  One block of kQueryWaves waves serves one episode; its 16 lane groups probe 16 members per
// round, ceil(G / 16) rounds per step; every thread integrates the same state, so the episode's end is block-uniform and no action is
// handed back.  What differs is everything between the probe and the action:
//
//   1. A member's work stays in the lane group that summed its Q.  Lane j < NA of the group holds q_m[j] in a register; the NA values
//      travel among the group's lanes by ds_bpermute (gather), never through LDS.  Each entry of the member's distribution d_m is computed
//      ONCE, by the lane that owns the action: under the SOFTMAX member that is one pexp per (member, action) in the whole block, where
//      evaluate_ensemble_kernel's walk over all member slots would put G * NA of them into every thread.  The entries are gathered again
//      and every lane of the group scans them for the member's vote; lane j counts the entries below its own for the rank of action j.
//   2. The scores are integers, so their sums are exact in any order and the members need no serial pass.  Within a wave: one __ballot
//      per action over the groups' lead lanes, counted by __popcll, for the votes; one more for the members with a tie; two __shfl_xor adds
//      over the four groups for the ranks.  Across the waves: lanes 0 ... NA - 1 of each wave add the wave's counts to the step's
//      accumulator in LDS (ds_add), one add per wave, action and round.
//   3. ONE block barrier per step, after the last round -- the rounds need none, no thread reads another wave's result before it.  Then
//      every thread reads the 2 NA + 1 integers (broadcast reads), converts them and evaluates the combined softmax and the draw itself:
//      NA exponentials per step and thread, identical bits in every thread, and every thread advances the same rand48 state.
//   4. agreement needs the action, which is known only after the draw: the per-action vote counts are kept beside the rank sums (under
//      MAJORITY they are the score itself) and votes[action] is added.
//
// LDS hazards.  A wave's tile W is written by member_probe and read by member_q of the same wave; a wave barrier stands between the two
// and another one between the reads and the next round's probe.  The accumulator sh_acc has THREE buffers, used in turn by step: buffer
// b = step % 3 receives the adds of step k before the step's block barrier and is read after it.  After that barrier threads 0 ... 15
// clear buffer (b + 2) % 3, which is the buffer of step k - 1 -- every thread finished reading it before it reached barrier k -- and of
// step k + 2, whose adds come after barrier k + 1, which the clearing threads reach after their stores.  Two buffers by the step's parity
// are not enough where a step has a single barrier (G <= 16): the clear of the other buffer would have to fall after the slowest wave's
// reads of step k - 1 and before the fastest wave's adds of step k + 1, and only barrier k separates those two.  All three buffers are
// cleared once before the loop, under a barrier of their own.  Dead member slots (member >= G: the partial last round) run the same
// instructions on zeros -- the exchanges are wave-wide -- and add nothing.
//
// Compiled with -ffp-contract=off like every unit: every quotient, product and sum of the distributions is a plain one.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_evaluate_ensemble_sampled.h"
#include "grlx_episode.h"

namespace grlx {
namespace ensemble_sampled {

constexpr int kVotes = 0, kRanks = 8, kMemberTies = 15, kAccWords = 16;      // the words of one accumulator buffer

// the NA values that lanes 0 ... NA - 1 of a 16-lane group hold, one each, into every lane of the group
template <int NA>
__device__ __forceinline__ void gather(double own, double (&v)[NA])
{
#pragma unroll
  for (int a = 0; a < NA; ++a) v[a] = __shfl(own, a, 16);
}

// v[i] for a run-time i in 0 ... NA - 1 by selects.  The chain starts from a constant and not from v[0]: a select between two array
// elements is rewritten into one load through a selected address, which keeps the whole array in memory (scratch, or LDS taken for it).
template <int NA, class V>
__device__ __forceinline__ V pick(const V (&v)[NA], int i)
{
  V out = 0;
#pragma unroll
  for (int a = 0; a < NA; ++a) out = (i == a) ? v[a] : out;
  return out;
}

// SoftmaxSampler::distribution's frame over the powers p: the least power kept (exclusive) and the center the exponentials are taken about
template <int NA>
__device__ __forceinline__ void softmax_frame(const double (&p)[NA], double &minp, double &center)
{
  double maxp = -0x1.fffffffffffffp+1023;                 // -DBL_MAX
#pragma unroll
  for (int a = 0; a < NA; ++a) maxp = (maxp < p[a]) ? p[a] : maxp;
  minp = maxp + (-100);
  center = (maxp + minp) / 2.0;
}

// softmax(v, t) shared out over a 16-lane group: lane j < NA owns v[j] and returns entry j of the distribution; one pexp per lane
template <int NA>
__device__ __forceinline__ double softmax_own(double v_own, double t)
{
  const double p_own = v_own / t;
  double p[NA], e[NA];
  gather<NA>(p_own, p);
  double minp, center;
  softmax_frame<NA>(p, minp, center);
  const bool kept = p_own > minp;
  const double e_own = kept ? pexp(p_own - center) : 0.0;
  gather<NA>(e_own, e);
  double sum = 0;
#pragma unroll
  for (int a = 0; a < NA; ++a) sum = (p[a] > minp) ? sum + e[a] : sum;
  return kept ? e_own / sum : 0.0;
}

// softmax(v, t) whole, in one thread: the combined distribution
template <int NA>
__device__ __forceinline__ void softmax_all(const double (&v)[NA], double t, double (&d)[NA])
{
  double p[NA], e[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) p[a] = v[a] / t;
  double minp, center;
  softmax_frame<NA>(p, minp, center);
  double sum = 0;
#pragma unroll
  for (int a = 0; a < NA; ++a)
  {
    e[a] = (p[a] > minp) ? pexp(p[a] - center) : 0.0;
    sum = (p[a] > minp) ? sum + e[a] : sum;
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) d[a] = (p[a] > minp) ? e[a] / sum : 0.0;
}

// entry j of member m's distribution, by the lane that owns action j; q: the member's Q-values (in every lane of the group), man: its
// number of maxima.  GREEDY: 1 / man on the maximal entries.  EPSILON: the greedy entry, 1 replaced by 1 - e, plus e / NA.
template <int NA>
__device__ __forceinline__ double member_entry(const double (&q)[NA], double q_own, int man, int member, double param)
{
  if (member == GRLX_MEMBER_SOFTMAX) return softmax_own<NA>(q_own, param);       // kernel argument: the exchanges inside are wave-uniform
  double best = q[0];
#pragma unroll
  for (int a = 1; a < NA; ++a) best = (q[a] > best) ? q[a] : best;
  double d = (q_own == best) ? 1. / (double)man : 0.;
  if (member == GRLX_MEMBER_EPSILON)
  {
    d = (d == 1) ? 1 - param : d;
    d += param / (double)NA;
  }
  return d;
}

// the member's vote (multi_discrete.cpp:218-229): the first entry strictly above every entry before it and above 0.0; NA - 1 without one
template <int NA>
__device__ __forceinline__ int vote_of(const double (&d)[NA])
{
  double best = 0.0;
  int idx = NA - 1;
#pragma unroll
  for (int a = 0; a < NA; ++a)
  {
    const bool up = d[a] > best;
    idx = up ? a : idx;
    best = up ? d[a] : best;
  }
  return idx;
}

// grl::sample (utils.h:227-250) on one drand48 of the episode's stream
template <int NA>
__device__ __forceinline__ int draw(const double (&dist)[NA], uint64_t &rng)
{
  double s = 0;
#pragma unroll
  for (int a = 0; a < NA; ++a) s += dist[a];
  rng = lcg_next(rng);
  const double r = lcg_double(rng) * s;
  double acc = 0;
  int at = NA - 1;
  bool found = false;
#pragma unroll
  for (int a = 0; a < NA; ++a)
  {
    acc += dist[a];
    const bool here = !found && r < acc;
    at = here ? a : at;
    found = found || here;
  }
  return at;
}

// Word w of a step's record: the ensemble trajectory's words in their order, then `explored` and the probability of the action taken.
// Any w outside the record gives the action.
template <int D, int S>
__device__ __forceinline__ double record_word(int w, double action, double reward, double value, int idx, int man, int code, int agree, int member_ties,
                                              bool explored, double prob, const double (&obs)[D], const double (&x)[S])
{
  constexpr int R = GRLX_TRAJ_ENS_OBS + D + S + 2;
  double out = action;
  out = (w == GRLX_TRAJ_REWARD) ? reward : out;
  out = (w == GRLX_TRAJ_VALUE) ? value : out;
  out = (w == GRLX_TRAJ_ACTION_INDEX) ? (double)idx : out;
  out = (w == GRLX_TRAJ_N_MAX) ? (double)man : out;
  out = (w == GRLX_TRAJ_TERMINAL) ? (double)code : out;
  out = (w == GRLX_TRAJ_ENS_AGREEMENT) ? (double)agree : out;
  out = (w == GRLX_TRAJ_ENS_MEMBER_TIES) ? (double)member_ties : out;
#pragma unroll
  for (int i = 0; i < D; ++i) out = (w == GRLX_TRAJ_ENS_OBS + i) ? obs[i] : out;
#pragma unroll
  for (int i = 0; i < S; ++i) out = (w == GRLX_TRAJ_ENS_OBS + D + i) ? x[i] : out;
  out = (w == R - 2) ? (explored ? 1.0 : 0.0) : out;
  out = (w == R - 1) ? prob : out;
  return out;
}

// thread 0 of the block writes the pair's outputs once, after the loop
template <int S>
__device__ __forceinline__ void store(const EnsembleSampledArgs &T, const EpisodeSums &e, long long member_ties, long long agreement, int explored,
                                      uint64_t rng, const double (&x)[S])
{
  const EnsembleArgs &A = T.e;
  const long long pair = blockIdx.x;                   // group * n_starts + start
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
  A.member_ties[pair] = member_ties;
  A.agreement[pair] = agreement;
  T.explored[pair] = explored;
  T.streams_out[pair] = rng;
#pragma unroll
  for (int i = 0; i < S; ++i) A.final_state[(size_t)pair * S + i] = x[i];
}

} // namespace ensemble_sampled

// REC: one record per step taken; threads 0 ... R - 1 of the block (all of wave 0) store one word each
template <int ENV, int NA, bool REC>
__global__ __launch_bounds__(kQueryWaves * 64) void ensemble_sampled_kernel(DevParams P, EnsembleSampledArgs T)
{
  using namespace ensemble_sampled;
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D, kSlots = kQueryWaves * 4, R = GRLX_TRAJ_ENS_OBS + D + S + 2;
  static_assert(R <= 64, "the record is stored by one wave");
  static_assert(NA <= kRanks && kRanks + NA <= kMemberTies, "an accumulator buffer holds the votes, the ranks and the members with a tie");
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ int sh_acc[3][kAccWords];
  const EnsembleArgs &A = T.e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int slot = wave * 4 + g;                       // the member of a round this lane group serves
  const int G = A.group_size, member = T.member;
  const bool rank = A.rule == GRLX_ENSEMBLE_RANK;
  const int grp = (int)(blockIdx.x / (unsigned)A.n_starts), s = (int)(blockIdx.x - (unsigned)grp * (unsigned)A.n_starts);
  const int r0 = A.first_replica + grp * G;
  double *W = sh_w[wave];
  double *rec = REC ? T.records + (size_t)blockIdx.x * (size_t)A.max_steps * R + threadIdx.x : nullptr;   // the thread's word of the first record

  const double gamma = A.sweep ? A.sweep[r0].gamma : P.gamma;      // the group's first replica's
  uint64_t rng = T.streams ? T.streams[blockIdx.x] : P.states[r0].G;
  double x[S], obs[D];
#pragma unroll
  for (int i = 0; i < S; ++i) x[i] = A.states[(size_t)s * S + i];
  (void)Env<ENV>::observe(P, x, obs);                  // the start state's terminal code is ignored, as Environment::start has none

  if (threadIdx.x < 3 * kAccWords) (&sh_acc[0][0])[threadIdx.x] = 0;
  __syncthreads();

  EpisodeSums e;
  e.ret = 0; e.disc = 0; e.g = 1; e.steps = 0; e.code = 0; e.ties = 0;
  long long member_ties = 0, agreement = 0;
  int explored = 0, buf = 0;
  bool active = true;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // block-uniform: every thread holds the same state
    int *ACC = sh_acc[buf];
    for (int m0 = 0; m0 < G; m0 += kSlots)
    {
      const bool is_member = m0 + slot < G;
      const int r = r0 + (is_member ? m0 + slot : 0);
      const ReplicaState &rs = P.states[r];
      if (is_member) member_probe<ENV, NA>(P, table_of(P, 0, r), rs, obs, j, lane, W);
      wave_sync();
      const double q_own = (is_member && j < NA) ? member_q(P, W, g, j) : 0.;
      wave_sync();                                     // the reads above come before the next round's weights
      double q[NA], d[NA];
      gather<NA>(q_own, q);
      int mai, man;
      findmax<NA>(q, mai, man);
      double param = T.member_param;
      if (member == GRLX_MEMBER_EPSILON && param < 0.)
        param = rs.eps_decay * (A.sweep ? A.sweep[r].epsilon : P.epsilon);      // GRLX_EPSILON_OWN: the member's own, read and never advanced
      const double d_own = member_entry<NA>(q, q_own, man, member, param);
      gather<NA>(d_own, d);
      const int vote = vote_of<NA>(d);
      const bool lead = is_member && j == 0;
      int n[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) n[a] = __popcll(__ballot(lead && vote == a));
      const int tied = __popcll(__ballot(lead && man > 1));
      int rk = 0;
      if (rank)
      { // the rank of action j among the member's entries: 1 + the entries strictly below it; summed over the wave's four groups
        int below = 1;
#pragma unroll
        for (int a = 0; a < NA; ++a) below += (d_own > d[a]) ? 1 : 0;
        rk = (is_member && j < NA) ? below : 0;
        rk += __shfl_xor(rk, 16, 64);
        rk += __shfl_xor(rk, 32, 64);
      }
      if (lane < NA)
      {
        atomicAdd(&ACC[kVotes + lane], pick<NA>(n, lane));
        if (rank) atomicAdd(&ACC[kRanks + lane], rk);
      }
      if (lane == 15) atomicAdd(&ACC[kMemberTies], tied);
    }
    __syncthreads();
    int votes[NA], score[NA];
    double sc[NA], dist[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
    {
      votes[a] = ACC[kVotes + a];
      score[a] = rank ? ACC[kRanks + a] : votes[a];
      sc[a] = (double)score[a];
    }
    const int step_ties = ACC[kMemberTies];
    const int clear = buf == 0 ? 2 : buf - 1;          // (buf + 2) % 3: the buffer of the step before, and of the step after the next
    if (threadIdx.x < kAccWords) sh_acc[clear][threadIdx.x] = 0;
    buf = buf == 2 ? 0 : buf + 1;
    softmax_all<NA>(sc, T.tau, dist);
    const int idx = draw<NA>(dist, rng);
    int mai, man;
    findmax<NA>(score, mai, man);
    const int agree = pick<NA>(votes, idx);
    const bool off = idx != mai;
    member_ties += step_ties;
    agreement += agree;
    explored += off ? 1 : 0;
    const double action = action_of<NA>(P, idx);
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
    active = episode_account(e, reward, gamma, terminal, status, man > 1);
    if constexpr (REC)
    {
      if (threadIdx.x < R)
        rec[(size_t)(e.steps - 1) * R] = record_word<D, S>((int)threadIdx.x, action, reward, pick<NA>(sc, idx), idx, man, e.code, agree, step_ties, off,
                                                          pick<NA>(dist, idx), before, x);
    }
  }
  if (threadIdx.x == 0) store<S>(T, e, member_ties, agreement, explored, rng, x);
}

int ensemble_sampled_trajectory_words(int env)
{
  const int words = trajectory_words(env, true);
  return words ? words + 2 : 0;
}

// one block per (group, start state).  Every output pointer of the kernels is written without a test, so all of them are required here.
static hipError_t launch_ensemble_sampled(const DevParams &P, const EnsembleSampledArgs &T, bool rec, hipStream_t stream)
{
  const EnsembleArgs &A = T.e;
  if (A.group_size < 1 || A.n_replicas % A.group_size != 0) return hipErrorInvalidValue;
  const long long blocks = (long long)(A.n_replicas / A.group_size) * A.n_starts;
  if (blocks == 0) return hipSuccess;
  const bool member_ok = T.member == GRLX_MEMBER_GREEDY || (T.member == GRLX_MEMBER_EPSILON && (T.member_param == GRLX_EPSILON_OWN || (T.member_param >= 0. && T.member_param <= 1.))) ||
                         (T.member == GRLX_MEMBER_SOFTMAX && T.member_param > 0. && T.member_param < __builtin_inf());
  if (P.agent == GRLX_AGENT_AC || !evaluate_built(P.agent, P.env, P.A) || A.max_steps < 1 || blocks > 0x7fffffffll || (rec && !T.records) ||
      (A.rule != GRLX_ENSEMBLE_MAJORITY && A.rule != GRLX_ENSEMBLE_RANK) || !member_ok || !(T.tau > 0. && T.tau < __builtin_inf()) ||
      !T.streams_out || !T.explored || !A.states || !A.ret || !A.disc || !A.steps || !A.terminal || !A.ties || !A.member_ties || !A.agreement ||
      !A.final_state)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kQueryWaves * 64);
  with_q_instance(P, [&](auto env, auto na) {
    constexpr int ENV = decltype(env)::value, NA = decltype(na)::value;
    if (rec) hipLaunchKernelGGL((ensemble_sampled_kernel<ENV, NA, true>), grid, block, 0, stream, P, T);
    else hipLaunchKernelGGL((ensemble_sampled_kernel<ENV, NA, false>), grid, block, 0, stream, P, T);
  });
  return hipGetLastError();
}

hipError_t launch_evaluate_ensemble_sampled(const DevParams &P, const EnsembleSampledArgs &A, hipStream_t stream) { return launch_ensemble_sampled(P, A, false, stream); }
hipError_t launch_trajectory_ensemble_sampled(const DevParams &P, const EnsembleSampledArgs &A, hipStream_t stream) { return launch_ensemble_sampled(P, A, true, stream); }

} // namespace grlx
