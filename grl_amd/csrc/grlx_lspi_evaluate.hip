// grlx_lspi_evaluate.hip -- the LSPI context's read side beyond the plain query: greedy evaluation episodes from model states of the
// caller's choice, their per-step records, and the same over groups of replicas (grlx_lspi_evaluate, grlx_lspi_evaluate_trajectory,
// grlx_lspi_query_ensemble, grlx_lspi_evaluate_ensemble, grlx_lspi_evaluate_ensemble_trajectory).  The specification of a read is S3-S5
// and D2-D5 of grlx_lspi.h, restated by lspi_read (grlx_lspi_read.h), which lspi_query_kernel and lspi_test_kernel call; every kernel
// here produces lspi_read's bits by other means, and tests/test_gpu_lspi_evaluate.py holds them to that.
//
// Shape of the work.  A call is a few thousand episodes of about 100 serial steps: far too few lanes to fill the device, so the LENGTH of
// one step sets the call's time.  lspi_read walks all F basis functions per action under Gauss and recomputes everything per action; one
// lane per episode, as the test trial runs, would pay action_steps x that per step.  Here:
//
//   A QUAD of four lanes per episode.  Lane a of the quad computes the reads of the actions a, a + 4 (kLspiOwn slots).  The values are
//   exchanged inside the quad by DPP (quad_perm broadcasts: no LDS, no barrier), after which EVERY lane runs findmax over k ascending and
//   the model step redundantly -- the same bits in all four by construction, no divergence inside a quad.  The words of a record are
//   shared out over the quad (words a, a + 4, a + 8, ...).
//
//   A block of 256 threads is 64 episodes of ONE replica: grid (ceil(n_starts / 64), n_replicas).  The replica's F weights are staged
//   into LDS once; one barrier before the loop, none inside.  Quads beyond n_starts are inactive; an episode that ends early idles
//   until its wave's longest ends (the loop is wave-uniform: it runs while a ballot finds an active lane).
//
//   Triangle.  What does not depend on the action is formed once per step: gridpos / cell / dist of the two observation dimensions and
//   the four corner products (1 * f0) * f1 -- S3 multiplies over dd ascending, so these are the reference's own partial products.  The
//   action dimension's cell and dist are constants of (context, action), formed once before the loop by the same operations.  Per action
//   and step 8 multiplications, 8 LDS reads and the 8 products and sums of S5 remain, in the ii order.
//
//   Gauss.  A basis function is kept only where distsq < cutoff_distsq (D4), which needs every |base_d + k_d| below the root of that
//   bound.  Per dimension k_d is bounded by an integer range that is conservative (lspi_box) and clamped to the grid; only that box is
//   visited, in index order (k2, k1, k0 innermost), and D4's exact test is applied inside it by lspi_gauss itself.  The same pairs in
//   the same order: the same bits, from about 75 candidates per read at the reference's file instead of 363.
//
//   Ensemble.  The same quad and block, a block per 64 episodes of one GROUP, the members walked in ascending order; sumq[k] lives in
//   the lane that owns action k, the vote needs one quad exchange per member.  The members' weights are read through their
//   block-uniform base address from global memory (L2): nothing is staged.
//
// Two builds exist for measurement only (tools/lspi_evaluate_throughput.py), never in the library the package
// loads: -DGRLX_LSPI_EVAL_FULL_WALK makes lspi_box give the whole grid (lspi_read's walk inside the same kernel), and
// -DGRLX_LSPI_ENS_LDS stages a group of up to kLspiLdsMembers members' weights into LDS before the loop.
//
// Nothing is indexed at run time by a lane's value: the lane's actions, the chosen action and the votes are selects.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_lspi.h"
#include "grlx_lspi_read.h"
#include "grlx_lspi_evaluate.h"
#include "grlx_episode.h"

namespace grlx {

constexpr int kLspiLdsMembers = 8;         // -DGRLX_LSPI_ENS_LDS: the largest group whose weights are staged (8 x 512 doubles = 32 KB)

// ------------------------------------------------------------------------------------------ the quad ---
// v of lane SRC of the caller's quad, in every lane of it (v_mov_b32 with quad_perm:[SRC, SRC, SRC, SRC], twice)
template <int SRC>
__device__ __forceinline__ double quad_bcast(double v)
{
  constexpr int ctrl = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  int lo = (int)(unsigned)b, hi = (int)(unsigned)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// all[k] = own[k / 4] of lane k % 4: the values of all action slots, in every lane of the quad.  Every lane of the quad must be here.
__device__ __forceinline__ void quad_exchange(const double (&own)[kLspiOwn], double (&all)[kMaxActions])
{
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o)
  {
    all[4 * o + 0] = quad_bcast<0>(own[o]);
    all[4 * o + 1] = quad_bcast<1>(own[o]);
    all[4 * o + 2] = quad_bcast<2>(own[o]);
    all[4 * o + 3] = quad_bcast<3>(own[o]);
  }
}

// findmax (grlx_episode.h) over the first A of kMaxActions values, A uniform: the first maximum, the number of maxima, the maximum
__device__ __forceinline__ void lspi_findmax(const double (&v)[kMaxActions], int A, int &mai, int &man, double &best)
{
  mai = 0; man = 1;
  best = v[0];
#pragma unroll
  for (int a = 1; a < kMaxActions; ++a)
    if (a < A)
    {
      if (v[a] > best) { best = v[a]; mai = a; man = 1; }
      else if (v[a] == best) man++;
    }
}

__device__ __forceinline__ double lspi_action_of(const LspiParams &L, int k)
{
  double action = L.actions[0];
#pragma unroll
  for (int a = 1; a < kMaxActions; ++a) action = (k == a) ? L.actions[a] : action;
  return action;
}

// ------------------------------------------------------------------------------------------ the lane's actions ---
// what a lane keeps about the action slots it owns (actions a + 4 o below action_steps), formed once before the loop
template <int PROJ> struct LspiActs;
template <> struct LspiActs<GRLX_RBF_TRIANGLE> {
  bool   has[kLspiOwn];
  int    off[kLspiOwn];                    // cell of the action dimension x its stride
  double d[kLspiOwn], omd[kLspiOwn];       // dist of the action dimension, and 1 - dist
};
template <> struct LspiActs<GRLX_RBF_GAUSS> {
  bool   has[kLspiOwn];
  double base2[kLspiOwn];                  // lspi_gauss_base's third component
  int    lo2[kLspiOwn], hi2[kLspiOwn];     // lspi_box of the action dimension
  double rad;
};

// The range [lo, hi] of k outside which |base + k| < sqrt(cutoff_distsq) cannot hold, clamped to the grid (lo > hi: nothing is kept).
// rad is that root widened by 1e-9, relatively and absolutely: a kept function has fl(d * d) < cutoff_distsq for d = fl(base + k), so
// |base + k| < root (1 + 2^-53) + ulp(base) / 2, and |base| stays below 2^17 / delta < 2^20, whose ulp is 2^-32; forming -base -+ rad
// errs by as much again.  Both are far inside the widening, and floor / ceil only move the bounds further out.
__device__ __forceinline__ void lspi_box(double base, double rad, int steps, int &lo, int &hi)
{
  const double top = (double)(steps - 1);
#ifdef GRLX_LSPI_EVAL_FULL_WALK
  base = -0.5 * top; rad = top;            // measurement build: every k of the grid
#endif
  lo = (int)fmin(fmax(floor(-base - rad), 0.), top + 1);
  hi = (int)fmax(fmin(ceil(-base + rad), top), -1.);
}

template <int PROJ>
__device__ __forceinline__ void lspi_acts(const LspiParams &L, int a, LspiActs<PROJ> &act)
{
  if constexpr (PROJ == GRLX_RBF_GAUSS) act.rad = sqrt(L.cutoff_distsq) * (1 + 1e-9) + 1e-9;
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o)
  {
    const int k = a + kLspiQuad * o;
    act.has[o] = k < L.A;
    const double ak = lspi_action_of(L, k);
    if constexpr (PROJ == GRLX_RBF_TRIANGLE)
    { // lspi_triangle's dd = 2
      const double gridpos = fmin(fmax((ak - L.in_min[2]) / L.delta[2], 0.), L.top[2]);
      const int v = (int)gridpos;
      act.off[o] = v * L.stride[2];
      act.d[o] = gridpos - v;
      act.omd[o] = 1 - act.d[o];
    }
    else
    { // lspi_gauss_base's dd = 2
      act.base2[o] = (L.in_min[2] - ak) / L.delta[2];
      lspi_box(act.base2[o], act.rad, L.steps[2], act.lo2[o], act.hi2[o]);
    }
  }
}

// ------------------------------------------------------------------------------------------ the reads ---
// q[o] = the read of S5 at (obs, the lane's action o) on the weights w; slots the lane does not own stay 0.  w: LDS (the single
// policy) or global (a member of a group).
template <int PROJ>
__device__ __forceinline__ void lspi_quad_reads(const LspiParams &L, const LspiActs<PROJ> &act, const double (&obs)[kLspiD], const double *w,
                                                double (&q)[kLspiOwn])
{
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o) q[o] = 0;
  if constexpr (PROJ == GRLX_RBF_TRIANGLE)
  {
    // lspi_triangle's dd = 0, 1 and the products over them, once for all actions
    int index = 0;
    double dist[kLspiD];
#pragma unroll
    for (int dd = 0; dd < kLspiD; ++dd)
    {
      const double gridpos = fmin(fmax((obs[dd] - L.in_min[dd]) / L.delta[dd], 0.), L.top[dd]);
      const int v = (int)gridpos;
      index += v * L.stride[dd];
      dist[dd] = gridpos - v;
    }
    double c[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
    {
      double p = 1;
#pragma unroll
      for (int dd = 0; dd < kLspiD; ++dd) p *= (ii & (1 << dd)) ? dist[dd] : (1 - dist[dd]);
      c[ii] = p;
    }
#pragma unroll
    for (int o = 0; o < kLspiOwn; ++o)
      if (act.has[o])
      {
#pragma unroll
        for (int ii = 0; ii < 8; ++ii)
        {
          const int id = index + act.off[o] + ((ii & 1) ? L.stride[0] : 0) + ((ii & 2) ? L.stride[1] : 0) + ((ii & 4) ? L.stride[2] : 0);
          const double wt = c[ii & 3] * ((ii & 4) ? act.d[o] : act.omd[o]);
          q[o] += w[id] * wt;
        }
      }
  }
  else
  {
    int lo0, hi0, lo1, hi1;
    const double b0 = (L.in_min[0] - obs[0]) / L.delta[0], b1 = (L.in_min[1] - obs[1]) / L.delta[1];      // lspi_gauss_base's dd = 0, 1
    lspi_box(b0, act.rad, L.steps[0], lo0, hi0);
    lspi_box(b1, act.rad, L.steps[1], lo1, hi1);
    const int s0 = L.steps[0], s01 = L.steps[0] * L.steps[1];
#pragma unroll
    for (int o = 0; o < kLspiOwn; ++o)
      if (act.has[o])
      {
        const double base[kLspiNIn] = {b0, b1, act.base2[o]};
        for (int k2 = act.lo2[o]; k2 <= act.hi2[o]; ++k2)
          for (int k1 = lo1; k1 <= hi1; ++k1)
            for (int k0 = lo0; k0 <= hi0; ++k0)
            {
              const double g = lspi_gauss(L, base, k0, k1, k2);
              if (g >= 0.) q[o] += w[k2 * s01 + k1 * s0 + k0] * g;
            }
      }
  }
}

// ------------------------------------------------------------------------------------------ records ---
// lane a's words of a step's record: a, a + 4, a + 8, ...
__device__ __forceinline__ void lspi_record_store(double *rec, int a, double action, double reward, double value, int mai, int man, int code,
                                                  const double (&obs)[kLspiD], const double (&x)[kLspiS])
{
#pragma unroll
  for (int w0 = 0; w0 < kLspiTrajWords; w0 += kLspiQuad)
    if (w0 + a < kLspiTrajWords) rec[w0 + a] = record_head<kLspiD, kLspiS>(w0 + a, action, reward, value, mai, man, code, obs, x);
}

// the ensemble's record: record_head's words with the step's agreement and member ties before the observation
__device__ __forceinline__ void lspi_ens_record_store(double *rec, int a, double action, double reward, double value, int mai, int man, int code, int agree,
                                                      int mties, const double (&obs)[kLspiD], const double (&x)[kLspiS])
{
#pragma unroll
  for (int w0 = 0; w0 < kLspiEnsTrajWords; w0 += kLspiQuad)
  {
    const int w = w0 + a;
    const int hw = w >= GRLX_TRAJ_ENS_OBS ? w - (GRLX_TRAJ_ENS_OBS - GRLX_TRAJ_OBS) : (w >= GRLX_TRAJ_OBS ? 0 : w);
    double out = record_head<kLspiD, kLspiS>(hw, action, reward, value, mai, man, code, obs, x);
    out = (w == GRLX_TRAJ_ENS_AGREEMENT) ? (double)agree : out;
    out = (w == GRLX_TRAJ_ENS_MEMBER_TIES) ? (double)mties : out;
    if (w < kLspiEnsTrajWords) rec[w] = out;
  }
}

// behind an episode's end: all-zero bits up to max_steps, a quarter per lane
template <int R>
__device__ __forceinline__ void lspi_record_zeros(double *rec, int a, int steps, int max_steps)
{
  for (size_t k = (size_t)steps * R + (size_t)a; k < (size_t)max_steps * R; k += kLspiQuad) rec[k] = 0.;
}

// ------------------------------------------------------------------------------------------ the single policy ---
template <int PROJ, bool RECORD>
__global__ __launch_bounds__(kLspiEvalBlock) void lspi_evaluate_kernel(LspiParams L, LspiEvalArgs A)
{
  constexpr int R = kLspiTrajWords;
  __shared__ double sw[kLspiMaxF];
  const int rl = blockIdx.y, tid = threadIdx.x, a = tid & (kLspiQuad - 1);
  const double *w = L.w + (size_t)(A.first_replica + rl) * 2 * L.Fp;
  for (int k = tid; k < L.F; k += kLspiEvalBlock) sw[k] = w[k];
  __syncthreads();
  const int s = (int)blockIdx.x * kLspiEvalQuads + (tid >> 2);
  const bool live = s < A.n_starts;                    // the quads past the chunk's end neither load nor store
  const size_t pair = (size_t)rl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kLspiS], obs[kLspiD];
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) x[i] = live ? A.states[(size_t)s * kLspiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(L.env, x, obs);                // the start state's terminal code is ignored
  LspiActs<PROJ> act;
  lspi_acts<PROJ>(L, a, act);

  EpisodeSums e = {0., 0., 1., 0, 0, 0};
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    double own[kLspiOwn], q[kMaxActions], best;
    lspi_quad_reads<PROJ>(L, act, obs, sw, own);
    quad_exchange(own, q);
    int mai, man;
    lspi_findmax(q, L.A, mai, man, best);
    if (active)
    {
      const double action = lspi_action_of(L, mai);
      double before[kLspiD];
#pragma unroll
      for (int i = 0; i < kLspiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(L.env, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, L.gamma_tau, terminal, status, man > 1);
      if constexpr (RECORD) lspi_record_store(rec + (size_t)(e.steps - 1) * R, a, action, reward, best, mai, man, e.code, before, x);
    }
  }
  if (!live) return;
  if constexpr (RECORD) lspi_record_zeros<R>(rec, a, e.steps, A.max_steps);
  if (a != 0) return;
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) A.final_state[pair * kLspiS + i] = x[i];
}

// ------------------------------------------------------------------------------------------ the ensemble ---
// One observation under a group: the members [0, G) at `nets + m * pitch` in ascending order; q_m by lspi_quad_reads, (mai_m, man_m) by
// findmax, votes[mai_m] += 1, sumq[k] += q_m[k] in the lane that owns k, mties += man_m > 1.  visit(q_m, best_m, man_m) sees every member.
template <int PROJ, class V>
__device__ __forceinline__ void lspi_members(const LspiParams &L, const LspiActs<PROJ> &act, const double (&obs)[kLspiD], const double *nets, size_t pitch,
                                             int G, int (&votes)[kMaxActions], double (&sumq)[kLspiOwn], int &mties, V &&visit)
{
#pragma unroll
  for (int k = 0; k < kMaxActions; ++k) votes[k] = 0;
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o) sumq[o] = 0.;
  mties = 0;
  for (int m = 0; m < G; ++m)                          // uniform: every lane of a quad is at the exchange
  {
    double own[kLspiOwn], q[kMaxActions], best;
    int mai, man;
    lspi_quad_reads<PROJ>(L, act, obs, nets + (size_t)m * pitch, own);
#pragma unroll
    for (int o = 0; o < kLspiOwn; ++o) sumq[o] += own[o];
    quad_exchange(own, q);
    lspi_findmax(q, L.A, mai, man, best);
#pragma unroll
    for (int k = 0; k < kMaxActions; ++k) votes[k] += (mai == k) ? 1 : 0;
    mties += man > 1 ? 1 : 0;
    visit(q, best, man);
  }
}

template <int PROJ, bool RECORD>
__global__ __launch_bounds__(kLspiEvalBlock) void lspi_evaluate_ensemble_kernel(LspiParams L, LspiEnsArgs A)
{
  constexpr int R = kLspiEnsTrajWords;
  const int gl = blockIdx.y, G = A.group_size, tid = threadIdx.x, a = tid & (kLspiQuad - 1);
  const double *nets = L.w + (size_t)(A.first_replica + gl * G) * 2 * L.Fp;       // member m: nets + m * pitch, its current weights
  size_t pitch = 2 * (size_t)L.Fp;
#ifdef GRLX_LSPI_ENS_LDS
  __shared__ double sg[kLspiLdsMembers * kLspiMaxF];   // measurement build: a group that fits is staged, one barrier before the loop
  if (G <= kLspiLdsMembers)
  {
    for (int k = tid; k < G * L.Fp; k += kLspiEvalBlock) sg[k] = nets[(size_t)(k / L.Fp) * pitch + (size_t)(k % L.Fp)];
    __syncthreads();
    nets = sg;
    pitch = (size_t)L.Fp;
  }
#endif
  const int s = (int)blockIdx.x * kLspiEvalQuads + (tid >> 2);
  const bool live = s < A.n_starts;
  const size_t pair = (size_t)gl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kLspiS], obs[kLspiD];
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) x[i] = live ? A.states[(size_t)s * kLspiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(L.env, x, obs);                // the start state's terminal code is ignored
  LspiActs<PROJ> act;
  lspi_acts<PROJ>(L, a, act);
  const bool vote = A.rule == GRLX_ENSEMBLE_VOTE;

  EpisodeSums e = {0., 0., 1., 0, 0, 0};
  long long member_ties = 0, agreement = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    int votes[kMaxActions], mties;
    double sumq[kLspiOwn], score[kMaxActions], best;
    lspi_members<PROJ>(L, act, obs, nets, pitch, G, votes, sumq, mties, [](const double (&)[kMaxActions], double, int) {});
    quad_exchange(sumq, score);
#pragma unroll
    for (int k = 0; k < kMaxActions; ++k) score[k] = vote ? (double)votes[k] : score[k];
    int mai, man, agree = votes[0];
    lspi_findmax(score, L.A, mai, man, best);
#pragma unroll
    for (int k = 1; k < kMaxActions; ++k) agree = (mai == k) ? votes[k] : agree;
    if (active)
    {
      const double action = lspi_action_of(L, mai);
      double before[kLspiD];
#pragma unroll
      for (int i = 0; i < kLspiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(L.env, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, L.gamma_tau, terminal, status, man > 1);
      member_ties += mties;
      agreement += agree;
      if constexpr (RECORD)
        lspi_ens_record_store(rec + (size_t)(e.steps - 1) * R, a, action, reward, best, mai, man, e.code, agree, mties, before, x);
    }
  }
  if (!live) return;
  if constexpr (RECORD) lspi_record_zeros<R>(rec, a, e.steps, A.max_steps);
  if (a != 0) return;
  A.ret[pair] = e.ret;
  A.disc[pair] = e.disc;
  A.steps[pair] = e.steps;
  A.terminal[pair] = e.code;
  A.ties[pair] = e.ties;
  A.member_ties[pair] = member_ties;
  A.agreement[pair] = agreement;
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) A.final_state[pair * kLspiS + i] = x[i];
}

// a quad per (group, observation), blockIdx.y the group: grlx_query_ensemble's columns, every sum over the members in ascending order
// into one accumulator.  out[group][n_obs][2 + 2 A]
template <int PROJ>
__global__ __launch_bounds__(kLspiEvalBlock) void lspi_query_ensemble_kernel(LspiParams L, int first_replica, int group_size, const double *obs, int n_obs,
                                                                             double *out)
{
  const int gl = blockIdx.y, tid = threadIdx.x, a = tid & (kLspiQuad - 1);
  const int o = (int)blockIdx.x * kLspiEvalQuads + (tid >> 2);
  const bool live = o < n_obs;
  const double *nets = L.w + (size_t)(first_replica + gl * group_size) * 2 * L.Fp;
  double ob[kLspiD];
#pragma unroll
  for (int d = 0; d < kLspiD; ++d) ob[d] = live ? obs[(size_t)o * kLspiD + d] : 0.;
  LspiActs<PROJ> act;
  lspi_acts<PROJ>(L, a, act);
  int votes[kMaxActions], mties;
  double sumq[kLspiOwn], sums[kMaxActions], sv = 0, svv = 0;
  const int NA = L.A;
  lspi_members<PROJ>(L, act, ob, nets, 2 * (size_t)L.Fp, group_size, votes, sumq, mties, [&](const double (&q)[kMaxActions], double best, int man) {
    double v = 0;                                       // q.cpp:56-68 over greedy.cpp:88-98, as grlx_query_q forms it
#pragma unroll
    for (int k = 0; k < kMaxActions; ++k)
      if (k < NA) v += q[k] * (q[k] == best ? 1. / man : 0.);
    sv += v;
    svv += v * v;
  });
  quad_exchange(sumq, sums);
  if (!live || a != 0) return;
  double *row = out + ((size_t)gl * (size_t)n_obs + (size_t)o) * (size_t)(2 + 2 * NA);
  row[0] = sv;
  row[1] = svv;
#pragma unroll
  for (int k = 0; k < kMaxActions; ++k)
    if (k < NA)
    {
      row[2 + k] = sums[k];
      row[2 + NA + k] = (double)votes[k];
    }
}

// ------------------------------------------------------------------------------------------ launchers ---
hipError_t launch_lspi_evaluate(const LspiParams &L, const LspiEvalArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.n_starts + kLspiEvalQuads - 1) / kLspiEvalQuads), (unsigned)rows), block(kLspiEvalBlock);
  const bool tri = L.projector == GRLX_RBF_TRIANGLE;
  if (A.records)
  {
    if (tri) hipLaunchKernelGGL((lspi_evaluate_kernel<GRLX_RBF_TRIANGLE, true>), grid, block, 0, stream, L, A);
    else hipLaunchKernelGGL((lspi_evaluate_kernel<GRLX_RBF_GAUSS, true>), grid, block, 0, stream, L, A);
  }
  else
  {
    if (tri) hipLaunchKernelGGL((lspi_evaluate_kernel<GRLX_RBF_TRIANGLE, false>), grid, block, 0, stream, L, A);
    else hipLaunchKernelGGL((lspi_evaluate_kernel<GRLX_RBF_GAUSS, false>), grid, block, 0, stream, L, A);
  }
  return hipGetLastError();
}

hipError_t launch_lspi_evaluate_ensemble(const LspiParams &L, const LspiEnsArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.n_starts + kLspiEvalQuads - 1) / kLspiEvalQuads), (unsigned)rows), block(kLspiEvalBlock);
  const bool tri = L.projector == GRLX_RBF_TRIANGLE;
  if (A.records)
  {
    if (tri) hipLaunchKernelGGL((lspi_evaluate_ensemble_kernel<GRLX_RBF_TRIANGLE, true>), grid, block, 0, stream, L, A);
    else hipLaunchKernelGGL((lspi_evaluate_ensemble_kernel<GRLX_RBF_GAUSS, true>), grid, block, 0, stream, L, A);
  }
  else
  {
    if (tri) hipLaunchKernelGGL((lspi_evaluate_ensemble_kernel<GRLX_RBF_TRIANGLE, false>), grid, block, 0, stream, L, A);
    else hipLaunchKernelGGL((lspi_evaluate_ensemble_kernel<GRLX_RBF_GAUSS, false>), grid, block, 0, stream, L, A);
  }
  return hipGetLastError();
}

hipError_t launch_lspi_query_ensemble(const LspiParams &L, int first_replica, int groups, int group_size, const double *obs, int n_obs, double *out,
                                      hipStream_t stream)
{
  const dim3 grid((unsigned)((n_obs + kLspiEvalQuads - 1) / kLspiEvalQuads), (unsigned)groups), block(kLspiEvalBlock);
  if (L.projector == GRLX_RBF_TRIANGLE)
    hipLaunchKernelGGL(lspi_query_ensemble_kernel<GRLX_RBF_TRIANGLE>, grid, block, 0, stream, L, first_replica, group_size, obs, n_obs, out);
  else
    hipLaunchKernelGGL(lspi_query_ensemble_kernel<GRLX_RBF_GAUSS>, grid, block, 0, stream, L, first_replica, group_size, obs, n_obs, out);
  return hipGetLastError();
}

} // namespace grlx
