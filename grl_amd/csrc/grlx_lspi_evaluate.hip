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
#include "grlx_lspi_quad.h"
#include "grlx_episode.h"

namespace grlx {

constexpr int kLspiLdsMembers = 8;         // -DGRLX_LSPI_ENS_LDS: the largest group whose weights are staged (8 x 512 doubles = 32 KB)

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
