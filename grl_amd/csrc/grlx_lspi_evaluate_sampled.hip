// grlx_lspi_evaluate_sampled.hip -- the LSPI context's sampled episodes: one policy under the reference's samplers
// (grlx_lspi_evaluate_sampled, grlx_lspi_evaluate_sampled_trajectory) and the draw from a group's majority or rank votes
// (grlx_lspi_evaluate_ensemble_sampled, grlx_lspi_evaluate_ensemble_sampled_trajectory).  A read is S3-S5 and D2-D5 of grlx_lspi.h, as
// lspi_read (grlx_lspi_read.h) restates it; both kernels produce lspi_read's bits by other means, and tests/
// test_gpu_lspi_evaluate_sampled.py holds them to that.  The step after the read is the FQI siblings' (grlx_fqi.hip), as include/grlx.h
// states it.
//
// One policy: lspi_evaluate_kernel's quad per episode (grlx_lspi_evaluate.hip, its helpers in grlx_lspi_quad.h) with the two rand48
// words of the episode carried in registers, the same in all four lanes of the quad.  A step's draws are selects: whether the step
// explores and whether it draws at all decide WHICH value a lane keeps, never which instructions it runs.
//
// The ensemble: a WAVE per (group, start state) pair, a block of up to four waves of one group; grid (ceil(n_starts / waves), groups).
// No block barrier anywhere: a wave's region of LDS is its own, and the order between its lanes' writes and reads is the wave's own
// (wave_sync).  A step has three phases:
//
//   A  The projection, ONCE for the whole group.  The members of a group share the environment's state and the projector, so the
//      (index, weight) pairs of phi(obs, a_k) are the same for all of them.  The wave's 64 lanes form them for all k < action_steps and
//      write them to LDS per action in the order of S5.  Triangle: lane 8 k + ii forms pair ii of action k -- one round, 8 pairs per
//      action.  Gauss: the candidates of lspi_box are numbered in index order and shared out 64 at a time; a lane applies D4's test to
//      its candidate and forms the exponential where it is kept; a ballot and the count of kept lanes below compact the round's pairs
//      behind those of the rounds before.  Every exponential is formed once per step, where lspi_evaluate_ensemble_kernel forms it
//      once per member.
//   B  The members, side by side.  Lane j serves the members j, j + 64, ...: per action it walks the pair list (every lane reads the
//      same LDS address: a broadcast) and accumulates w_m[index] * weight from 0 in list order, products and sums rounded separately.
//      w_m is read through the member's base address in global memory.  Then the member's distribution, vote and ranks in the lane.
//      A group below 64 leaves lanes idle here, not in A.
//   C  Votes and member ties are counted by ballots, the ranks summed over the wave by DPP row rotations and four lane reads: integers,
//      any order.  Every lane then holds the same totals, the same model state and the same stream word, and runs the combined softmax,
//      the draw and env_step itself.  The 15 words of a record go out through the first 15 lanes.
//
// Nothing is indexed at run time by a lane's value but LDS and the weights: the actions, the Q-values and the votes are selects.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_query_weights.h"
#include "grlx_softmax.h"
#include "grlx_lspi.h"
#include "grlx_lspi_read.h"
#include "grlx_lspi_evaluate.h"
#include "grlx_lspi_evaluate_sampled.h"
#include "grlx_lspi_quad.h"
#include "grlx_episode.h"

namespace grlx {

// ------------------------------------------------------------------------------------------ one policy ---
template <int PROJ, int SAMPLER, bool RECORD>
__global__ __launch_bounds__(kLspiEvalBlock) void lspi_evaluate_sampled_kernel(LspiParams L, LspiSampledArgs T)
{
  constexpr int R = kLspiSampledTrajWords;
  __shared__ double sw[kLspiMaxF];
  const LspiEvalArgs &A = T.e;
  const int rl = blockIdx.y, r = A.first_replica + rl, tid = threadIdx.x, a = tid & (kLspiQuad - 1);
  const double *w = L.w + (size_t)r * 2 * L.Fp;
  for (int k = tid; k < L.F; k += kLspiEvalBlock) sw[k] = w[k];
  __syncthreads();
  const int s = (int)blockIdx.x * kLspiEvalQuads + (tid >> 2);
  const bool live = s < A.n_starts;                    // the quads past the chunk's end neither load nor store nor draw
  const size_t pair = (size_t)rl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kLspiS], obs[kLspiD];
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) x[i] = live ? A.states[(size_t)s * kLspiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(L.env, x, obs);                // the start state's terminal code is ignored
  uint64_t S = 0, G = 0;                               // the sampler's stream, the global stream: the same in the quad's four lanes
  if (live)
  {
    S = T.streams ? T.streams[pair * 2] : 0ull;
    G = T.streams ? T.streams[pair * 2 + 1] : L.rep[r].G;              // a copy: the replica's own stream does not move
  }
  LspiActs<PROJ> act;
  lspi_acts<PROJ>(L, a, act);

  EpisodeSums e = {0., 0., 1., 0, 0, 0};
  int explored = 0;
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
    { // the draws sit under the step's predicate: a finished quad's streams stand where its last step left them
      bool random = false;
      if constexpr (SAMPLER == GRLX_SAMPLER_EPSILON_GREEDY)
      { // EpsilonGreedySampler::sample (greedy.cpp:144-218): the sampler's stream first
        S = lcg_next(S);
        random = lcg_double(S) < T.epsilon;
      }
      // one draw of the global stream where the step explores (lrand48 % action_steps acts) or ties (greedy.cpp:77-85: lrand48 % man
      // counts down over the maximal entries), none otherwise
      const bool tie = !random && man > 1;
      const uint64_t G1 = lcg_next(G);
      G = (random || tie) ? G1 : G;
      int jj = (int)(lcg_long(G1) % (uint32_t)(random ? L.A : man));
      int idx = random ? jj : mai;
#pragma unroll
      for (int k = 0; k < kMaxActions; ++k)
      {
        const bool m = k < L.A && q[k] == best;
        idx = (tie && m && jj == 0) ? k : idx;
        jj -= m ? 1 : 0;
      }
      const double action = lspi_action_of(L, idx);
      double value = q[0];
#pragma unroll
      for (int k = 1; k < kMaxActions; ++k) value = (idx == k) ? q[k] : value;
      double before[kLspiD];
#pragma unroll
      for (int i = 0; i < kLspiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(L.env, x, action, obs, reward, terminal, status);
      active = episode_account(e, reward, L.gamma_tau, terminal, status, tie);
      explored += random ? 1 : 0;
      if constexpr (RECORD)
      { // lane a's words: a, a + 4, a + 8; the last word of the record is `explored`
        double *at = rec + (size_t)(e.steps - 1) * R;
#pragma unroll
        for (int w0 = 0; w0 < R; w0 += kLspiQuad)
        {
          const double out = record_head<kLspiD, kLspiS>(w0 + a, action, reward, value, idx, man, e.code, before, x);
          if (w0 + a < R) at[w0 + a] = (w0 + a == R - 1) ? (random ? 1.0 : 0.0) : out;
        }
      }
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
  T.explored[pair] = explored;
  T.streams_out[pair * 2] = S;
  T.streams_out[pair * 2 + 1] = G;
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) A.final_state[pair * kLspiS + i] = x[i];
}

// ------------------------------------------------------------------------------------------ the ensemble ---
// (wave_sync, grlx_table.h: what one lane of the wave wrote to LDS before it, every lane of the wave reads after it, and the other way round)
// the sum of v over the wave's 64 lanes, in every lane (all 64 must be here): DPP row_ror 8, 4, 2, 1 inside the rows of 16, then one
// lane of each row
template <int N>
__device__ __forceinline__ int lspi_row_ror(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_sum(int v)
{
  v += lspi_row_ror<8>(v);
  v += lspi_row_ror<4>(v);
  v += lspi_row_ror<2>(v);
  v += lspi_row_ror<1>(v);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// A member's distribution over the first NA of q (findmax: best, man), its vote and its ranks, as grlx_evaluate_ensemble_sampled states
// them and fqi_ensemble_sampled_kernel forms them (that kernel keeps its own lines and its instructions).
__device__ __forceinline__ void lspi_member_ballot(const double (&q)[kMaxActions], double best, int man, int NA, int member, double param, bool rank,
                                                   int &vote, int (&ranks)[kMaxActions])
{
  double d[kMaxActions];
  if (member == GRLX_MEMBER_SOFTMAX) batch_softmax(q, NA, param, d);
  else
  { // greedy.cpp:88-98, and :229-236 for the epsilon-greedy member
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
    {
      d[a] = (a < NA && q[a] == best) ? 1. / (double)man : 0.;
      if (member == GRLX_MEMBER_EPSILON)
      {
        d[a] = (d[a] == 1) ? 1 - param : d[a];
        d[a] += param / (double)NA;
      }
    }
  }
  // the member's vote (multi_discrete.cpp:218-229): the first entry above every entry before it and above 0.0; NA - 1 without one
  double top = 0.0;
  vote = NA - 1;
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a)
  {
    const bool up = a < NA && d[a] > top;
    vote = up ? a : vote;
    top = up ? d[a] : top;
  }
  if (rank)
  { // the rank of action a among the member's entries: 1 + the entries strictly below it (:237-281)
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
    {
      int below = 1;
#pragma unroll
      for (int k = 0; k < kMaxActions; ++k) below += (k < NA && d[a] > d[k]) ? 1 : 0;
      ranks[a] += (a < NA) ? below : 0;
    }
  }
}

template <int PROJ, bool RECORD>
__global__ __launch_bounds__(kLspiEnsWave * kLspiEnsMaxWaves) void lspi_ensemble_sampled_kernel(LspiParams L, LspiEnsSampledArgs T)
{
  constexpr int R = kLspiEnsSampledTrajWords;
  extern __shared__ double lspi_ens_lds[];
  const LspiEnsArgs &A = T.e;
  const int gl = blockIdx.y, G = A.group_size, NA = L.A, cap = T.cap;
  const int lane = threadIdx.x & (kLspiEnsWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kLspiEnsWave), waves = (int)blockDim.x / kLspiEnsWave;
  const int s = (int)blockIdx.x * waves + wv;
  if (s >= A.n_starts) return;                         // a whole wave: the kernel has no block barrier
  // the wave's region: weights [NA][cap], indices [NA][cap], pairs kept per action [kMaxActions]
  double *pw = (double *)((char *)lspi_ens_lds + (size_t)wv * lspi_ens_wave_bytes(NA, cap));
  int *pi = (int *)(pw + NA * cap), *pn = pi + NA * cap;
  const bool rank = A.rule == GRLX_ENSEMBLE_RANK;
  const int r0 = A.first_replica + gl * G;
  const double *nets = L.w + (size_t)r0 * 2 * L.Fp;    // member m: nets + m * pitch, its current weights
  const size_t pitch = 2 * (size_t)L.Fp;
  const size_t pair = (size_t)gl * (size_t)A.n_starts + (size_t)s;
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kLspiS], obs[kLspiD];
#pragma unroll
  for (int i = 0; i < kLspiS; ++i) x[i] = A.states[(size_t)s * kLspiS + i];
  (void)Env<GRLX_ENV_PENDULUM>::observe(L.env, x, obs);                // the start state's terminal code is ignored
  uint64_t rng = T.streams ? T.streams[pair] : L.rep[r0].G;            // a copy: the replica's own stream does not move

  // phase A's constants of the lane.  Triangle: the lane's action ka and corner ii -- lspi_triangle's dd = 2 and the corner's offset.
  const int ka = lane >> 3, ii = lane & 7;
  int t_off = 0;
  double t_f2 = 0, rad = 0;
  if constexpr (PROJ == GRLX_RBF_TRIANGLE)
  {
    const double gridpos = fmin(fmax((lspi_action_of(L, ka) - L.in_min[2]) / L.delta[2], 0.), L.top[2]);
    const int v = (int)gridpos;
    const double d2 = gridpos - v;
    t_off = v * L.stride[2] + ((ii & 1) ? L.stride[0] : 0) + ((ii & 2) ? L.stride[1] : 0) + ((ii & 4) ? L.stride[2] : 0);
    t_f2 = (ii & 4) ? d2 : (1 - d2);
  }
  else rad = lspi_box_radius(L.cutoff_distsq);

  EpisodeSums e = {0., 0., 1., 0, 0, 0};
  int explored = 0;
  long long member_ties = 0, agreement = 0;
  bool active = true;
  for (int step = 0; step < A.max_steps && active; ++step)             // wave-uniform: every lane carries the same episode
  {
    // ---- A: the pairs of phi(obs, a_k), k < NA, in the order of S5
    if constexpr (PROJ == GRLX_RBF_TRIANGLE)
    { // lspi_triangle: dd = 0, 1 here, the weight the product over dd ascending from 1
      int index = 0;
      double p = 1;
#pragma unroll
      for (int dd = 0; dd < kLspiD; ++dd)
      {
        const double gridpos = fmin(fmax((obs[dd] - L.in_min[dd]) / L.delta[dd], 0.), L.top[dd]);
        const int v = (int)gridpos;
        index += v * L.stride[dd];
        const double dist = gridpos - v;
        p *= (ii & (1 << dd)) ? dist : (1 - dist);
      }
      p *= t_f2;
      if (ka < NA)
      {
        pi[ka * cap + ii] = index + t_off;
        pw[ka * cap + ii] = p;
      }
    }
    else
    {
      int lo0, hi0, lo1, hi1;
      const double b0 = (L.in_min[0] - obs[0]) / L.delta[0], b1 = (L.in_min[1] - obs[1]) / L.delta[1];    // lspi_gauss_base's dd = 0, 1
      lspi_box(b0, rad, L.steps[0], lo0, hi0);
      lspi_box(b1, rad, L.steps[1], lo1, hi1);
      const int n0 = hi0 >= lo0 ? hi0 - lo0 + 1 : 0, n1 = hi1 >= lo1 ? hi1 - lo1 + 1 : 0;
      const int s0 = L.steps[0], s01 = L.steps[0] * L.steps[1];
      for (int k = 0; k < NA; ++k)
      {
        int lo2, hi2;
        const double base[kLspiNIn] = {b0, b1, (L.in_min[2] - lspi_action_of(L, k)) / L.delta[2]};
        lspi_box(base[2], rad, L.steps[2], lo2, hi2);
        const int n = n0 * n1 * (hi2 >= lo2 ? hi2 - lo2 + 1 : 0);      // the box's candidates, numbered in index order (k0 fastest)
        int kept = 0;
        for (int c0 = 0; c0 < n; c0 += kLspiEnsWave)
        {
          const int c = c0 + lane < n ? c0 + lane : 0;                 // n > 0 here: n0, n1 >= 1
          const int k0 = lo0 + c % n0, k1 = lo1 + (c / n0) % n1, k2 = lo2 + (c / n0) / n1;
          const double g = lspi_gauss(L, base, k0, k1, k2);            // D4's test and D5's exponential: negative where dropped
          const bool keep = c0 + lane < n && g >= 0.;
          const unsigned long long mask = __ballot(keep);
          const int at = kept + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
          if (keep && at < cap)                                        // at < cap holds by the launcher's bound; the test keeps a store inside the region
          {
            pi[k * cap + at] = k2 * s01 + k1 * s0 + k0;
            pw[k * cap + at] = g;
          }
          kept += __popcll(mask);
        }
        if (lane == 0) pn[k] = kept < cap ? kept : cap;
      }
    }
    wave_sync();

    // ---- B: the members, lane j serving j, j + 64, ...
    int votes[kMaxActions], ranks[kMaxActions], mties = 0;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a) { votes[a] = 0; ranks[a] = 0; }
    for (int m0 = 0; m0 < G; m0 += kLspiEnsWave)
    {
      const int m = m0 + lane;
      int vote = -1;
      bool tied = false;
      if (m < G)
      {
        const double *wm = nets + (size_t)m * pitch;
        double q[kMaxActions], best = 0;
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a) q[a] = 0;
        int mai = 0, man = 1;                          // findmax as the reads arrive
        for (int k = 0; k < NA; ++k)
        {
          const int n = PROJ == GRLX_RBF_TRIANGLE ? 8 : pn[k];
          const int *ki = pi + k * cap;
          const double *kw = pw + k * cap;
          double qk = 0;
          for (int p = 0; p < n; ++p) qk += wm[ki[p]] * kw[p];         // S5
#pragma unroll
          for (int a = 0; a < kMaxActions; ++a) q[a] = (k == a) ? qk : q[a];
          if (k == 0 || qk > best) { best = qk; mai = k; man = 1; }
          else if (qk == best) man++;
        }
        lspi_member_ballot(q, best, man, NA, T.member, T.member_param, rank, vote, ranks);
        tied = man > 1;
      }
      // every lane is here again: the members' votes and ties of this round, counted
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
        if (a < NA) votes[a] += __popcll(__ballot(vote == a));
      mties += __popcll(__ballot(tied));
    }
    if (rank)
    {
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
        if (a < NA) ranks[a] = wave_sum(ranks[a]);
    }
    wave_sync();                                       // the next step's pairs overwrite what the members have read

    // ---- C: the combined distribution, the draw and the model step, the same bits in every lane
    double sc[kMaxActions], dist[kMaxActions];
    int score[kMaxActions];
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
    {
      score[a] = rank ? ranks[a] : votes[a];
      sc[a] = (double)score[a];
    }
    batch_softmax(sc, NA, T.tau, dist);
    // grl::sample (utils.h:227-250) on one drand48 of the episode's stream
    double sum = 0;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
      if (a < NA) sum += dist[a];
    rng = lcg_next(rng);
    const double u = lcg_double(rng) * sum;
    double acc = 0;
    int idx = NA - 1;
    bool found = false;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
      if (a < NA)
      {
        acc += dist[a];
        const bool here = !found && u < acc;
        idx = here ? a : idx;
        found = found || here;
      }
    int mai = 0, man = 1, top = score[0];              // findmax over the score
#pragma unroll
    for (int a = 1; a < kMaxActions; ++a)
      if (a < NA)
      {
        if (score[a] > top) { top = score[a]; mai = a; man = 1; }
        else if (score[a] == top) man++;
      }
    double value = 0, prob = 0;
    int agree = 0;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
    {
      value = (idx == a) ? sc[a] : value;
      prob = (idx == a) ? dist[a] : prob;
      agree = (idx == a) ? votes[a] : agree;
    }
    const double action = lspi_action_of(L, idx);
    const bool off = idx != mai;
    double before[kLspiD];
#pragma unroll
    for (int i = 0; i < kLspiD; ++i) before[i] = obs[i];
    double reward = 0;
    int terminal = 0;
    uint32_t status = 0;
    env_step<GRLX_ENV_PENDULUM, false>(L.env, x, action, obs, reward, terminal, status);
    active = __builtin_amdgcn_readfirstlane((int)episode_account(e, reward, L.gamma_tau, terminal, status, man > 1)) != 0;      // a scalar: the loop's branch
    member_ties += mties;
    agreement += agree;
    explored += off ? 1 : 0;
    if constexpr (RECORD)
    { // word `lane` of the record: the head's words with agreement and member ties before the observation, `explored` and `prob` last
      const int hw = lane >= GRLX_TRAJ_ENS_OBS ? lane - (GRLX_TRAJ_ENS_OBS - GRLX_TRAJ_OBS) : (lane >= GRLX_TRAJ_OBS ? 0 : lane);
      double out = record_head<kLspiD, kLspiS>(hw, action, reward, value, idx, man, e.code, before, x);
      out = (lane == GRLX_TRAJ_ENS_AGREEMENT) ? (double)agree : out;
      out = (lane == GRLX_TRAJ_ENS_MEMBER_TIES) ? (double)mties : out;
      out = (lane == R - 2) ? (off ? 1.0 : 0.0) : out;
      out = (lane == R - 1) ? prob : out;
      if (lane < R) rec[(size_t)(e.steps - 1) * R + lane] = out;
    }
  }
  if constexpr (RECORD)                                // behind the episode's end: all-zero bits
    for (size_t k = (size_t)e.steps * R + (size_t)lane; k < (size_t)A.max_steps * R; k += kLspiEnsWave) rec[k] = 0.;
  if (lane != 0) return;
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
  for (int i = 0; i < kLspiS; ++i) A.final_state[pair * kLspiS + i] = x[i];
}

// ------------------------------------------------------------------------------------------ launchers ---
template <int PROJ, int SAMPLER>
static void lspi_sampled_launch(const LspiParams &L, const LspiSampledArgs &A, dim3 grid, hipStream_t stream)
{
  const dim3 block(kLspiEvalBlock);
  if (A.e.records) hipLaunchKernelGGL((lspi_evaluate_sampled_kernel<PROJ, SAMPLER, true>), grid, block, 0, stream, L, A);
  else hipLaunchKernelGGL((lspi_evaluate_sampled_kernel<PROJ, SAMPLER, false>), grid, block, 0, stream, L, A);
}

hipError_t launch_lspi_evaluate_sampled(const LspiParams &L, const LspiSampledArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.e.n_starts + kLspiEvalQuads - 1) / kLspiEvalQuads), (unsigned)rows);
  const bool tri = L.projector == GRLX_RBF_TRIANGLE, eps = A.sampler == GRLX_SAMPLER_EPSILON_GREEDY;
  if (tri && eps) lspi_sampled_launch<GRLX_RBF_TRIANGLE, GRLX_SAMPLER_EPSILON_GREEDY>(L, A, grid, stream);
  else if (tri) lspi_sampled_launch<GRLX_RBF_TRIANGLE, GRLX_SAMPLER_GREEDY>(L, A, grid, stream);
  else if (eps) lspi_sampled_launch<GRLX_RBF_GAUSS, GRLX_SAMPLER_EPSILON_GREEDY>(L, A, grid, stream);
  else lspi_sampled_launch<GRLX_RBF_GAUSS, GRLX_SAMPLER_GREEDY>(L, A, grid, stream);
  return hipGetLastError();
}

// The slots per action of a wave's region.  Triangle: 8.  Gauss: lspi_box keeps, per dimension, the k between floor(-base - rad) and
// ceil(-base + rad), both formed with an error far below 1: fewer than 2 rad + 3 + 2 err of them, so at most ceil(2 rad) + 3, and never
// more than the grid has.  In the measurement build whose lspi_box gives the whole grid, the whole grid.
static int lspi_ens_cap(const LspiParams &L)
{
  if (L.projector == GRLX_RBF_TRIANGLE) return 8;
#ifdef GRLX_LSPI_EVAL_FULL_WALK
  return L.F;
#endif
  const double rad = lspi_box_radius(L.cutoff_distsq), per = ceil(2 * rad) + 3;
  int cap = 1;
  for (int d = 0; d < kLspiNIn; ++d) cap *= per < (double)L.steps[d] ? (int)per : L.steps[d];
  return cap;
}

hipError_t launch_lspi_evaluate_ensemble_sampled(const LspiParams &L, LspiEnsSampledArgs A, int rows, hipStream_t stream)
{
  A.cap = lspi_ens_cap(L);
  const size_t bytes = lspi_ens_wave_bytes(L.A, A.cap);
  if (bytes > kLspiEnsLdsLimit) return hipErrorInvalidValue;           // unreachable for F <= kLspiMaxF (the header's static_assert)
  int waves = kLspiEnsMaxWaves;                                        // as many episodes per block as their regions leave room for
  while (waves > 1 && (size_t)waves * bytes > kLspiEnsLdsLimit) waves /= 2;
  const dim3 grid((unsigned)((A.e.n_starts + waves - 1) / waves), (unsigned)rows), block((unsigned)(kLspiEnsWave * waves));
  const size_t lds = (size_t)waves * bytes;
  const bool tri = L.projector == GRLX_RBF_TRIANGLE;
  if (A.e.records)
  {
    if (tri) hipLaunchKernelGGL((lspi_ensemble_sampled_kernel<GRLX_RBF_TRIANGLE, true>), grid, block, lds, stream, L, A);
    else hipLaunchKernelGGL((lspi_ensemble_sampled_kernel<GRLX_RBF_GAUSS, true>), grid, block, lds, stream, L, A);
  }
  else
  {
    if (tri) hipLaunchKernelGGL((lspi_ensemble_sampled_kernel<GRLX_RBF_TRIANGLE, false>), grid, block, lds, stream, L, A);
    else hipLaunchKernelGGL((lspi_ensemble_sampled_kernel<GRLX_RBF_GAUSS, false>), grid, block, lds, stream, L, A);
  }
  return hipGetLastError();
}

} // namespace grlx
