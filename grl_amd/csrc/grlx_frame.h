// grlx_frame.h -- the experiment frame shared by the kernels that run four replicas per wave (OnlineLearningExperiment::run,
// online_learning.cpp:140-262): who a lane is, what a replica carries from launch to launch, what a trial, a counted step,
// a tap record and a result row are.  The kernels keep their own loops and their own algorithm; these are the parts that
// are the same in all of them.
// Part of the single translation unit grlx_kernels.hip (included there, in order; not self-contained).
#pragma once

namespace grlx {

// ------------------------------------------------------------ lane identity ---
// One wave = 4 replicas x 16 lanes: group g works on replica r, lane j of the group owns tiling j.  Groups beyond the last
// replica work on replica 0 without writing anything back (live = false).
struct WaveIds {
  int lane, g, j, r;
  bool live, tapped;
  unsigned long long gmask;           // the wave lanes of this replica
};

__device__ __forceinline__ WaveIds wave_ids(const DevParams &P)
{
  WaveIds ids;
  ids.lane = threadIdx.x & 63;
  ids.g = ids.lane >> 4;
  ids.j = ids.lane & 15;
  const int r_raw = blockIdx.x * kReplicasPerWave + ids.g;
  ids.live = r_raw < P.n_replicas;
  ids.r = ids.live ? r_raw : 0;
  ids.tapped = ids.live && (ids.r == P.tap_replica);
  ids.gmask = 0xFFFFull << (16 * ids.g);
  return ids;
}

// ------------------------------------------------- what a replica carries ---
// The part of ReplicaState every discrete-action kernel reads at its start and writes at its end.  What only one kernel
// persists stays in that kernel, next to run_store.
template <int S>
struct RunRegs {
  double x[S];
  uint64_t G, TL, S1;
  double eps_decay;
  int64_t tt, ss;
  uint64_t test_steps;
  uint32_t status, rows;
};

template <int S>
__device__ __forceinline__ void run_load(const ReplicaState &RS, RunRegs<S> &run)
{
#pragma unroll
  for (int i = 0; i < S; ++i) run.x[i] = RS.x[i];
  run.G = RS.G; run.TL = RS.TL; run.S1 = RS.S1;
  run.eps_decay = RS.eps_decay;
  run.tt = RS.tt; run.ss = RS.ss;
  run.test_steps = RS.test_steps;
  run.status = RS.status; run.rows = RS.rows;
}

// write the replica back; `inserted` = slots this lane created in table 0
template <int S>
__device__ __forceinline__ void run_store(ReplicaState &RS, const WaveIds &ids, const RunRegs<S> &run, uint32_t inserted)
{
  uint32_t ins = inserted;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) ins += __shfl_xor(ins, off, 16);
  if (ids.live && ids.j == 0)
  {
#pragma unroll
    for (int i = 0; i < S; ++i) RS.x[i] = run.x[i];
    RS.G = run.G;
    RS.TL = run.TL;
    RS.S1 = run.S1;
    RS.eps_decay = run.eps_decay;
    RS.tt = run.tt;
    RS.ss = run.ss;
    RS.test_steps = run.test_steps;
    RS.n_slots[0] += ins;
    RS.rows = run.rows;
  }
}

// status may differ per lane (a probe failure is lane-local): OR over the replica
__device__ __forceinline__ void store_status(ReplicaState &RS, const WaveIds &ids, uint32_t status)
{
  uint32_t st = status;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) st |= __shfl_xor(st, off, 16);
  if (ids.live && ids.j == 0) RS.status = st;
}

// ------------------------------------------------------------- trial plan ---
struct TrialPlan {
  bool act;                           // the replica runs this trial
  int ti, test, subtrials;            // test interval; test trial?; episodes the trial consists of
};

// P: steps budget and test_trials; N: the numeric block test_interval comes from (a constant in a specialised build)
__device__ __forceinline__ TrialPlan trial_plan(const DevParams &P, const DevParams &N, const WaveIds &ids, int64_t ss, int64_t tt)
{
  TrialPlan plan;
  // online_learning.cpp:154: a replica whose learning steps have reached the steps budget starts no further trial
  plan.act = ids.live && !(P.steps_budget != 0u && (uint64_t)ss >= P.steps_budget);
  plan.ti = N.test_interval;
  plan.test = (plan.ti >= 0 && tt % (plan.ti + 1) == plan.ti) ? 1 : 0;        // online_learning.cpp:160
  // a test trial is test_trials greedy episodes (online_learning.cpp:161-170): each starts the environment and the agent anew, while
  // reward and time keep adding up (:202-203); a learning trial is one episode
  plan.subtrials = (plan.test && P.test_trials > 1) ? P.test_trials : 1;
  return plan;
}

// one control step of a running episode has been taken (not the start() pass)
__device__ __forceinline__ void count_step(int64_t &ss, uint64_t &test_steps, int test, bool first)
{
  if (!first)
  {
    if (test) test_steps++;
    else ss++;                                                       // online_learning.cpp:218
  }
}

// row of a test trial (online_learning.cpp:238-262) -- or of every trial when test_interval < 0
__device__ __forceinline__ void record_row(const DevParams &P, const WaveIds &ids, const TrialPlan &plan, uint32_t &rows, uint32_t &status,
                                           int64_t ss, int64_t tt, double total_reward, double time)
{
  if (plan.act && (plan.ti >= 0 ? plan.test : 1))
  {
    if (rows < (uint32_t)P.max_rows)
    {
      if (ids.j == 0)
      {
        size_t at = (size_t)rows * (size_t)P.n_replicas + (size_t)ids.r;
        P.row_reward[at] = total_reward / (double)plan.subtrials;              // online_learning.cpp:224-225
        P.row_time[at] = time / (double)plan.subtrials;
        P.row_steps[at] = ss;
        P.row_trial[at] = (plan.ti >= 0) ? (tt + 1 - (tt + 1) / (plan.ti + 1)) : tt;
      }
      rows++;
    }
    else
      status |= ST_ROWS_FULL;
  }
}

// ------------------------------------------------------- action constants ---
// The action coordinate of tiling j and the tiling index itself do not change: their murmur
// key words are computed once (32-bit multiplies are quarter rate).
template <int T, int D, int NA>
__device__ __forceinline__ void action_keys(const TileParams &tile, const double *actions, int j, double (&acts)[NA], uint32_t (&key_act)[NA],
                                            uint32_t &key_j)
{
#pragma unroll
  for (int a = 0; a < NA; ++a) acts[a] = actions[a];
#pragma unroll
  for (int a = 0; a < NA; ++a)
    key_act[a] = in_reg(murmur_key(tile_coord<T>(tile, D, tile_quant(tile, D, actions[a]), j)));
  key_j = in_reg(murmur_key(j));
}

// ---------------------------------------------------------------- row sums ---
// LinearRepresentation::read (linear.cpp:136-184): serial sum over the 16 tilings, then the mean.  Lane r of the replica sums
// row r of the LDS tile in the reference's order (linear.cpp:147-151); the results are shared through sh_res (lanes beyond
// NROWS repeat row 0, harmlessly).  The caller orders the tile's writes before and the reads of sh_res after (wave_sync).
template <int NROWS>
__device__ __forceinline__ void sum_rows(const double *sh_w, double *sh_res, int g, int j)
{
  const int row = (j < NROWS) ? j : 0;
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) sum += SHW(row, k, g);
  sh_res[g * 16 + j] = sum / 16;
}

// -------------------------------------------------------------- tap record ---
// The fields of a per-step record that every kernel fills the same way (lane 0 of the tapped replica); p_idx, trace_len
// and delta are the caller's.
template <int NA, int S, int D>
__device__ __forceinline__ void tap_common(grlx_tap *tp, int test, int action_index, int terminal, const double (&obs)[D], double action,
                                           double reward, const double (&x)[S], const double (&q)[NA], bool has_next)
{
  tp->test = test;
  tp->action_index = action_index;
  tp->terminal = terminal;
  for (int i = 0; i < GRLX_MAX_DIMS; ++i) tp->obs[i] = (i < D) ? obs[i] : 0.;
  tp->action = action;
  tp->reward = reward;
  for (int i = 0; i < GRLX_MAX_STATE; ++i) tp->state[i] = (i < S) ? x[i] : 0.;
  for (int a = 0; a < kMaxActions; ++a) tp->q[a] = 0.;
#pragma unroll
  for (int a = 0; a < NA; ++a) tp->q[a] = has_next ? q[a] : 0.;
}

} // namespace grlx
