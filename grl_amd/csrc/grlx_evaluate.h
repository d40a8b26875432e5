// grlx_evaluate.h -- greedy evaluation episodes (grlx_evaluate): what grlx_api.cpp hands to the kernels of grlx_evaluate.hip.
// Included by those two only: no rollout kernel sees it, the kernels have no row in the kernel table and DevParams does not grow.
#pragma once
#include "grlx_internal.h"

namespace grlx {

// One chunk of start states for a range of replicas; every pointer is a device pointer.  A pair is (replica, start state) with the
// index (replica - first_replica) * n_starts + start: the layout of every per-pair array.
struct EvaluateArgs {
  int32_t            first_replica, n_replicas;
  int32_t            n_starts;      // start states of this chunk
  int32_t            max_steps;     // 1 ... GRLX_MAX_EPISODE_STEPS: no episode runs further, whatever its state says
  const double      *states;        // [n_starts][model state dimensions]
  const SweepParams *sweep;         // [replica of the context]: the replica's own gamma; null = DevParams::gamma
  double            *ret, *disc;    // [pair]
  int32_t           *steps, *terminal, *ties;   // [pair]
  double            *final_state;   // [pair][model state dimensions]
};

// terminal code of an episode that left the portable math's domain (Env::in_domain at a step end); 0 / 1 / 2 are the task's
constexpr int kEvaluateDomain = 3;

// grlx_evaluate_ensemble: one chunk of start states for a range of replicas in groups of group_size consecutive ones; every pointer is
// a device pointer.  A pair is (group, start state) with the index group * n_starts + start.
struct EnsembleArgs {
  int32_t            first_replica, n_replicas;
  int32_t            group_size;    // divides n_replicas
  int32_t            rule;          // GRLX_ENSEMBLE_VOTE / GRLX_ENSEMBLE_MEAN_Q
  int32_t            n_starts, max_steps;
  const double      *states;        // [n_starts][model state dimensions]
  const SweepParams *sweep;         // the gamma of a group's FIRST replica; null = DevParams::gamma
  double            *ret, *disc;    // [pair]
  int32_t           *steps, *terminal, *ties;   // [pair]
  int64_t           *member_ties, *agreement;   // [pair]
  double            *final_state;   // [pair][model state dimensions]
};

// grlx_evaluate_trajectory / grlx_evaluate_ensemble_trajectory: the same chunk with a place for every step.  records[pair][max_steps][R]
// doubles, R = trajectory_words(); record t of a pair is its step t (include/grlx.h: GRLX_TRAJ_*).  The launchers expect the records
// zero-filled: a kernel writes the records of the steps it takes and nothing behind an episode's end.  Structs of their own: the
// parameter blocks of the evaluation kernels, and with them their machine code, stay what they were.
struct TrajectoryArgs {
  EvaluateArgs e;
  double      *records;
};
struct EnsembleTrajectoryArgs {
  EnsembleArgs e;
  double      *records;
};

bool evaluate_built(int agent, int env, int actions);      // is there an instantiation for this context?
int  trajectory_words(int env, bool ensemble);             // R of an environment's record; 0 for one without an instantiation
hipError_t launch_evaluate(const DevParams &P, const EvaluateArgs &A, hipStream_t stream);
hipError_t launch_evaluate_ensemble(const DevParams &P, const EnsembleArgs &A, hipStream_t stream);    // Q agents only
hipError_t launch_trajectory(const DevParams &P, const TrajectoryArgs &A, hipStream_t stream);
hipError_t launch_trajectory_ensemble(const DevParams &P, const EnsembleTrajectoryArgs &A, hipStream_t stream);    // Q agents only

} // namespace grlx
