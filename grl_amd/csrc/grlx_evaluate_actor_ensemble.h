// grlx_evaluate_actor_ensemble.h -- episodes of an ensemble of actors on the members' combined action (grlx_evaluate_actor_ensemble,
// grlx_evaluate_actor_ensemble_trajectory): what grlx_api_read.cpp hands to the kernels of grlx_evaluate_actor_ensemble.hip.  Included by
// those two only.  An argument block of its own beside EvaluateArgs and EnsembleArgs: the parameter blocks of the other evaluation
// kernels, and with them their machine code, stay what they were.
#pragma once
#include "grlx_internal.h"
#include "grlx_evaluate.h"

namespace grlx {

// One chunk of start states for a range of replicas in groups of group_size consecutive ones; every pointer is a device pointer.  A pair
// is (group, start state) with the index group * n_starts + start: the layout of every per-pair array.
struct ActorEnsembleArgs {
  int32_t            first_replica, n_replicas;
  int32_t            group_size;    // divides n_replicas; 1 ... GRLX_ACTOR_ENSEMBLE_MAX
  int32_t            rule;          // GRLX_ACTOR_ENSEMBLE_*
  int32_t            bins;          // BINNING: the bins, 1 ... 64; DATA_CENTER: the members kept, >= 1; not read otherwise
  int32_t            n_starts, max_steps;
  double             r;             // DENSITY: the kernel's radius, > 0; not read otherwise
  const double      *states;        // [n_starts][model state dimensions]
  const SweepParams *sweep;         // filled by the staging path and never read: an actor-critic context has no sweep, disc is on DevParams::gamma
  double            *ret, *disc;    // [pair]
  int32_t           *steps, *terminal, *ties;   // [pair]
  int64_t           *kept;          // [pair]
  double            *spread;        // [pair]
  double            *final_state;   // [pair][model state dimensions]
  double            *records;       // trajectory kernel only: [pair][max_steps][R], R = actor_ensemble_trajectory_words(), zero-filled by the caller
};

int actor_ensemble_trajectory_words(int env);      // trajectory_words(env, false) + 2; 0 for an environment without an instantiation
hipError_t launch_evaluate_actor_ensemble(const DevParams &P, const ActorEnsembleArgs &A, hipStream_t stream);       // the actor-critic only
hipError_t launch_trajectory_actor_ensemble(const DevParams &P, const ActorEnsembleArgs &A, hipStream_t stream);     // the actor-critic only

} // namespace grlx
