// grlx_evaluate_ensemble_sampled.h -- sampled ensemble episodes (grlx_evaluate_ensemble_sampled, grlx_evaluate_ensemble_sampled_trajectory):
// what grlx_api_read.cpp hands to the kernels of grlx_evaluate_ensemble_sampled.hip.  Included by those two only.  A struct of its own
// beside EnsembleArgs: the parameter blocks of the greedy ensemble kernels, and with them their machine code, stay what they were.
#pragma once
#include "grlx_internal.h"
#include "grlx_evaluate.h"

namespace grlx {

// One chunk of start states for a range of replicas in groups; every pointer is a device pointer.  e: grlx_evaluate_ensemble's chunk, its
// rule the STRATEGY (GRLX_ENSEMBLE_MAJORITY / GRLX_ENSEMBLE_RANK), its ties the steps at which the score's maximum was not unique.  The
// per-pair arrays of this struct have the chunk's layout too, pair = group * e.n_starts + start.
struct EnsembleSampledArgs {
  EnsembleArgs    e;
  double          tau;          // > 0: the temperature of the combined softmax
  int32_t         member;       // GRLX_MEMBER_GREEDY / _EPSILON / _SOFTMAX: the members' distribution
  double          member_param; // EPSILON: e in [0, 1] or GRLX_EPSILON_OWN (every member's eps_decay * epsilon); SOFTMAX: tau_m > 0
  const uint64_t *streams;      // [pair]: the episode's rand48 state; null = the global stream of the group's first replica as it stands
  uint64_t       *streams_out;  // [pair]: after the episode's last step
  int32_t        *explored;     // [pair]
  double         *records;      // trajectory kernels only: [pair][max_steps][R], R = ensemble_sampled_trajectory_words(), zero-filled by the caller
};

int ensemble_sampled_trajectory_words(int env);     // trajectory_words(env, true) + 2; 0 for an environment without an instantiation
hipError_t launch_evaluate_ensemble_sampled(const DevParams &P, const EnsembleSampledArgs &A, hipStream_t stream);      // Q agents only
hipError_t launch_trajectory_ensemble_sampled(const DevParams &P, const EnsembleSampledArgs &A, hipStream_t stream);    // Q agents only

} // namespace grlx
