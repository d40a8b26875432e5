// grlx_evaluate_sampled.h -- sampled evaluation episodes (grlx_evaluate_sampled, grlx_evaluate_sampled_trajectory): what grlx_api_read.cpp
// hands to the kernels of grlx_evaluate_sampled.hip.  Included by those two only.  A struct of its own beside EvaluateArgs: the parameter
// blocks of the greedy evaluation kernels, and with them their machine code, stay what they were.
#pragma once
#include "grlx_internal.h"
#include "grlx_evaluate.h"

namespace grlx {

// One chunk of start states for a range of replicas; every pointer is a device pointer.  e: grlx_evaluate's chunk, its ties counting the
// tie breaks DRAWN.  The per-pair arrays of this struct have the chunk's layout too, pair = (replica - first_replica) * e.n_starts + start:
// the host stages the caller's [replica][start][2] streams chunk by chunk, so that a chunk's rows begin at its first start state.
struct SampledArgs {
  EvaluateArgs    e;
  int32_t         sampler;      // GRLX_SAMPLER_GREEDY / GRLX_SAMPLER_EPSILON_GREEDY
  double          epsilon;      // [0, 1]: the caller's, for every replica; GRLX_EPSILON_OWN: eps_decay * epsilon of the replica
  const uint64_t *streams;      // [pair][2]: the sampler's stream, the global stream; null = the replica's own S1 and G as they stand
  uint64_t       *streams_out;  // [pair][2]: both after the episode's last step
  int32_t        *explored;     // [pair]
  double         *records;      // trajectory kernels only: [pair][max_steps][R], R = sampled_trajectory_words(), zero-filled by the caller
};

int sampled_trajectory_words(int env);     // trajectory_words(env, false) + 1; 0 for an environment without an instantiation
hipError_t launch_evaluate_sampled(const DevParams &P, const SampledArgs &A, hipStream_t stream);          // Q agents only
hipError_t launch_trajectory_sampled(const DevParams &P, const SampledArgs &A, hipStream_t stream);        // Q agents only

} // namespace grlx
