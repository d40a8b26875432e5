// grlx_evaluate_noisy.h -- noisy evaluation episodes of the actor-critic (grlx_evaluate_noisy, grlx_evaluate_noisy_trajectory): what
// grlx_api_read.cpp hands to the kernels of grlx_evaluate_noisy.hip.  Included by those two only.  A struct of its own beside EvaluateArgs:
// the parameter blocks of the greedy evaluation kernels, and with them their machine code, stay what they were.
#pragma once
#include "grlx_internal.h"
#include "grlx_evaluate.h"

namespace grlx {

// an `inputs` stream word that means "the replica's own thread-local stream as it stands": no rand48 state reaches 2^48
constexpr uint64_t kNoisyOwnStream = ~0ull;

// One chunk of start states for a range of replicas; every pointer is a device pointer.  e: grlx_evaluate's chunk; e.ties receives the
// steps whose noisy action lay outside the action range (`clipped`).  The per-pair arrays of this struct have the chunk's layout too,
// pair = (replica - first_replica) * e.n_starts + start.
struct NoisyArgs {
  EvaluateArgs    e;
  double          sigma;        // >= 0: the caller's, for every replica; GRLX_SIGMA_OWN: ac_decay * sigma of the replica
  double          theta;        // [0, 1]: the caller's; GRLX_THETA_OWN is resolved on the host
  const uint64_t *inputs;       // [pair][2]: the episode's rand48 state (kNoisyOwnStream = the replica's TL), the bits of its noise state;
                                // null = the replica's TL and 0.0 for every pair
  uint64_t       *streams_out;  // [pair]: the stream after the episode's last step
  double         *noise_out;    // [pair]: the noise state after the episode's last step
  double         *records;      // trajectory kernel only: [pair][max_steps][R], R = noisy_trajectory_words(), zero-filled by the caller
};

int noisy_trajectory_words(int env);       // trajectory_words(env, false) + 2; 0 for an environment without an instantiation
hipError_t launch_evaluate_noisy(const DevParams &P, const NoisyArgs &A, hipStream_t stream);          // the actor-critic only
hipError_t launch_trajectory_noisy(const DevParams &P, const NoisyArgs &A, hipStream_t stream);        // the actor-critic only

} // namespace grlx
