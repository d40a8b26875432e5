// grlx_query.h -- the policy queries (grlx_query_q / _state / _ensemble): what grlx_api.cpp hands to the kernels of grlx_query.hip.
// Included by those two only: no rollout kernel sees it, and DevParams does not grow.
#pragma once
#include "grlx_internal.h"

namespace grlx {

// One chunk of observations for a range of replicas; every pointer is a device pointer.  A pair is (replica, observation) with the
// index (replica - first_replica) * n_obs + observation: the layout of every per-pair array.
struct QueryArgs {
  int32_t       first_replica, n_replicas;
  int32_t       n_obs;        // observations of this chunk
  const double *obs;          // [n_obs][observation dimensions]
  double       *q;            // [pair][A]   query_q_kernel; null = not wanted
  double       *value;        // [pair]      query_q_kernel: QPolicy::value; query_state_kernel: the table read; null = not wanted
  int32_t      *greedy;       // [pair]      first maximum; null = not wanted
  int32_t      *n_max;        // [pair]      number of maxima; null = not wanted
};

hipError_t launch_query_q(const DevParams &P, const QueryArgs &A, hipStream_t stream);                    // P.A must be 3 or 5
hipError_t launch_query_state(const DevParams &P, int table, const QueryArgs &A, hipStream_t stream);
// out[n_groups][n_obs][2 + 2A] = { sum value, sum value * value, sum q[0..A), votes[0..A) } over the group_size consecutive replicas of a
// group, in ascending order; q / value / greedy as query_q_kernel wrote them for n_groups * group_size replicas
hipError_t launch_query_reduce(int A, int n_groups, int group_size, int n_obs, const double *q, const double *value, const int32_t *greedy,
                               double *out, hipStream_t stream);

} // namespace grlx
