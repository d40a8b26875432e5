// grlx_evaluate_stream.h -- streamed trajectories (grlx_evaluate_trajectory_stream): what grlx_api_read.cpp hands to the kernels of
// grlx_evaluate_stream.hip.  Included by those two only.  The chunk is grlx_evaluate_trajectory's (TrajectoryArgs), with one difference in
// what the launcher expects of the records: nothing.  The kernels write every word of every live pair's column themselves.
#pragma once
#include "grlx_internal.h"
#include "grlx_evaluate.h"

namespace grlx {

// launch_trajectory's grid on `stream`; A.records need NOT be zero-filled
hipError_t launch_trajectory_stream(const DevParams &P, const TrajectoryArgs &A, hipStream_t stream);

} // namespace grlx
