// grlx_lspi_evaluate.h -- the LSPI context's evaluation episodes and ensemble (grlx_lspi_evaluate*, grlx_lspi_query_ensemble): what
// grlx_api_lspi.cpp hands to the kernels of grlx_lspi_evaluate.hip.  Included by those two only, after grlx_lspi.h.
#pragma once
#include "grlx_lspi.h"

namespace grlx {

constexpr int kLspiTrajWords = GRLX_TRAJ_OBS + kLspiD + kLspiS;             // 11
constexpr int kLspiEnsTrajWords = GRLX_TRAJ_ENS_OBS + kLspiD + kLspiS;      // 13

// The layout of every kernel of the unit: a QUAD of four lanes per episode (or observation), lane a of the quad owning the actions
// a, a + 4 (kLspiOwn of them); a block of 256 threads is 64 quads of one replica or group
constexpr int kLspiQuad = 4;
constexpr int kLspiOwn = kMaxActions / kLspiQuad;
constexpr int kLspiEvalBlock = 256, kLspiEvalQuads = kLspiEvalBlock / kLspiQuad;
static_assert(kMaxActions % kLspiQuad == 0, "every lane of a quad owns the same number of action slots");

struct LspiEvalArgs {
  int32_t first_replica, n_starts, max_steps;      // n_starts: of this chunk; max_steps: 1 ... GRLX_MAX_EPISODE_STEPS
  const double *states;                            // [n_starts][3]
  double  *ret, *disc;                             // [n_replicas][n_starts], as are steps, terminal and ties
  int32_t *steps, *terminal, *ties;
  double  *final_state;                            // [n_replicas][n_starts][3]
  double  *records;                                // RECORD: [n_replicas][n_starts][max_steps][kLspiTrajWords]
};

struct LspiEnsArgs {
  int32_t first_replica, group_size, rule, n_starts, max_steps;
  const double *states;                            // [n_starts][3]
  double  *ret, *disc;                             // [groups][n_starts], as are steps, terminal, ties, member_ties and agreement
  int32_t *steps, *terminal, *ties;
  int64_t *member_ties, *agreement;
  double  *final_state;                            // [groups][n_starts][3]
  double  *records;                                // RECORD: [groups][n_starts][max_steps][kLspiEnsTrajWords]
};

// the episodes of a chunk for `rows` replicas (groups); A.records null: the sums alone.  Every pointer is a device pointer.
hipError_t launch_lspi_evaluate(const LspiParams &L, const LspiEvalArgs &A, int rows, hipStream_t stream);
hipError_t launch_lspi_evaluate_ensemble(const LspiParams &L, const LspiEnsArgs &A, int rows, hipStream_t stream);
hipError_t launch_lspi_query_ensemble(const LspiParams &L, int first_replica, int groups, int group_size, const double *obs, int n_obs, double *out,
                                      hipStream_t stream);

} // namespace grlx
