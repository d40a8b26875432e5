// grlx_lspi_evaluate_sampled.h -- the LSPI context's sampled episodes (grlx_lspi_evaluate_sampled*, grlx_lspi_evaluate_ensemble_sampled*):
// what grlx_api_lspi.cpp hands to the kernels of grlx_lspi_evaluate_sampled.hip.  Included by those two only, after grlx_lspi_evaluate.h.
#pragma once
#include "grlx_lspi_evaluate.h"

namespace grlx {

constexpr int kLspiSampledTrajWords = kLspiTrajWords + 1;              // ... then `explored`
constexpr int kLspiEnsSampledTrajWords = kLspiEnsTrajWords + 2;        // ... then `explored`, `prob`

struct LspiSampledArgs {
  LspiEvalArgs e;                                  // e.records: [n_replicas][n_starts][max_steps][kLspiSampledTrajWords]
  int32_t sampler;                                 // GRLX_SAMPLER_*
  double  epsilon;                                 // [0, 1]
  const uint64_t *streams;                         // [n_replicas][n_starts][2]: {sampler's, global}; null: {0, the replica's G}
  int32_t  *explored;                              // [n_replicas][n_starts]
  uint64_t *streams_out;                           // [n_replicas][n_starts][2]
};

// The sampled ensemble: a WAVE per (group, start state) pair.  Once per step the wave writes the projection of (obs, a_k), k < A, as
// (index, weight) pairs in the order of S5 into its own region of LDS: `cap` slots per action -- 8 under the triangle projector, the
// largest box lspi_box can give under Gauss -- and the number of pairs kept per action behind them.
constexpr int kLspiEnsWave = 64;
constexpr int kLspiEnsMaxWaves = 4;                                    // episodes of one group per block, where their regions fit
constexpr size_t kLspiEnsLdsLimit = 64 * 1024;                         // what a block may take without asking the runtime for more
constexpr size_t lspi_ens_wave_bytes(int A, int cap)
{ // weights [A][cap], indices [A][cap], counts [kMaxActions]; a multiple of 16 bytes, so that the next wave's doubles are aligned
  return ((size_t)A * (size_t)cap * (sizeof(double) + sizeof(int32_t)) + kMaxActions * sizeof(int32_t) + 15) & ~(size_t)15;
}
static_assert(lspi_ens_wave_bytes(kMaxActions, kLspiMaxF) <= kLspiEnsLdsLimit, "one wave's pairs fit at the bound of features and actions");

struct LspiEnsSampledArgs {
  LspiEnsArgs e;                                   // e.rule: GRLX_ENSEMBLE_MAJORITY / _RANK; e.records: [...][kLspiEnsSampledTrajWords]
  double  tau;                                     // the combined softmax's temperature, > 0
  int32_t member;                                  // GRLX_MEMBER_*
  double  member_param;                            // e in [0, 1] (EPSILON), tau_m > 0 (SOFTMAX)
  int32_t cap;                                     // slots per action of a wave's region (the launcher sets it)
  const uint64_t *streams;                         // [groups][n_starts]; null: G of the group's first replica
  int32_t  *explored;                              // [groups][n_starts]
  uint64_t *streams_out;                           // [groups][n_starts]
};

// the episodes of a chunk for `rows` replicas (groups); every output pointer is written without a test, e.records null: the sums alone
hipError_t launch_lspi_evaluate_sampled(const LspiParams &L, const LspiSampledArgs &A, int rows, hipStream_t stream);
hipError_t launch_lspi_evaluate_ensemble_sampled(const LspiParams &L, LspiEnsSampledArgs A, int rows, hipStream_t stream);

} // namespace grlx
