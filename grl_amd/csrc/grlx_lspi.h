// grlx_lspi.h -- the batch path's second predictor (grlx_lspi_*): what grlx_api_lspi.cpp hands to the kernels of grlx_lspi.hip.
// Included by those two only.
//
// experiment/batch_learning + predictor/lspi + representation/parameterized/linear over projector/rbf/triangle or projector/rbf/gauss on
// the (observation ++ action) pair of the pendulum swing-up, R independently seeded replicas per GPU.  Reference: batch_learning.cpp:
// 88-205, lspi.cpp:110-206, rbf.cpp:99-211, linear.cpp:136-180.  PARITY UNPINNED, as for FQI: Eigen's sums and its LU have no order that
// can be restated.  The specification (DESIGN.md section 4.4 repeats it):
//
//   S1  Sampling.  fqi_generate_kernel's, draw for draw: four draws per transition from the thread-local stream, invert, one model step.
//       The store keeps the raw (obs, action), the next observation, the reward and the absorbing flag.
//   S2  Initial weights.  w0[k] = init_min + u_k (init_max - init_min), u_k = draw k of the initialisation stream srand48(seed).
//   S3  Triangle projection (rbf.cpp:99-150), operation for operation: gridpos = min(max((in - min) / delta, 0), steps - 1 - 1e-10),
//       truncation, 8 (index, weight) pairs in the reference's ii order, each weight the product over dd ascending from 1.
//   S4  Gauss projection (rbf.cpp:173-211), basis functions in index order (dimension 0 fastest).
//   S5  Read (linear.cpp:155-158): Q = sum over the projection's pairs in their order of w[index] * weight, products and sums rounded
//       separately, from 0.
//   S6  phi as it enters A and b: entries with |weight| <= 1e-5 are dropped (sparseView(1., 0.00001)); reads use the unpruned projection.
//   S7  Per rebuild: A_s = 1e-5 I + Phi^T Phi and b = Phi^T r over the whole store.
//   S8  Per iteration: best_j = the first maximum over the action_steps next-state actions of the read on the current weights (a NaN is
//       never larger); A = A_s - Phi^T Psi, Psi_j = gamma^tau phi(s'_j, a_best) (pruned as S6, then scaled); an absorbing transition
//       contributes no Psi (the pendulum never produces one: the flag is carried, the branch unreachable); then A w = b by LU with
//       partial pivoting -- first largest magnitude, lowest row on equal magnitude.
//   S9  A zero or non-finite pivot sets ST_LSPI_PIVOT, which grlx_lspi_sync returns as an error.
//   S10 After the last iteration one greedy test trial from the task's start state: first maximum, ties counted; one row.
//
// Deviations from the reference:
//   D1  Initialisation draws come from a stream of their own (S2), as fqi.c D1; the reference draws them from the thread-local stream.
//   D2  Gauss: diff_dd = (min_dd - in_dd) / delta_dd + k_dd, one addition instead of k repeated ones.
//   D3  Gauss: distsq = (diff_0^2 + diff_1^2) + diff_2^2, summed over dd ascending (Eigen's dot has no fixed order).
//   D4  Gauss: a basis function is kept where distsq < -sigma^2 log(cutoff), the bound computed once on the host.
//   D5  Gauss: weight = pexp(-distsq / sigma^2), the portable exponential (oracle/portable_math.c: orc_pexp).
//   D6  The sums of A_s, b and Phi^T Psi run in the order of section "accumulation" below, not Eigen's; the elimination order inside the
//       LU is the blocked one of lspi_solve_kernel.  Both are fixed: two runs of one context give the same bytes.
//   D7  The test trial takes the first maximum (S10); the reference's greedy sampler draws among ties from the global stream.
#pragma once
#include "grlx_internal.h"

namespace grlx {

constexpr int kLspiNIn = 3;                // task/pendulum/swingup: observation (2) ++ action (1)
constexpr int kLspiD = 2;
constexpr int kLspiS = 3;
constexpr int kLspiMaxF = 512;             // features the kernels are built for (the reference's file: 11 * 11 * 3 = 363): two LDS slabs fit
constexpr uint32_t ST_LSPI_PIVOT = 64u;

// ---- accumulation (lspi_accumulate_kernel).  C = X^T Y over the store, X = Phi; Y = [Phi | r] (pass 0: A_s and b, the upper triangle
// of tiles only) or Psi (pass 1).  A tile is 16 x 16; a wave keeps kLspiTilesPerWave accumulator tiles, a block of four waves
// kLspiTilesPerBlock consecutive tiles of the pass's tile list.  The store is cut into `splits` chunks of `chunk` transitions (a multiple
// of the slab); a block walks its chunk a slab of kLspiSlab transitions at a time.  Partial tiles go to `partials`, which
// lspi_reduce_kernel adds in ascending chunk order.
constexpr int kLspiSlab = 16;              // transitions projected into LDS at a time (4 K-steps of the matrix instruction)
constexpr int kLspiTilesPerWave = 8;
constexpr int kLspiTilesPerBlock = 4 * kLspiTilesPerWave;
constexpr int kLspiChunkMin = 256;         // a chunk is at least this many transitions ...
constexpr int kLspiMaxSplits = 16;         // ... and there are at most this many chunks

// padded feature count, and the pitch of an LDS slab row in doubles: room for the tile of r behind the features, and = 16 (mod 32) so
// that the operand reads of two consecutive K rows (16 doubles each) fall on disjoint halves of the 64 banks
constexpr int lspi_padded(int F) { return (F + 15) / 16 * 16; }
constexpr int lspi_pitch(int Fp) { return Fp % 32 == 0 ? Fp + 16 : Fp + 32; }
// tiles of a pass: the upper triangle plus the column of r-tiles (pass 0), the full square (pass 1)
constexpr int lspi_tiles(int T, int pass) { return pass == 0 ? T * (T + 1) / 2 + T : T * T; }
inline int lspi_splits(int n) { const int s = (n + kLspiChunkMin - 1) / kLspiChunkMin; return s < 1 ? 1 : s > kLspiMaxSplits ? kLspiMaxSplits : s; }
inline int lspi_chunk(int n) { const int s = lspi_splits(n); return ((n + s - 1) / s + kLspiSlab - 1) / kLspiSlab * kLspiSlab; }

struct LspiRep {                           // per-replica state between launches
  uint64_t G, TL;                          // global / thread-local streams, seeded as the FQI context seeds them
  int64_t  n;                              // transitions stored
  int64_t  batches_done;
  int64_t  ties;                           // steps of the test trials at which the maximum was not unique
  uint32_t status;
  uint32_t rows;
};

struct LspiParams {
  DevParams env;                           // h, integration_steps, timeout, randomization of the pendulum
  int32_t  R, A, F, Fp, LP, batch_size, cap, max_rows, projector;      // LP: row pitch of the LU's work copy [A | b], Fp + 16
  int32_t  steps[kLspiNIn], stride[kLspiNIn];
  double   in_min[kLspiNIn], delta[kLspiNIn], top[kLspiNIn];            // top = steps - 1 - 1e-10
  double   sigmasq, cutoff_distsq;
  double   actions[kMaxActions];
  double   obs_min[kLspiD], obs_range[kLspiD], action_min, action_range;
  double   gamma_tau, init_min, init_range;
  LspiRep *rep;
  double  *in, *next_obs, *reward;         // [R][cap][3], [R][cap][2], [R][cap]
  int32_t *absorbing, *best;               // [R][cap]
  double  *w;                              // [R][2][Fp]: the current weights, those of the last greedy choice
  double  *As, *Asys, *b;                  // [R][Fp][Fp] twice, [R][Fp]
  double  *lu;                             // [R][Fp][LP]
  double  *partials;                       // [R][splits][tiles][256]
  size_t   partials_per_replica;           // doubles
  double  *row_reward;                     // [R][max_rows]
  int64_t *row_batch, *row_transitions;
};

// the launchers of grlx_lspi.hip; every pointer is a device pointer
hipError_t launch_lspi_init(const LspiParams &L, const uint64_t *r0, hipStream_t stream);
// one batch: generate, rebuild (A_s and b once, then iterations x (greedy choice, Phi^T Psi, solve)), the test trial
hipError_t launch_lspi_batch(const LspiParams &L, int batches_run, int iterations, hipStream_t stream);
// lspi_solve_kernel alone, on whatever Asys and b hold: one block per replica, w[1] = w[0], w[0] = x, ST_LSPI_PIVOT or-ed into the status
hipError_t launch_lspi_solve(const LspiParams &L, hipStream_t stream);
hipError_t launch_lspi_query(const LspiParams &L, int first_replica, int n_replicas, const double *obs, int n_obs, double *q, hipStream_t stream);

} // namespace grlx
