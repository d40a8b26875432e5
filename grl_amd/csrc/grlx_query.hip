// grlx_query.hip -- the read side of the policies (grlx_query_q / _state / _ensemble): Q-values, state values and greedy actions of
// every replica at observations of the caller's choice.  Reference: QPolicy::values / value / act const (q.cpp:94-107, 56-68, 129-141),
// GreedySampler::findmax / distribution (greedy.cpp:47-61, 88-98), ActionPolicy::read (action.cpp:99-112), LinearRepresentation::read
// (linear.cpp:136-184).
//
// A query writes to nothing but its own output arrays.  Slots are resolved as table_peek resolves them -- the key words of the home
// bucket, the following buckets only while a bucket is full of other slots -- and a slot without an entry contributes initial_weight():
// no entry is created, no counter, stream, trace or key bit is touched.
//
// Layout.  A 16-lane group serves one (replica, observation) pair, lane = tiling, four pairs per wave, four waves per block (no wave
// waits for another: every LDS region belongs to one wave).  Pair = replica * n_obs + observation, so the groups of a wave mostly probe
// one replica's table.  The kernels are bound by the latency of two dependent global loads per probe (key words, then the value): each
// lane issues the key loads of all its probes before it uses any, then all value loads; what hides the rest is other waves on the SIMD,
// hence no scratch and a register count far below the rollout kernels'.
//
// LDS.  A row (action) holds the 64 weights of the wave by lane ([group][tiling]), rows kRowStride = 66 doubles apart.  The write
// is a ds_write_b64 of consecutive addresses (16-lane groups, banks mod 32 dwords: 32 consecutive dwords per group, conflict-free).
// The serial sums are read by lane a of each group with ds_read_b64, whose banks are (byte address / 4) mod 64 over a 32-lane half:
// the lanes (group g, row a) of one half sit at dword 132 a + 32 g + 2 k, bank 4 a + 32 (g & 1) + 2 k mod 64 and the one after it
// -- all different for a < 8.  With a stride of 64 every row would fall on the same banks: NA-way.
//
// Compiled with -ffp-contract=off like every unit: value * value and q * dist are plain products, the sums plain additions.
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_query_weights.h"    // query_weights, query_clamp, kQueryWaves, kRowStride: shared with grlx_evaluate.hip
#include "grlx_query.h"

namespace grlx {

// QPolicy::values, GreedySampler::findmax and QPolicy::value under the greedy sampler, for the pairs of one chunk
template <int NA>
__global__ __launch_bounds__(kQueryWaves * 64) void query_q_kernel(DevParams P, QueryArgs A)
{
  constexpr int T = kLanesPerReplica;
  __shared__ double sh_w[kQueryWaves][NA * kRowStride];
  __shared__ double sh_q[kQueryWaves][4 * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_obs;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;                    // dead groups of the last wave neither load nor store
  double *W = sh_w[wave], *Q = sh_q[wave];
  const int D = P.tile.D - 1;                          // the projector's input is (observation, action)

  if (live)
  {
    const int rl = (int)(pair / A.n_obs), o = (int)(pair - (long long)rl * A.n_obs);
    const int r = A.first_replica + rl;
    // project(obs, a_k), k < NA: the hash of the observation once, then the action's coordinate and the tiling (tile_coding.cpp:103-149)
    uint32_t hpre = 449u ^ (uint32_t)(D + 2);
    for (int i = 0; i < D; ++i)
      hpre = murmur_mix(hpre, tile_coord<T>(P.tile, i, tile_quant(P.tile, i, A.obs[(size_t)o * D + i]), j));
    uint32_t slot[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
    {
      uint32_t h = murmur_mix(hpre, tile_coord<T>(P.tile, D, tile_quant(P.tile, D, P.actions[a]), j));
      h = murmur_mix(h, j);
      slot[a] = murmur_final(h) % (uint32_t)P.tile.memory;
    }
    double w[NA];
    query_weights<NA>(table_of(P, 0, r), P.states[r], 0, P.lin, slot, w);
#pragma unroll
    for (int a = 0; a < NA; ++a) W[a * kRowStride + lane] = w[a];
  }
  wave_sync();
  if (live && j < NA)
  { // LinearRepresentation::read (linear.cpp:136-184): serial sum over the 16 tilings, mean, clamp
    double sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += W[j * kRowStride + g * 16 + k];
    sum /= 16;
    sum = query_clamp(sum, P.lin.out_min, P.lin.out_max);
    if (A.q) A.q[(size_t)pair * NA + j] = sum;
    Q[g * 8 + j] = sum;
  }
  wave_sync();
  if (live && j == 0)
  {
    double q[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) q[a] = Q[g * 8 + a];
    int mai = 0, man = 1;                               // greedy.cpp:47-61; best = values[mai]
    double best = q[0];
#pragma unroll
    for (int a = 1; a < NA; ++a)
    {
      if (q[a] > best) { best = q[a]; mai = a; man = 1; }
      else if (q[a] == best) man++;
    }
    double v = 0;                                       // q.cpp:56-68 over greedy.cpp:88-98
#pragma unroll
    for (int a = 0; a < NA; ++a) v += q[a] * (q[a] == best ? 1. / man : 0.);
    if (A.value) A.value[pair] = v;
    if (A.greedy) A.greedy[pair] = mai;
    if (A.n_max) A.n_max[pair] = man;
  }
}

// the read of a table whose projector takes the observation alone (table 0: P.tile / P.lin, table 1: P.tile_actor / P.lin_actor)
__global__ __launch_bounds__(kQueryWaves * 64) void query_state_kernel(DevParams P, int table, QueryArgs A)
{
  __shared__ double sh_w[kQueryWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const long long n_pairs = (long long)A.n_replicas * A.n_obs;
  const long long pair = ((long long)blockIdx.x * kQueryWaves + wave) * 4 + g;
  const bool live = pair < n_pairs;
  double *W = sh_w[wave];
  const TileParams &tp = table == 1 ? P.tile_actor : P.tile;
  const LinearParams &lp = table == 1 ? P.lin_actor : P.lin;

  if (live)
  {
    const int rl = (int)(pair / A.n_obs), o = (int)(pair - (long long)rl * A.n_obs);
    const int r = A.first_replica + rl;
    uint32_t slot[1] = {tile_slot_generic(tp, A.obs + (size_t)o * tp.D, j)};
    double w[1];
    query_weights<1>(table_of(P, table, r), P.states[r], table, lp, slot, w);      // twin tables: each holds its own keys
    W[lane] = w[0];
  }
  wave_sync();
  if (live && j == 0)
  {
    double sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += W[g * 16 + k];
    sum /= 16;
    A.value[pair] = query_clamp(sum, lp.out_min, lp.out_max);
  }
}

// one thread per (group, observation, column): a serial loop over the group's replicas, ascending
__global__ __launch_bounds__(256) void query_reduce_kernel(int NA, int n_groups, int group_size, int n_obs, const double *q, const double *value,
                                                           const int32_t *greedy, double *out)
{
  const int cols = 2 + 2 * NA;
  const long long total = (long long)n_groups * n_obs * cols;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % cols);
  const long long go = i / cols;
  const int o = (int)(go % n_obs), grp = (int)(go / n_obs);
  double s = 0;
  for (int m = 0; m < group_size; ++m)
  {
    const size_t pair = ((size_t)grp * group_size + m) * (size_t)n_obs + o;
    double x;
    if (c == 0) x = value[pair];
    else if (c == 1) { const double v = value[pair]; x = v * v; }
    else if (c < 2 + NA) x = q[pair * NA + (c - 2)];
    else x = greedy[pair] == c - 2 - NA ? 1. : 0.;
    s += x;
  }
  out[i] = s;
}

static unsigned query_blocks(const QueryArgs &A)
{
  const long long pairs = (long long)A.n_replicas * A.n_obs;
  return (unsigned)((pairs + 4 * kQueryWaves - 1) / (4 * kQueryWaves));
}

hipError_t launch_query_q(const DevParams &P, const QueryArgs &A, hipStream_t stream)
{
  const unsigned blocks = query_blocks(A);
  if (blocks == 0) return hipSuccess;
  if (P.A == 3) hipLaunchKernelGGL(query_q_kernel<3>, dim3(blocks), dim3(kQueryWaves * 64), 0, stream, P, A);
  else if (P.A == 5) hipLaunchKernelGGL(query_q_kernel<5>, dim3(blocks), dim3(kQueryWaves * 64), 0, stream, P, A);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_query_state(const DevParams &P, int table, const QueryArgs &A, hipStream_t stream)
{
  const unsigned blocks = query_blocks(A);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(query_state_kernel, dim3(blocks), dim3(kQueryWaves * 64), 0, stream, P, table, A);
  return hipGetLastError();
}

hipError_t launch_query_reduce(int A, int n_groups, int group_size, int n_obs, const double *q, const double *value, const int32_t *greedy,
                               double *out, hipStream_t stream)
{
  const long long total = (long long)n_groups * n_obs * (2 + 2 * A);
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(query_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, A, n_groups, group_size, n_obs, q, value,
                     greedy, out);
  return hipGetLastError();
}

} // namespace grlx
