// grlx_fqi.hip -- the batch path (BASELINE.json configs[4]): experiment/batch_learning + predictor/fqi +
// representation/iterative + representation/parameterized/ann over projector/pre/normalizing, R independent-seed
// replicas per GPU.  Reference: batch_learning.cpp:88-205, fqi.cpp:187-285, iterative.cpp:63-107, ann.cpp:133-263,
// normalizing.cpp:78-87, greedy.cpp:47-86.  The operation-by-operation specification (incl. the documented
// deviations D1-D4 from the unpinnable parts of the reference) is oracle/fqi.c; this file restates it for the GPU.
//
// Shape of the work.  A rebuild is `iterations` x (targets + `epochs` x (gradient over all samples + RPROP step)): a
// long chain of tiny dense passes (3 -> H -> 1 per sample, 2 x 101 parameters) whose only coupling is the gradient
// sum.  One lane = one sample; the network (101 doubles) sits in LDS; the per-sample gradient stays in registers
// only as long as it takes to park its factors in LDS, and is summed by the fixed two-level tree of the specification
// (chunks of 64 samples in sample order -> chunk sums strided over 64 lanes + wave shuffle), independent of the grid.  No contraction here is large enough for MFMA
// (K = 3 and K = 20, N = 1; a 16x16x4 f64 tile would be 80 % padding) and the chain is bound by launch latency and
// the reduction, not by FLOPs: see DESIGN.md section 4.3 for the measurement.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_math_batch.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_softmax.h"
#include "grlx_fqi.h"

namespace grlx {
// ANNRepresentation::read (ann.cpp:133-160): net input ((w0 a0 + w1 a1) + w2 a2) + bias, logistic hidden layer, linear output.
// Written stage by stage over the hidden units (per unit the operations and their order are those of the scalar text:
// oracle/fqi.c ann_forward): independent chains for the wave to overlap -- a branchy exp per unit serialises them.  Up to 20
// units are one batch; wider layers go 16 at a time (two batches of stage values would not fit the registers), the output sum
// still adds the units in their order.  a_out: registers (H <= 20) or the lane's row of the factor tile in LDS.
template <int H>
__device__ __forceinline__ double ann_forward(const double *w, const double (&in)[kFqiNIn], double *a_out)
{
  constexpr int CH = (H <= 20) ? H : 16;
  static_assert(H % CH == 0, "hidden units per batch");
  const double *W2 = w + (kFqiNIn + 1) * H;
  double out = 0;
#pragma unroll
  for (int h0 = 0; h0 < H; h0 += CH)
  {
    double net[CH], e[CH];
#pragma unroll
    for (int h = 0; h < CH; ++h)
    {
      double v = 0;
#pragma unroll
      for (int i = 0; i < kFqiNIn; ++i) v += w[(h0 + h) * (kFqiNIn + 1) + i] * in[i];
      v += w[(h0 + h) * (kFqiNIn + 1) + kFqiNIn];
      net[h] = -v;
    }
    plogistic_batch<CH>(net, e);                                  // a = 1 / (1 + exp(-net)), ann.h:108-111; -net clamped to +-690 (fqi.c D5)
#pragma unroll
    for (int h = 0; h < CH; ++h)
    {
      if (a_out) a_out[h0 + h] = e[h];
      out += W2[h0 + h] * e[h];
    }
  }
  out += W2[H];
  return out;
}

__device__ __forceinline__ void fqi_normalise(const FqiParams &F, const double *obs, double action, double (&in)[kFqiNIn])
{ // NormalizingProjector::project (normalizing.cpp:78-87), signed = 0
#pragma unroll
  for (int i = 0; i < kFqiD; ++i) in[i] = (obs[i] - F.in_min[i]) * F.in_scale[i] - 0;
  in[kFqiD] = (action - F.in_min[kFqiD]) * F.in_scale[kFqiD] - 0;
}

// weights: w[i] = 0.01 * (2 u_i - 1) from the initialisation stream (fqi.c D1); eta = Ones, x 0.1 for RPROP (ann.cpp:106-109)
__global__ void fqi_init_kernel(FqiParams F, const uint64_t *r0)
{
  const int r = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= F.P) return;
  double *net = F.net + (size_t)r * 4 * F.P;
  const uint64_t x = lcg_next(lcg_jump(r0[r], (uint64_t)k));
  net[k] = (2 * lcg_double(x) - 1) * 0.01;
  net[F.P + k] = (F.eta == 0) ? 1. * 0.1 : 1.;
  net[2 * F.P + k] = 0;
  net[3 * F.P + k] = 0;
}

// BatchLearningExperiment::run, the sampling loop (batch_learning.cpp:107-138): one lane per transition; the
// replica's thread-local stream is consumed 4 draws per transition in sample order (LCG jump-ahead)
__global__ __launch_bounds__(256) void fqi_generate_kernel(FqiParams F)
{
  const int r = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= F.batch_size) return;
  const FqiRep &rep = F.rep[r];
  uint64_t x = lcg_jump(rep.TL, 4ull * (uint64_t)s);
  double obs[kFqiD];
#pragma unroll
  for (int i = 0; i < kFqiD; ++i) { x = lcg_next(x); obs[i] = 0 + lcg_double(x) * (1 - 0); }
  x = lcg_next(x);
  double action = 0 + lcg_double(x) * (1 - 0);
  // (the fourth draw is next_action: consumed, never read by FQI)
#pragma unroll
  for (int i = 0; i < kFqiD; ++i) obs[i] = F.obs_min[i] + obs[i] * F.obs_range[i];
  action = F.action_min + action * F.action_range;
  double st[kFqiS] = {obs[0] - GRLX_PI, obs[1], 0.};                          // PendulumSwingupTask::invert (pendulum.cpp:147-155)
  double nobs[kFqiD], reward;
  int terminal;
  uint32_t status = 0;
  env_step<GRLX_ENV_PENDULUM, false>(F.env, st, action, nobs, reward, terminal, status);
  const size_t at = (size_t)r * (size_t)F.cap + (size_t)rep.n + (size_t)s;
  double in[kFqiNIn];
  fqi_normalise(F, obs, action, in);
#pragma unroll
  for (int i = 0; i < kFqiNIn; ++i) F.in[at * kFqiNIn + i] = in[i];
#pragma unroll
  for (int i = 0; i < kFqiD; ++i) F.next_obs[at * kFqiD + i] = nobs[i];
  F.reward[at] = reward;
  F.absorbing[at] = terminal == 2 ? 1 : 0;
  F.targets[at] = 0.;
  if (status) atomicOr(&F.rep[r].status, status);
}

// after the generate kernel: the batch is part of the store, the stream has moved on, a rebuild begins
__global__ void fqi_batch_begin_kernel(FqiParams F)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= F.R) return;
  FqiRep &rep = F.rep[r];
  rep.TL = lcg_jump(rep.TL, 4ull * (uint64_t)F.batch_size);
  rep.n += F.batch_size;
  rep.done = 0;
  rep.iterations = 0;
  rep.maxdelta_bits = 0x7FF0000000000000ull;                                  // +inf (fqi.cpp:208)
}

// head of iteration ii of FQIPredictor::rebuild (fqi.cpp:213): `ii < iterations_ && maxdelta > 0.001`
__global__ void fqi_iter_begin_kernel(FqiParams F, int ii)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= F.R) return;
  FqiRep &rep = F.rep[r];
  if (rep.done) return;
  const double md = __longlong_as_double((long long)rep.maxdelta_bits);
  rep.maxdelta_last = md;
  if (!(md > 0.001)) { rep.done = 1; return; }
  rep.iterations = ii + 1;
  rep.maxdelta_bits = 0ull;
}

// targets of one iteration (fqi.cpp:227-262): r + gamma^tau max_a Q(s', a); L-infinity change against the previous targets
template <int H>
__global__ __launch_bounds__(256) void fqi_targets_kernel(FqiParams F, int first_iteration)
{
  __shared__ double sh_net[(kFqiNIn + 1) * H + H + 1];
  __shared__ double sh_max[4];
  const int r = blockIdx.y;
  const FqiRep &rep = F.rep[r];
  if (rep.done) return;
  const double *net = F.net + (size_t)r * 4 * F.P;
  for (int k = threadIdx.x; k < F.P; k += blockDim.x) sh_net[k] = net[k];
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double diff = 0;
  if (s < rep.n)
  {
    const size_t at = (size_t)r * (size_t)F.cap + (size_t)s;
    double target = F.reward[at];
    if (!F.absorbing[at])
    {
      double nobs[kFqiD];
#pragma unroll
      for (int i = 0; i < kFqiD; ++i) nobs[i] = F.next_obs[at * kFqiD + i];
      double v = -__builtin_inf();
      for (int k = 0; k < F.A; ++k)
      {
        double in[kFqiNIn];
        fqi_normalise(F, nobs, F.actions[k], in);
        v = fmax(v, ann_forward<H>(sh_net, in, nullptr));
      }
      target += F.gamma_tau * v;
    }
    const double prev = first_iteration ? 0. : F.targets[at];
    diff = __builtin_fabs(prev - target);
    F.targets[at] = target;
  }
  // max is order-independent: any reduction gives the reference's value
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) diff = fmax(diff, __shfl_down(diff, off, 64));
  if ((threadIdx.x & 63) == 0) sh_max[threadIdx.x >> 6] = diff;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    const double m = fmax(fmax(sh_max[0], sh_max[1]), fmax(sh_max[2], sh_max[3]));
    atomicMax(&F.rep[r].maxdelta_bits, (unsigned long long)__double_as_longlong(m));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The epochs of one iteration in ONE launch: `fqi_epochs_kernel`.
//
// An epoch = the gradient of every stored transition (ann.cpp:224-263), summed, and one RPROP step (ann.cpp:186-192).  The
// specification's sum (oracle/fqi.c) is a fixed tree: level 1 = a chunk of 64 samples in sample order; level 2 = 64 partial
// sums per parameter, the L-th over the chunks L, L+64, L+128, ... in this order; level 3 = v[L] += v[L + off], off = 32..1.
// Level 2 is the mapping: wave (replica r, L) walks ITS chunks in order and keeps its partial sums in registers -- no
// per-chunk sums ever reach memory (round 2 wrote and re-read 41 MB of them per epoch at 16 x 200 000 transitions, in two
// launches per epoch whose dispatch gaps were a quarter of the time).  A block = 4 waves = 4 consecutive L of one replica;
// 16 blocks per replica; 16 replicas fill the 256 CUs with one block each (93 KB of LDS per block: four factor tiles) -- for the
// 20 hidden units of the reference's file; FqiShape<H> gives the numbers of the other instantiated widths (8, 16, 32, 64).
// One wave per SIMD means nothing but the wave's own instruction-level parallelism hides latency: the forward pass is
// written stage by stage over the 20 hidden units (pexp_batch, pdiv_batch: grlx_math.h), the next chunk's inputs are
// loaded while the current one is computed.
// Once per epoch the 64 waves of a replica meet (agent-scope hand-off, cdna_hip_programming.md Guideline 16): every wave
// publishes its 102 partial sums (write-through stores, double-buffered by epoch parity), the block's leader adds 1 to the
// replica's arrival counter and polls it; behind an agent-scope acquire EVERY block runs level 3 and the RPROP step for
// ALL parameters itself (wave w: parameters w, w+4, ...: lane l loads partial sum l, the tree runs in the wave, lane 0
// steps).  The 16 copies are bit-identical, so the network, eta and the previous gradient live in each block's LDS for
// the whole launch and nobody waits for a second hand-off; block 0 of the replica writes them back at the end.
// The replicas never wait for each other.  All blocks of a launch must be resident (they spin on each other): the launch is
// cooperative (the runtime refuses a grid that does not fit) and every spin is bounded -- a wait that runs out raises
// ST_SYNC_TIMEOUT and the block leaves, so the grid always drains.
typedef __attribute__((address_space(1))) unsigned int fqi_gu32;
typedef __attribute__((address_space(1))) unsigned long long fqi_gu64;
#define FQI_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr unsigned kFqiSpinLimit = 4u << 20;            // x (s_sleep 2 + one L2 round trip) = seconds

__device__ __forceinline__ void fqi_publish(double *p, double x)
{ // write-through (sc1) 8-byte store: visible to other XCDs without a release fence once drained
  __hip_atomic_store((fqi_gu64 *)p, (unsigned long long)__double_as_longlong(x), FQI_RLX_AGENT);
}

// All threads of the block call this after their publishing stores.  Returns false when the wait timed out.
__device__ __forceinline__ bool fqi_meet(unsigned int *counter, unsigned target, int *sh_ok)
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its stores ...
  __syncthreads();                                       // ... before the leader signals for all of them
  if (threadIdx.x == 0)
  {
    __hip_atomic_fetch_add((fqi_gu32 *)counter, 1u, FQI_RLX_AGENT);
    bool ok = true;
    for (unsigned spins = 0; __hip_atomic_load((fqi_gu32 *)counter, FQI_RLX_AGENT) < target;)
    {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kFqiSpinLimit) { ok = false; break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // ONE acquire after the match: drops this CU's stale lines
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *sh_ok = ok ? 1 : 0;
  }
  __syncthreads();
  return *sh_ok != 0;
}

// lane i of a row of 16 receives the value of lane i + N of the same row (DPP row_shl: N); lanes past the row's end keep their own
template <int N>
__device__ __forceinline__ double fqi_row_shl(double v)
{
  const long long b = __double_as_longlong(v);
  const int lo = (int)b, hi = (int)(b >> 32);
  const int rlo = __builtin_amdgcn_update_dpp(lo, lo, 0x100 + N, 0xF, 0xF, false);
  const int rhi = __builtin_amdgcn_update_dpp(hi, hi, 0x100 + N, 0xF, 0xF, false);
  return __longlong_as_double(((long long)rhi << 32) | (unsigned int)rlo);
}

// The shape of the epochs kernel for H hidden units.  A lane sums KP parameters (lane, lane + 64, ...: P + 1 <= 64 KP, the extra one
// is the squared error); a wave's factor tile is 64 samples x COLS doubles (COLS odd: a column read by 64 lanes hits 64 banks); as many
// waves per block as their tiles fit the CU's 160 KB of LDS (4 up to 32 hidden units, 2 for 64), 64 waves = the 64 partial sums of
// level 2 per replica.  LDS reads of level 1 go SPB samples (2 KP SPB <= 12 reads) at a time.
template <int H> struct FqiShape {
  static constexpr int P = (kFqiNIn + 1) * H + H + 1;
  static constexpr int KP = (P + 1 + 63) / 64;
  static constexpr int COLS = 2 * H + kFqiNIn + 2;        // in[3], d1[H], a[H], d2, 1.0
  static constexpr int WAVES = ((size_t)4 * 64 * COLS * 8 + 3 * P * 8 + 64 <= 160 * 1024) ? 4 : 2;
  static constexpr int BLOCKS = 64 / WAVES;               // per replica
  // KP == 2 (16 and 20 hidden units): a lane's two terms SHARE a factor (below), three LDS reads per sample instead of four
  static constexpr bool SHARED = KP == 2 && 2 * H + (H + 3) / 2 <= 64;
  static constexpr int RS = SHARED ? 3 : 2 * KP;          // LDS reads per sample and lane
  static constexpr int SPB = 12 / RS;
  static constexpr int QSPLIT = (63 * COLS * 8 <= 65535) ? 64 : 32;      // ds_read offsets are 16 bits: a second base address beyond
  static_assert(KP <= 6 && RS * SPB <= 12 && SPB >= 1, "reads per batch");
  static_assert((size_t)WAVES * 64 * COLS * 8 + 3 * P * 8 + 64 <= 160 * 1024, "factor tiles exceed the LDS");
};

// s_waitcnt lgkmcnt(N) that the compiler may not move the uses of x[] across
template <int N>
__device__ __forceinline__ void fqi_lds_wait(double (&x)[12])
{
  asm volatile("s_waitcnt lgkmcnt(%12)"
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11])
               : "n"(N));
}

template <int H>
__global__ __launch_bounds__(FqiShape<H>::WAVES * 64) void fqi_epochs_kernel(FqiParams F, int r_first, int epochs)
{
  typedef FqiShape<H> Sh;
  constexpr int P = Sh::P, KP = Sh::KP, COLS = Sh::COLS, WAVES = Sh::WAVES, BLOCKS = Sh::BLOCKS, SPB = Sh::SPB, QSPLIT = Sh::QSPLIT, NT = WAVES * 64;
  constexpr int C_IN = 0, C_D1 = kFqiNIn, C_A = kFqiNIn + H, C_D2 = kFqiNIn + 2 * H, C_ONE = C_D2 + 1;
  constexpr int TREES = (P + 1 + WAVES - 1) / WAVES;     // level-3 trees per wave: parameters w, w + WAVES, ... (and the squared error)
  constexpr int GROUPS = (TREES + 3) / 4;                // ... taken four at a time, one per row of 16 lanes
  constexpr int GB = 8;                                  // ... and at most 8 groups of leaves in registers together
  static_assert(COLS == C_ONE + 1, "factor tile width");
  __shared__ double sh_net[P], sh_eta[P], sh_prev[P];
  __shared__ double sh_tile[WAVES][64 * COLS];
  __shared__ int sh_ok;
  const int r = r_first + (int)blockIdx.x / BLOCKS, bl = (int)blockIdx.x % BLOCKS;
  if (r >= F.R || epochs <= 0) return;
  FqiRep &rep = F.rep[r];
  if (rep.done) return;                                  // uniform over the replica's blocks
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int L = bl * WAVES + w;
  const int64_t n = rep.n, chunks = (n + 63) / 64;
  double *net = F.net + (size_t)r * 4 * F.P;
  unsigned int *counter = F.sync + (size_t)r * 4;        // one 16-byte slot per replica
  double *tile = sh_tile[w];
  double *row = tile + lane * COLS;
  for (int k = (int)threadIdx.x; k < P; k += NT)
  {
    sh_net[k] = net[k];
    sh_eta[k] = net[F.P + k];
    sh_prev[k] = net[3 * F.P + k];
  }
  // the two factors of the per-sample gradient terms this lane sums (x * 1.0 is exact) and the parameter each sum belongs to (P: the squared
  // error, ann.cpp:240; -1: none).  General layout: parameters lane, lane + 64, ...  SHARED layout (two terms per lane): the two share one
  // factor, so a sample costs three LDS reads instead of four -- layer 1: lane (h, pair) sums Delta1(2 pair, h) and Delta1(2 pair + 1, h),
  // both times d1[h]; layer 2, its bias and the error: neighbours two by two, all times d2.  Which lane sums a parameter does not touch the
  // order of its sum (samples of a chunk in order, then the fixed tree).
  constexpr bool SHARED = Sh::SHARED;
  int cx[KP], cy[KP], pidx[KP];
  if constexpr (SHARED)
  {
    constexpr int L1 = 2 * H, E2 = H + 2, L2 = (E2 + 1) / 2;
    static_assert(L1 + L2 <= 64, "lanes of the shared-factor layout");
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
      if (lane < L1)
      {
        const int h = lane >> 1, i = 2 * (lane & 1) + k;
        cx[k] = (i < kFqiNIn) ? C_IN + i : C_ONE;                  // Delta1(i, h) += a0[i] * d1[h]; bias row: d1[h]
        cy[k] = C_D1 + h;
        pidx[k] = h * (kFqiNIn + 1) + i;
      }
      else
      {
        const int q = 2 * (lane - L1) + k;
        cy[k] = C_D2;
        if (lane < L1 + L2 && q < H) { cx[k] = C_A + q; pidx[k] = (kFqiNIn + 1) * H + q; }   // Delta2(h) += a1[h] * d2
        else if (lane < L1 + L2 && q == H) { cx[k] = C_ONE; pidx[k] = P - 1; }                // bias: d2
        else if (lane < L1 + L2 && q == H + 1) { cx[k] = C_D2; pidx[k] = P; }                 // squared error
        else { cx[k] = C_D2; pidx[k] = -1; }
      }
    }
  }
  else
  {
#pragma unroll
    for (int k = 0; k < KP; ++k)
    {
      const int p = lane + 64 * k;
      pidx[k] = (p <= P) ? p : -1;
      if (p < (kFqiNIn + 1) * H)
      {
        const int h = p / (kFqiNIn + 1), i = p % (kFqiNIn + 1);
        cx[k] = (i < kFqiNIn) ? C_IN + i : C_ONE;                  // Delta1(i, h) += a0[i] * d1[h]; bias row: d1[h]
        cy[k] = C_D1 + h;
      }
      else if (p < P - 1) { cx[k] = C_A + (p - (kFqiNIn + 1) * H); cy[k] = C_D2; }   // Delta2(h) += a1[h] * d2
      else if (p == P - 1) { cx[k] = C_ONE; cy[k] = C_D2; }                          // bias: d2
      else { cx[k] = C_D2; cy[k] = C_D2; }                                           // p == P: squared error (ann.cpp:240); beyond: unused
    }
  }
  row[C_ONE] = 1.;                                        // the constant factor of the bias terms: written once
  const size_t base = (size_t)r * (size_t)F.cap;
  double last_error = 0.;
  bool has_error = false;                                 // this lane ran the tree of the squared error
  __syncthreads();
#define FQI_STAMP(k) do { if (F.stamps && e < 4 && bl < kFqiStampBlocks && threadIdx.x == 0) F.stamps[(((size_t)r * kFqiStampBlocks + bl) * 4 + e) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
  for (int e = 0; e < epochs; ++e)
  {
    FQI_STAMP(0);
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.;
    // inputs of the wave's first chunk; inside the loop the next chunk's are requested before the current one is worked on
    double nin[kFqiNIn] = {0., 0., 0.}, ntarget = 0.;
    if (L < chunks && (int64_t)L * 64 + lane < n)
    {
      const size_t at = base + (size_t)L * 64 + (size_t)lane;
#pragma unroll
      for (int i = 0; i < kFqiNIn; ++i) nin[i] = F.in[at * kFqiNIn + i];
      ntarget = F.targets[at];
    }
    for (int64_t c = L; c < chunks; c += 64)
    { // level 1: one chunk of 64 samples; lane = sample for the forward / backward pass (ann.cpp:224-263)
      const int64_t s = c * 64 + lane;
      double in[kFqiNIn];
#pragma unroll
      for (int i = 0; i < kFqiNIn; ++i) in[i] = nin[i];
      const double target = ntarget;
      if (c + 64 < chunks && s + 64 * 64 < n)
      {
        const size_t at = base + (size_t)s + 64 * 64;
#pragma unroll
        for (int i = 0; i < kFqiNIn; ++i) nin[i] = F.in[at * kFqiNIn + i];
        ntarget = F.targets[at];
      }
      if (c == L) FQI_STAMP(5);
      if (s < n)
      {
        const double *W2 = sh_net + (kFqiNIn + 1) * H;
        if constexpr (H <= 20)
        { // the activations stay in registers between the two passes
          double a[H];
          const double out = ann_forward<H>(sh_net, in, a);
          if (c == L) FQI_STAMP(6);
          const double d2 = out - target;
#pragma unroll
          for (int i = 0; i < kFqiNIn; ++i) row[C_IN + i] = in[i];
#pragma unroll
          for (int h = 0; h < H; ++h)
          {
            row[C_D1 + h] = (W2[h] * d2) * (a[h] * (1. - a[h]));       // ann.cpp:249 with deviation D2
            row[C_A + h] = a[h];
          }
          row[C_D2] = d2;
        }
        else
        { // the activations go to the lane's row as they are produced and are read back for the hidden deltas
          const double out = ann_forward<H>(sh_net, in, row + C_A);
          asm volatile("" ::: "memory");                               // (read back from the row: do not keep H activations live in registers)
          if (c == L) FQI_STAMP(6);
          const double d2 = out - target;
#pragma unroll
          for (int i = 0; i < kFqiNIn; ++i) row[C_IN + i] = in[i];
#pragma unroll
          for (int h = 0; h < H; ++h)
          {
            const double ah = row[C_A + h];
            row[C_D1 + h] = (W2[h] * d2) * (ah * (1. - ah));           // ann.cpp:249 with deviation D2
          }
          row[C_D2] = d2;
        }
      }
      // the tile belongs to this wave alone: its LDS writes are complete before its LDS reads issue (in-order LDS, one wave)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int n_here = (int)((n - c * 64 < 64) ? n - c * 64 : 64);
      if (c == L) FQI_STAMP(7);
      { // the lane turns into one lane per PARAMETER (KP of them): per-sample products added in sample order (level 1), then level 2
        double v[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) v[k] = 0.;
        if (n_here == 64)
        { // 128 KP LDS reads per wave and chunk: issued as plain ds_read_b64 (2 LDS cycles each; the compiler pairs neighbouring rows
          // into ds_read2_b64, 8 cycles per pair: MI355X_MICROARCH.md, LDS table), SPB samples (<= 12 reads) per batch, the next
          // batch in flight while the current one is multiplied and added (lgkmcnt counts at most 15 operations)
          constexpr int RS = Sh::RS, RPB = RS * SPB, NB = 64 / SPB, REM = 64 % SPB;
          double x[2][12];
          const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) double *)tile;
          unsigned a_cx[64 / QSPLIT][KP], a_cy[64 / QSPLIT][KP];
#pragma unroll
          for (int hf = 0; hf < 64 / QSPLIT; ++hf)
#pragma unroll
            for (int k = 0; k < KP; ++k)
            {
              a_cx[hf][k] = lds0 + (unsigned)(hf * QSPLIT * COLS + cx[k]) * 8u;
              a_cy[hf][k] = lds0 + (unsigned)(hf * QSPLIT * COLS + cy[k]) * 8u;
            }
#define FQI_RD(dst, addr, off) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define FQI_ISSUE(buf, q0, cnt)                                                                                           \
          _Pragma("unroll") for (int t = 0; t < (cnt); ++t)                                                                \
          {                                                                                                               \
            if constexpr (SHARED)                                                                                         \
            {                                                                                                             \
              FQI_RD(x[buf][3 * t + 0], a_cy[((q0) + t) / QSPLIT][0], (((q0) + t) % QSPLIT) * COLS * 8);                   \
              FQI_RD(x[buf][3 * t + 1], a_cx[((q0) + t) / QSPLIT][0], (((q0) + t) % QSPLIT) * COLS * 8);                   \
              FQI_RD(x[buf][3 * t + 2], a_cx[((q0) + t) / QSPLIT][1], (((q0) + t) % QSPLIT) * COLS * 8);                   \
            }                                                                                                             \
            else                                                                                                          \
            {                                                                                                             \
              _Pragma("unroll") for (int k = 0; k < KP; ++k)                                                               \
              {                                                                                                           \
                FQI_RD(x[buf][2 * (t * KP + k) + 0], a_cx[((q0) + t) / QSPLIT][k], (((q0) + t) % QSPLIT) * COLS * 8);        \
                FQI_RD(x[buf][2 * (t * KP + k) + 1], a_cy[((q0) + t) / QSPLIT][k], (((q0) + t) % QSPLIT) * COLS * 8);        \
              }                                                                                                           \
            }                                                                                                             \
          }
#define FQI_USE(buf, cnt)                                                                                                 \
          _Pragma("unroll") for (int t = 0; t < (cnt); ++t)                                                                \
          {                                                                                                               \
            if constexpr (SHARED)                                                                                         \
            {                                                                                                             \
              v[0] += x[buf][3 * t + 1] * x[buf][3 * t + 0];                                                              \
              v[1] += x[buf][3 * t + 2] * x[buf][3 * t + 0];                                                              \
            }                                                                                                             \
            else                                                                                                          \
            {                                                                                                             \
              _Pragma("unroll") for (int k = 0; k < KP; ++k) v[k] += x[buf][2 * (t * KP + k) + 0] * x[buf][2 * (t * KP + k) + 1]; \
            }                                                                                                             \
          }
#define FQI_BATCH(cur, nxt)                                                                                               \
          {                                                                                                               \
            if (b + 1 < NB) { FQI_ISSUE(nxt, SPB * (b + 1), SPB); fqi_lds_wait<RPB>(x[cur]); }                             \
            else if (REM) { FQI_ISSUE(nxt, SPB * NB, REM); fqi_lds_wait<RS * REM>(x[cur]); }                               \
            else fqi_lds_wait<0>(x[cur]);                                                                                 \
            FQI_USE(cur, SPB);                                                                                            \
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the tile writes of this wave have left for the LDS
          FQI_ISSUE(0, 0, SPB);
#pragma unroll
          for (int b = 0; b < NB; ++b)
          { // batch b = samples SPB b .. SPB b + SPB - 1 (and one last batch of the REM samples that remain)
            if (b & 1) FQI_BATCH(1, 0)
            else FQI_BATCH(0, 1)
          }
          if (REM)
          {
            fqi_lds_wait<0>(x[NB & 1]);
            FQI_USE(NB & 1, REM);
          }
#undef FQI_RD
#undef FQI_ISSUE
#undef FQI_USE
#undef FQI_BATCH
        }
        else
          for (int q = 0; q < n_here; ++q)
#pragma unroll
            for (int k = 0; k < KP; ++k) v[k] += tile[q * COLS + cx[k]] * tile[q * COLS + cy[k]];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] += v[k];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    FQI_STAMP(1);
    // the hand-off: the 64 partial sums of every parameter (buffer e mod 2: a block that is one epoch ahead writes the other one)
    double *vL = F.vL + ((size_t)(e & 1) * (size_t)F.R + (size_t)r) * 64 * (size_t)(P + 1);
#pragma unroll
    for (int k = 0; k < KP; ++k)                                     // [parameter][L]: the 64 leaves of a tree are 512 contiguous bytes
      if (pidx[k] >= 0) fqi_publish(vL + (size_t)pidx[k] * 64 + L, acc[k]);
    if (!fqi_meet(counter, (unsigned)(e + 1) * BLOCKS, &sh_ok))
    {
      if (threadIdx.x == 0) atomicOr(&rep.status, ST_SYNC_TIMEOUT);
      return;
    }
    FQI_STAMP(2);
    // level 3 and the step of ANNRepresentation::finalize (ann.cpp:198-221), in every block for all parameters
    // Four trees at a time, one per row of 16 lanes: lane j of row t loads leaves j, j+32, j+16, j+48 of its tree and adds them as
    // levels 32 and 16 do -- (v[j] + v[j+32]) + (v[j+16] + v[j+48]) --, levels 8..1 are row shifts (DPP); lane 0 of the row holds the
    // sum and steps the parameter, whose eta / previous gradient live in LDS beside the network.
    const int rowi = lane >> 4, j16 = lane & 15;
#pragma unroll
    for (int g0 = 0; g0 < GROUPS; g0 += GB)
    {
      constexpr int GBmax = GB;
      double leaf[GBmax][4];
#pragma unroll
      for (int gg = 0; gg < GBmax; ++gg)
        if (g0 + gg < GROUPS)
        {
          const int p = w + WAVES * (4 * (g0 + gg) + rowi);
          const double *t = vL + (size_t)(p <= P ? p : P) * 64 + j16;
#pragma unroll
          for (int k = 0; k < 4; ++k) leaf[gg][k] = t[16 * k];
        }
      double st_eta[GBmax], st_prev[GBmax], st_net[GBmax];
#pragma unroll
      for (int gg = 0; gg < GBmax; ++gg)
        if (g0 + gg < GROUPS)
        {
          const int p = w + WAVES * (4 * (g0 + gg) + rowi), pc = p < P ? p : 0;
          st_eta[gg] = sh_eta[pc]; st_prev[gg] = sh_prev[pc]; st_net[gg] = sh_net[pc];
        }
#pragma unroll
      for (int gg = 0; gg < GBmax; ++gg)
        if (g0 + gg < GROUPS)
        {
          double v = (leaf[gg][0] + leaf[gg][2]) + (leaf[gg][1] + leaf[gg][3]);
          v += fqi_row_shl<8>(v);
          v += fqi_row_shl<4>(v);
          v += fqi_row_shl<2>(v);
          v += fqi_row_shl<1>(v);
          const int p = w + WAVES * (4 * (g0 + gg) + rowi);
          if (j16 == 0)
          {
            if (p == P) { last_error = v / (double)n; has_error = true; }
            else if (p < P)
            {
              const double Delta = 0. + v;                             // Delta was zero before this epoch (ann.cpp:221)
              if (F.eta == 0)
              { // RPROP (ann.cpp:207-213)
                const double eta = (Delta * st_prev[gg] > 0) ? st_eta[gg] * 1.2 : st_eta[gg] * 0.5;
                sh_net[p] = st_net[gg] - ((Delta > 0) ? eta : -eta);
                sh_eta[p] = eta;
                sh_prev[p] = Delta;
              }
              else if (F.eta > 0)
                sh_net[p] = st_net[gg] - (F.eta * Delta) / (double)n;   // gradient descent (:202-206), samples_ = n
              else
              { // RMSprop (:214-219); sqrt and the divisions are the correctly rounded IEEE operations
                const double gm = Delta / (double)n;
                const double eta = 0.9 * st_eta[gg] + 0.1 * (gm * gm);
                sh_eta[p] = eta;
                sh_net[p] = st_net[gg] + F.eta * (Delta / __builtin_sqrt(eta));
              }
            }
          }
        }
    }
    FQI_STAMP(3);
    __syncthreads();
    FQI_STAMP(4);
  }
#undef FQI_STAMP
  if (bl == 0)
  { // the blocks hold the same bits: one of them writes the state back for the kernels and launches that follow
    for (int k = (int)threadIdx.x; k < P; k += NT)
    {
      net[k] = sh_net[k];
      net[F.P + k] = sh_eta[k];
      net[3 * F.P + k] = sh_prev[k];
    }
    if (has_error) rep.last_error = last_error;
  }
}

// the test trial after a batch (batch_learning.cpp:141-186): agent/fixed + policy/discrete/q + sampler/greedy; one lane per replica
template <int H>
__global__ __launch_bounds__(64) void fqi_test_kernel(FqiParams F)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= F.R) return;
  FqiRep &rep = F.rep[r];
  const double *net = F.net + (size_t)r * 4 * F.P;
  uint64_t TL = rep.TL, G = rep.G;
  double x[kFqiS], obs[kFqiD], reward = 0, total = 0;
  int terminal = 0;
  uint32_t status = 0;
  Env<GRLX_ENV_PENDULUM>::start(F.env, 1, TL, G, x);
  Env<GRLX_ENV_PENDULUM>::observe(F.env, x, obs);
  for (int guard = 0; guard < GRLX_MAX_EPISODE_STEPS + 2; ++guard)
  {
    double q[kMaxActions];
    for (int k = 0; k < F.A; ++k)
    {
      double in[kFqiNIn];
      fqi_normalise(F, obs, F.actions[k], in);
      q[k] = ann_forward<H>(net, in, nullptr);
    }
    int mai = 0, man = 1;                                                    // GreedySampler::sample (greedy.cpp:47-86)
    for (int k = 1; k < F.A; ++k)
    {
      if (q[k] > q[mai]) { mai = k; man = 1; }
      else if (q[k] == q[mai]) man++;
    }
    if (man > 1)
    {
      G = lcg_next(G);
      int jj = (int)(lcg_long(G) % (uint32_t)man);
      for (int k = 0; k < F.A; ++k)
        if (q[k] == q[mai])
        {
          if (jj == 0) { mai = k; break; }
          --jj;
        }
    }
    if (terminal) break;
    env_step<GRLX_ENV_PENDULUM, false>(F.env, x, F.actions[mai], obs, reward, terminal, status);
    total += reward;
    if (terminal == 2) break;
  }
  if (rep.rows < (uint32_t)F.max_rows)
  {
    const size_t at = (size_t)r * (size_t)F.max_rows + rep.rows;
    F.row_reward[at] = total;
    F.row_batch[at] = rep.batches_done;
    F.row_transitions[at] = rep.batches_done * (int64_t)F.batch_size;
    rep.rows++;
  }
  else
    status |= ST_ROWS_FULL;
  rep.batches_done++;
  rep.TL = TL;
  rep.G = G;
  rep.status |= status;
}

// ------------------------------------------------------------------------------------------- policy query ---
// grlx_fqi_query: the batch path's Q(s, a_k) at observations of the caller's choice -- the projector's normalisation and the network's
// forward pass on the replica's CURRENT parameters, the operations of fqi_test_kernel's policy.  Reads F.net only: nothing of the
// context changes.

// one thread per (replica, observation), looping over the actions; q[(replica - first_replica) * n_obs + observation][F.A]
template <int H>
__global__ __launch_bounds__(64) void fqi_query_kernel(FqiParams F, int first_replica, int n_replicas, const double *obs, int n_obs, double *q)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_replicas * n_obs) return;
  const int rl = (int)(i / n_obs), o = (int)(i - (long long)rl * n_obs);
  const double *net = F.net + (size_t)(first_replica + rl) * 4 * F.P;
  double ob[kFqiD];
#pragma unroll
  for (int d = 0; d < kFqiD; ++d) ob[d] = obs[(size_t)o * kFqiD + d];
  for (int k = 0; k < F.A; ++k)
  {
    double in[kFqiNIn];
    fqi_normalise(F, ob, F.actions[k], in);
    q[(size_t)i * F.A + k] = ann_forward<H>(net, in, nullptr);
  }
}

// ----------------------------------------------------------------------------------- greedy evaluation episodes ---
// grlx_fqi_evaluate, grlx_fqi_evaluate_trajectory: for every (replica, start state) pair one greedy episode of the batch path's policy
// from a MODEL state of the caller's choice -- fqi_test_kernel's loop with the caller's state in place of Task::start and without the
// tie-breaking draw (the first maximum acts; `ties` counts the steps with more than one).  Reads F.net, F.env and the projector's
// constants only: no row, no batches_done, no stream, no status bit, no parameter changes.
//
// Layout.  The policy is A small dense forward passes per step, so ONE LANE is one pair; blockIdx.y is the replica, which makes the
// network block-uniform: its P = 5 H + 1 parameters (the first of the replica's four P-blocks in F.net) are staged once into LDS, as
// fqi_targets_kernel stages them, and handed to ann_forward<H> as they are (broadcast reads: every lane reads the same word).  blockIdx.x
// covers the start states 64 at a time.  After the staging barrier no lane talks to another.  The episode loop is wave-uniform: it runs
// while a ballot finds an active lane and the step counter is below max_steps; finished and dead lanes skip the step under a predicate.
// Nothing is indexed at run time by a lane's value: the action of pass k and the chosen action are selects over the A actions (an
// indexed read of F.actions, or of a local q[], would go to scratch), findmax runs on the Q-values as they are produced.
// The two observation inputs of a step are the same in its A passes: fqi_normalise forms them from the same operands by the same
// operations each time, so a compiler that forms them once changes no bit; ann_forward itself is not re-associated.
// RECORD: one record of GRLX_TRAJ_OBS + 2 + 3 doubles per step taken, and -- behind the lane's own episode's end -- zeros up to
// max_steps, written by the lane itself: the staging buffer is never filled twice.
template <int H, bool RECORD>
__global__ __launch_bounds__(64) void fqi_evaluate_kernel(FqiParams F, FqiEvalArgs A)
{
  constexpr int R = kFqiTrajWords;
  __shared__ double sh_net[(kFqiNIn + 1) * H + H + 1];
  const int rl = blockIdx.y, r = A.first_replica + rl;
  const double *net = F.net + (size_t)r * 4 * F.P;
  for (int k = threadIdx.x; k < F.P; k += blockDim.x) sh_net[k] = net[k];
  __syncthreads();
  const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const bool live = s < A.n_starts;                    // dead lanes of the last block neither load nor store
  const size_t pair = (size_t)rl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;      // 64-bit: pairs * max_steps * R * 8 bytes pass 2^32
  double x[kFqiS], obs[kFqiD];
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) x[i] = live ? A.states[(size_t)s * kFqiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(F.env, x, obs);                // the start state's terminal code is ignored

  double ret = 0, disc = 0, g = 1;
  int steps = 0, code = 0, ties = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active)
    {
      double best = 0, action = 0;
      int mai = 0, man = 1;                            // GreedySampler::findmax (greedy.cpp:47-61), as fqi_test_kernel runs it
      for (int k = 0; k < F.A; ++k)
      {
        double ak = F.actions[0];                      // k is uniform: scalar selects, no indexed read of the parameter block
#pragma unroll
        for (int a = 1; a < kMaxActions; ++a) ak = (k == a) ? F.actions[a] : ak;
        double in[kFqiNIn];
        fqi_normalise(F, obs, ak, in);
        const double q = ann_forward<H>(sh_net, in, nullptr);
        if (k == 0 || q > best) { best = q; action = ak; mai = k; man = 1; }
        else if (q == best) man++;
      }
      double before[kFqiD];
#pragma unroll
      for (int i = 0; i < kFqiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(F.env, x, action, obs, reward, terminal, status);
      ret += reward;
      disc += g * reward;
      g = g * F.gamma_tau;
      ties += man > 1 ? 1 : 0;
      code = (status & ST_DOMAIN) ? kFqiEvalDomain : terminal;
      active = code == 0;
      if constexpr (RECORD)
      {
        double *w = rec + (size_t)steps * R;
        w[GRLX_TRAJ_ACTION] = action;
        w[GRLX_TRAJ_REWARD] = reward;
        w[GRLX_TRAJ_VALUE] = best;
        w[GRLX_TRAJ_ACTION_INDEX] = (double)mai;
        w[GRLX_TRAJ_N_MAX] = (double)man;
        w[GRLX_TRAJ_TERMINAL] = (double)code;
#pragma unroll
        for (int i = 0; i < kFqiD; ++i) w[GRLX_TRAJ_OBS + i] = before[i];
#pragma unroll
        for (int i = 0; i < kFqiS; ++i) w[GRLX_TRAJ_OBS + kFqiD + i] = x[i];
      }
      steps++;
    }
  }
  if (!live) return;
  if constexpr (RECORD)
    for (size_t k = (size_t)steps * R; k < (size_t)A.max_steps * R; ++k) rec[k] = 0.;       // behind the episode's end: all-zero bits
  A.ret[pair] = ret;
  A.disc[pair] = disc;
  A.steps[pair] = steps;
  A.terminal[pair] = code;
  A.ties[pair] = ties;
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) A.final_state[pair * kFqiS + i] = x[i];
}

// ---------------------------------------------------------------------------- the ensemble over groups of replicas ---
// grlx_fqi_query_ensemble, grlx_fqi_evaluate_ensemble, grlx_fqi_evaluate_ensemble_trajectory: the replicas [first_replica, first_replica +
// n_replicas) in groups of group_size consecutive ones (bagged FQI: every replica is a network of its own fitted to transitions of its
// own).  Per observation the members are visited in ASCENDING replica order: q_m[k] by the operations of fqi_query_kernel, (mai_m, man_m)
// by findmax, votes[mai_m] += 1, sumq[k] += q_m[k] into one accumulator per action from 0.0 -- that order is the specification.  The
// episode is fqi_evaluate_kernel's with the first maximum of votes (GRLX_ENSEMBLE_VOTE) or sumq (GRLX_ENSEMBLE_MEAN_Q) acting.  Reads
// F.net, F.env and the projector's constants only.
//
// Layout of the episodes.  One lane is one (group, start state) pair, blockIdx.y the group, the block one wave: the member loop is
// block-uniform, and a lane walks its group's members one after the other.  A member's P = 5 H + 1 parameters (the first of the replica's
// four P-blocks in F.net) are read where ann_forward<H> uses them, through the member's block-uniform global address: no LDS, no barrier,
// no lane talks to another.  (Staging the members into LDS in rounds of 16 was measured against this and was never faster: DESIGN.md
// section 4.2i.)  The step loop is wave-uniform: it runs while a ballot finds an active lane; finished and dead lanes skip the step.
// Nothing is indexed at run time by a lane's value or by a loop counter that is not unrolled: the action of pass k, q[k] -> q[], the
// member's vote, the chosen action and its score are selects over the kMaxActions actions.  ann_forward is called as it is.
// one member at obs: q[k] = Q(obs, a_k) for k < F.A (the others stay 0), sumq[k] += q[k], and findmax over them (greedy.cpp:47-61) as
// they are produced.  A caller that does not read q[] pays nothing for it.
template <int H>
__device__ __forceinline__ void fqi_member_values(const FqiParams &F, const double *w, const double *obs, double (&q)[kMaxActions],
                                                  double (&sumq)[kMaxActions], double &best, int &mai, int &man)
{
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a) q[a] = 0;
  best = 0; mai = 0; man = 1;
  for (int k = 0; k < F.A; ++k)
  {
    double ak = F.actions[0];                          // k is uniform: scalar selects, no indexed read of the parameter block
#pragma unroll
    for (int a = 1; a < kMaxActions; ++a) ak = (k == a) ? F.actions[a] : ak;
    double in[kFqiNIn];
    fqi_normalise(F, obs, ak, in);
    const double qk = ann_forward<H>(w, in, nullptr);
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
    {
      q[a] = (k == a) ? qk : q[a];
      sumq[a] = (k == a) ? sumq[a] + qk : sumq[a];
    }
    if (k == 0 || qk > best) { best = qk; mai = k; man = 1; }
    else if (qk == best) man++;
  }
}

template <int H, bool RECORD>
__global__ __launch_bounds__(64) void fqi_evaluate_ensemble_kernel(FqiParams F, FqiEnsArgs A)
{
  constexpr int R = kFqiEnsTrajWords;
  const int gl = blockIdx.y, G = A.group_size;
  const double *nets = F.net + (size_t)(A.first_replica + gl * G) * 4 * F.P;       // member m: nets + m * 4 * F.P, its first P-block
  const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const bool live = s < A.n_starts;                    // dead lanes of the last block neither load nor store
  const size_t pair = (size_t)gl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;      // 64-bit: pairs * max_steps * R * 8 bytes pass 2^32
  double x[kFqiS], obs[kFqiD];
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) x[i] = live ? A.states[(size_t)s * kFqiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(F.env, x, obs);                // the start state's terminal code is ignored

  double ret = 0, disc = 0, g = 1;
  int steps = 0, code = 0, ties = 0;
  long long member_ties = 0, agreement = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    int votes[kMaxActions], mties = 0;
    double sumq[kMaxActions];
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a) { votes[a] = 0; sumq[a] = 0.; }
    if (active)
      for (int m = 0; m < G; ++m)
      {
        double q[kMaxActions], best;
        int mai, man;
        fqi_member_values<H>(F, nets + (size_t)m * 4 * F.P, obs, q, sumq, best, mai, man);
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a) votes[a] += (mai == a) ? 1 : 0;
        mties += man > 1 ? 1 : 0;
      }
    if (active)
    {
      const bool vote = A.rule == GRLX_ENSEMBLE_VOTE;
      double best = vote ? (double)votes[0] : sumq[0], action = F.actions[0];
      int mai = 0, man = 1, agree = votes[0];          // findmax over the combined score; the first maximum acts, no draw
#pragma unroll
      for (int a = 1; a < kMaxActions; ++a)
        if (a < F.A)
        {
          const double sc = vote ? (double)votes[a] : sumq[a];
          if (sc > best) { best = sc; action = F.actions[a]; mai = a; man = 1; agree = votes[a]; }
          else if (sc == best) man++;
        }
      double before[kFqiD];
#pragma unroll
      for (int i = 0; i < kFqiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(F.env, x, action, obs, reward, terminal, status);
      ret += reward;
      disc += g * reward;
      g = g * F.gamma_tau;
      ties += man > 1 ? 1 : 0;
      member_ties += mties;
      agreement += agree;
      code = (status & ST_DOMAIN) ? kFqiEvalDomain : terminal;
      active = code == 0;
      if constexpr (RECORD)
      {
        double *w = rec + (size_t)steps * R;
        w[GRLX_TRAJ_ACTION] = action;
        w[GRLX_TRAJ_REWARD] = reward;
        w[GRLX_TRAJ_VALUE] = best;
        w[GRLX_TRAJ_ACTION_INDEX] = (double)mai;
        w[GRLX_TRAJ_N_MAX] = (double)man;
        w[GRLX_TRAJ_TERMINAL] = (double)code;
        w[GRLX_TRAJ_ENS_AGREEMENT] = (double)agree;
        w[GRLX_TRAJ_ENS_MEMBER_TIES] = (double)mties;
#pragma unroll
        for (int i = 0; i < kFqiD; ++i) w[GRLX_TRAJ_ENS_OBS + i] = before[i];
#pragma unroll
        for (int i = 0; i < kFqiS; ++i) w[GRLX_TRAJ_ENS_OBS + kFqiD + i] = x[i];
      }
      steps++;
    }
  }
  if (!live) return;
  if constexpr (RECORD)
    for (size_t k = (size_t)steps * R; k < (size_t)A.max_steps * R; ++k) rec[k] = 0.;       // behind the episode's end: all-zero bits
  A.ret[pair] = ret;
  A.disc[pair] = disc;
  A.steps[pair] = steps;
  A.terminal[pair] = code;
  A.ties[pair] = ties;
  A.member_ties[pair] = member_ties;
  A.agreement[pair] = agreement;
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) A.final_state[pair * kFqiS + i] = x[i];
}

// one lane per (group, observation), blockIdx.y the group: grlx_query_ensemble's columns, every sum over the members in ascending order
// into one accumulator.  out[group][n_obs][2 + 2 F.A].  The members are read as the evaluation reads them.
template <int H>
__global__ __launch_bounds__(64) void fqi_query_ensemble_kernel(FqiParams F, int first_replica, int group_size, const double *obs, int n_obs, double *out)
{
  const int o = (int)blockIdx.x * 64 + (int)threadIdx.x, gl = blockIdx.y;
  if (o >= n_obs) return;
  const double *nets = F.net + (size_t)(first_replica + gl * group_size) * 4 * F.P;
  double ob[kFqiD];
#pragma unroll
  for (int d = 0; d < kFqiD; ++d) ob[d] = obs[(size_t)o * kFqiD + d];
  double sv = 0, svv = 0, sumq[kMaxActions], votes[kMaxActions];
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a) { sumq[a] = 0.; votes[a] = 0.; }
  for (int m = 0; m < group_size; ++m)
  {
    double q[kMaxActions], best;
    int mai, man;
    fqi_member_values<H>(F, nets + (size_t)m * 4 * F.P, ob, q, sumq, best, mai, man);
    double v = 0;                                       // q.cpp:56-68 over greedy.cpp:88-98, as grlx_query_q forms it
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
      if (a < F.A) v += q[a] * (q[a] == best ? 1. / man : 0.);
    sv += v;
    svv += v * v;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a) votes[a] += (mai == a) ? 1. : 0.;
  }
  double *row = out + ((size_t)gl * (size_t)n_obs + (size_t)o) * (size_t)(2 + 2 * F.A);
  row[0] = sv;
  row[1] = svv;
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a)
    if (a < F.A)
    {
      row[2 + a] = sumq[a];
      row[2 + F.A + a] = votes[a];
    }
}

// ------------------------------------------------------------------------------------------ sampled episodes ---
// grlx_fqi_evaluate_sampled, grlx_fqi_evaluate_sampled_trajectory: fqi_evaluate_kernel's episode -- its layout, its staging of the network,
// its wave-uniform loop -- acted by the reference's samplers on two rand48 words the lane carries: S, the sampler's stream (the epsilon
// draw), and G, the global stream (the random action index, the tie break).  The order of draws is fqi_test_kernel's and
// grlx_evaluate_sampled.hip's: S first, then G for the random action or, on a step that does not explore, for the tie break.  The Q-values of
// a step are kept (selects over kMaxActions, no run-time index: see above) because the (jj + 1)-th maximum and Q of the action taken are read
// after the last pass.  A kernel of its own and no shared body: fqi_evaluate_kernel keeps its instruction stream.
template <int H, bool RECORD>
__global__ __launch_bounds__(64) void fqi_evaluate_sampled_kernel(FqiParams F, FqiSampledArgs T)
{
  constexpr int R = kFqiSampledTrajWords;
  __shared__ double sh_net[(kFqiNIn + 1) * H + H + 1];
  const FqiEvalArgs &A = T.e;
  const int rl = blockIdx.y, r = A.first_replica + rl;
  const double *net = F.net + (size_t)r * 4 * F.P;
  for (int k = threadIdx.x; k < F.P; k += blockDim.x) sh_net[k] = net[k];
  __syncthreads();
  const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const bool live = s < A.n_starts;                    // dead lanes of the last block neither load nor store nor draw
  const size_t pair = (size_t)rl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kFqiS], obs[kFqiD];
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) x[i] = live ? A.states[(size_t)s * kFqiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(F.env, x, obs);                // the start state's terminal code is ignored
  uint64_t S = 0, G = 0;
  if (live)
  {
    S = T.streams ? T.streams[pair * 2] : 0ull;
    G = T.streams ? T.streams[pair * 2 + 1] : F.rep[r].G;              // a copy: the replica's own stream does not move
  }

  double ret = 0, disc = 0, g = 1;
  int steps = 0, code = 0, ties = 0, explored = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    if (active)
    { // the draws sit under the step's predicate: a finished lane's streams stand where its last step left them
      double q[kMaxActions], best = 0;
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a) q[a] = 0;
      int mai = 0, man = 1;                            // GreedySampler::findmax (greedy.cpp:47-61)
      for (int k = 0; k < F.A; ++k)
      {
        double ak = F.actions[0];
#pragma unroll
        for (int a = 1; a < kMaxActions; ++a) ak = (k == a) ? F.actions[a] : ak;
        double in[kFqiNIn];
        fqi_normalise(F, obs, ak, in);
        const double qk = ann_forward<H>(sh_net, in, nullptr);
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a) q[a] = (k == a) ? qk : q[a];
        if (k == 0 || qk > best) { best = qk; mai = k; man = 1; }
        else if (qk == best) man++;
      }
      int idx = mai;
      bool tie = false, random = false;
      if (T.sampler == GRLX_SAMPLER_EPSILON_GREEDY)
      { // EpsilonGreedySampler::sample (greedy.cpp:144-218)
        S = lcg_next(S);
        if (lcg_double(S) < T.epsilon)
        {
          G = lcg_next(G);
          idx = (int)(lcg_long(G) % (uint32_t)F.A);
          random = true;
        }
      }
      if (!random && man > 1)
      { // greedy.cpp:77-85 by selects: the entry at which the countdown over the maximal entries stands at zero
        G = lcg_next(G);
        int jj = (int)(lcg_long(G) % (uint32_t)man);
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a)
        {
          const bool m = a < F.A && q[a] == best;
          idx = (m && jj == 0) ? a : idx;
          jj -= m ? 1 : 0;
        }
        tie = true;
      }
      double action = 0, value = 0;
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
      {
        action = (idx == a) ? F.actions[a] : action;
        value = (idx == a) ? q[a] : value;
      }
      double before[kFqiD];
#pragma unroll
      for (int i = 0; i < kFqiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(F.env, x, action, obs, reward, terminal, status);
      ret += reward;
      disc += g * reward;
      g = g * F.gamma_tau;
      ties += tie ? 1 : 0;
      explored += random ? 1 : 0;
      code = (status & ST_DOMAIN) ? kFqiEvalDomain : terminal;
      active = code == 0;
      if constexpr (RECORD)
      {
        double *w = rec + (size_t)steps * R;
        w[GRLX_TRAJ_ACTION] = action;
        w[GRLX_TRAJ_REWARD] = reward;
        w[GRLX_TRAJ_VALUE] = value;
        w[GRLX_TRAJ_ACTION_INDEX] = (double)idx;
        w[GRLX_TRAJ_N_MAX] = (double)man;
        w[GRLX_TRAJ_TERMINAL] = (double)code;
#pragma unroll
        for (int i = 0; i < kFqiD; ++i) w[GRLX_TRAJ_OBS + i] = before[i];
#pragma unroll
        for (int i = 0; i < kFqiS; ++i) w[GRLX_TRAJ_OBS + kFqiD + i] = x[i];
        w[R - 1] = random ? 1.0 : 0.0;
      }
      steps++;
    }
  }
  if (!live) return;
  if constexpr (RECORD)
    for (size_t k = (size_t)steps * R; k < (size_t)A.max_steps * R; ++k) rec[k] = 0.;       // behind the episode's end: all-zero bits
  A.ret[pair] = ret;
  A.disc[pair] = disc;
  A.steps[pair] = steps;
  A.terminal[pair] = code;
  A.ties[pair] = ties;
  T.explored[pair] = explored;
  T.streams_out[pair * 2] = S;
  T.streams_out[pair * 2 + 1] = G;
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) A.final_state[pair * kFqiS + i] = x[i];
}

// grlx_fqi_evaluate_ensemble_sampled, grlx_fqi_evaluate_ensemble_sampled_trajectory: fqi_evaluate_ensemble_kernel's episodes with the action
// DRAWN from softmax(score / tau), the score being the members' votes (GRLX_ENSEMBLE_MAJORITY) or their summed ranks (GRLX_ENSEMBLE_RANK);
// include/grlx.h states the step (grlx_evaluate_ensemble_sampled).  Every score is an integer, so the members may be summed in any order,
// and that is what the layout is built on: the members of a group work side by side.
//
// Layout.  A ROW of 16 lanes is one (group, start state) pair; a wave holds four pairs of one group (blockIdx.y), blockIdx.x covers the start
// states four at a time, the block is one wave.  Lane j of a row serves the members j, j + 16, j + 32, ... of its group: a step costs
// ceil(G / 16) members' forward passes, where fqi_evaluate_ensemble_kernel's lane walks all G.  Per member the lane computes the A
// Q-values (fqi_member_values, as it is), the member's distribution, its vote and its ranks, and adds them to int accumulators of its own;
// a lane whose member index is >= G skips the member and adds nothing.  Then ONE all-reduce over the row: four DPP row rotations (8, 4, 2,
// 1) and adds per word, A vote words, A rank words under RANK, one word for the members with a tie -- no LDS, no barrier; after it every
// lane of the row holds the same totals.  Every lane of a row also holds the same model state and the same stream word, so all 16 run the
// combined softmax, the draw and env_step themselves, on identical bits: nothing is broadcast.  Lane 0 of the row writes the record, the
// outputs and the zeros behind the episode's end.  The step loop is wave-uniform (a ballot over the rows' `active`); a row is active or
// not as a whole, so the row rotations never cross a predicate's edge.
//
// Member parameters.  The lanes of a row read 16 DIFFERENT networks, so the block-uniform address of fqi_evaluate_ensemble_kernel is gone:
// each lane reads its member through its own global address (the four rows of a wave read the same 16 members).  Staging a round of 16
// members in LDS at an odd stride of P = 5 H + 1 doubles was measured against this: 5 % shorter calls for groups of exactly 16 at hidden =
// 20, up to 80 % longer ones for groups of 4 and of 64 (41 KB of LDS per wave at hidden = 64; a restaging per round and step beyond 16
// members), so it is not kept: DESIGN.md section 4.2o.
template <int N>
__device__ __forceinline__ int fqi_row_ror(int v)
{ // lane i of a row of 16 receives the value of lane (i - N) mod 16 of the same row (DPP row_ror: N)
  return __builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xF, 0xF, false);
}
__device__ __forceinline__ int fqi_row_sum(int v)
{ // the sum over the row's 16 lanes, in every one of them
  v += fqi_row_ror<8>(v);
  v += fqi_row_ror<4>(v);
  v += fqi_row_ror<2>(v);
  v += fqi_row_ror<1>(v);
  return v;
}

// (the distributions: batch_softmax, grlx_softmax.h)
template <int H, bool RECORD>
__global__ __launch_bounds__(64) void fqi_ensemble_sampled_kernel(FqiParams F, FqiEnsSampledArgs T)
{
  constexpr int R = kFqiEnsSampledTrajWords;
  const FqiEnsArgs &A = T.e;
  const int gl = blockIdx.y, G = A.group_size, NA = F.A;
  const int lane = threadIdx.x, row = lane >> 4, j = lane & 15;
  const bool rank = A.rule == GRLX_ENSEMBLE_RANK;
  const int r0 = A.first_replica + gl * G;
  const double *nets = F.net + (size_t)r0 * 4 * F.P;                   // member m: nets + m * 4 * F.P, its first P-block
  const int s = (int)blockIdx.x * 4 + row;
  const bool live = s < A.n_starts;                    // dead rows of the last block neither load nor store nor draw
  const size_t pair = (size_t)gl * (size_t)A.n_starts + (size_t)(live ? s : 0);
  double *rec = RECORD ? A.records + pair * (size_t)A.max_steps * R : nullptr;
  double x[kFqiS], obs[kFqiD];
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) x[i] = live ? A.states[(size_t)s * kFqiS + i] : 0.;
  (void)Env<GRLX_ENV_PENDULUM>::observe(F.env, x, obs);                // the start state's terminal code is ignored
  uint64_t rng = 0;
  if (live) rng = T.streams ? T.streams[pair] : F.rep[r0].G;           // a copy: the replica's own stream does not move

  double ret = 0, disc = 0, g = 1;
  int steps = 0, code = 0, ties = 0, explored = 0;
  long long member_ties = 0, agreement = 0;
  bool active = live;
  for (int step = 0; step < A.max_steps; ++step)
  {
    if (__ballot(active) == 0ull) break;               // wave-uniform
    int votes[kMaxActions], ranks[kMaxActions], mties = 0;
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a) { votes[a] = 0; ranks[a] = 0; }
    for (int m0 = 0; m0 < G; m0 += 16)
    {
      const int m = m0 + j;
      if (active && m < G)
      {
        const double *w = nets + (size_t)m * 4 * F.P;
        double q[kMaxActions], unused[kMaxActions], d[kMaxActions], best;
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a) unused[a] = 0.;
        int mai, man;
        fqi_member_values<H>(F, w, obs, q, unused, best, mai, man);
        if (T.member == GRLX_MEMBER_SOFTMAX) batch_softmax(q, NA, T.member_param, d);
        else
        { // greedy.cpp:88-98, and :229-236 for the epsilon-greedy member
#pragma unroll
          for (int a = 0; a < kMaxActions; ++a)
          {
            d[a] = (a < NA && q[a] == best) ? 1. / (double)man : 0.;
            if (T.member == GRLX_MEMBER_EPSILON)
            {
              d[a] = (d[a] == 1) ? 1 - T.member_param : d[a];
              d[a] += T.member_param / (double)NA;
            }
          }
        }
        // the member's vote (multi_discrete.cpp:218-229): the first entry above every entry before it and above 0.0; NA - 1 without one
        double top = 0.0;
        int vote = NA - 1;
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a)
        {
          const bool up = a < NA && d[a] > top;
          vote = up ? a : vote;
          top = up ? d[a] : top;
        }
#pragma unroll
        for (int a = 0; a < kMaxActions; ++a) votes[a] += (vote == a) ? 1 : 0;
        mties += man > 1 ? 1 : 0;
        if (rank)
        { // the rank of action a among the member's entries: 1 + the entries strictly below it (:237-281)
#pragma unroll
          for (int a = 0; a < kMaxActions; ++a)
          {
            int below = 1;
#pragma unroll
            for (int k = 0; k < kMaxActions; ++k) below += (k < NA && d[a] > d[k]) ? 1 : 0;
            ranks[a] += (a < NA) ? below : 0;
          }
        }
      }
    }
    // the row's totals, in every lane of the row: integer adds, exact in any order
#pragma unroll
    for (int a = 0; a < kMaxActions; ++a)
      if (a < NA)
      {
        votes[a] = fqi_row_sum(votes[a]);
        if (rank) ranks[a] = fqi_row_sum(ranks[a]);
      }
    mties = fqi_row_sum(mties);
    if (active)
    {
      double sc[kMaxActions], dist[kMaxActions];
      int score[kMaxActions];
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
      {
        score[a] = rank ? ranks[a] : votes[a];
        sc[a] = (double)score[a];
      }
      batch_softmax(sc, NA, T.tau, dist);
      // grl::sample (utils.h:227-250) on one drand48 of the episode's stream
      double sum = 0;
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
        if (a < NA) sum += dist[a];
      rng = lcg_next(rng);
      const double u = lcg_double(rng) * sum;
      double acc = 0;
      int idx = NA - 1;
      bool found = false;
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
        if (a < NA)
        {
          acc += dist[a];
          const bool here = !found && u < acc;
          idx = here ? a : idx;
          found = found || here;
        }
      int mai = 0, man = 1, top = score[0];            // findmax over the score
#pragma unroll
      for (int a = 1; a < kMaxActions; ++a)
        if (a < NA)
        {
          if (score[a] > top) { top = score[a]; mai = a; man = 1; }
          else if (score[a] == top) man++;
        }
      double action = 0, value = 0, prob = 0;
      int agree = 0;
#pragma unroll
      for (int a = 0; a < kMaxActions; ++a)
      {
        action = (idx == a) ? F.actions[a] : action;
        value = (idx == a) ? sc[a] : value;
        prob = (idx == a) ? dist[a] : prob;
        agree = (idx == a) ? votes[a] : agree;
      }
      const bool off = idx != mai;
      double before[kFqiD];
#pragma unroll
      for (int i = 0; i < kFqiD; ++i) before[i] = obs[i];
      double reward = 0;
      int terminal = 0;
      uint32_t status = 0;
      env_step<GRLX_ENV_PENDULUM, false>(F.env, x, action, obs, reward, terminal, status);
      ret += reward;
      disc += g * reward;
      g = g * F.gamma_tau;
      ties += man > 1 ? 1 : 0;
      member_ties += mties;
      agreement += agree;
      explored += off ? 1 : 0;
      code = (status & ST_DOMAIN) ? kFqiEvalDomain : terminal;
      active = code == 0;
      if constexpr (RECORD)
        if (j == 0)
        {
          double *w = rec + (size_t)steps * R;
          w[GRLX_TRAJ_ACTION] = action;
          w[GRLX_TRAJ_REWARD] = reward;
          w[GRLX_TRAJ_VALUE] = value;
          w[GRLX_TRAJ_ACTION_INDEX] = (double)idx;
          w[GRLX_TRAJ_N_MAX] = (double)man;
          w[GRLX_TRAJ_TERMINAL] = (double)code;
          w[GRLX_TRAJ_ENS_AGREEMENT] = (double)agree;
          w[GRLX_TRAJ_ENS_MEMBER_TIES] = (double)mties;
#pragma unroll
          for (int i = 0; i < kFqiD; ++i) w[GRLX_TRAJ_ENS_OBS + i] = before[i];
#pragma unroll
          for (int i = 0; i < kFqiS; ++i) w[GRLX_TRAJ_ENS_OBS + kFqiD + i] = x[i];
          w[R - 2] = off ? 1.0 : 0.0;
          w[R - 1] = prob;
        }
      steps++;
    }
  }
  if (!live || j != 0) return;
  if constexpr (RECORD)
    for (size_t k = (size_t)steps * R; k < (size_t)A.max_steps * R; ++k) rec[k] = 0.;       // behind the episode's end: all-zero bits
  A.ret[pair] = ret;
  A.disc[pair] = disc;
  A.steps[pair] = steps;
  A.terminal[pair] = code;
  A.ties[pair] = ties;
  A.member_ties[pair] = member_ties;
  A.agreement[pair] = agreement;
  T.explored[pair] = explored;
  T.streams_out[pair] = rng;
#pragma unroll
  for (int i = 0; i < kFqiS; ++i) A.final_state[pair * kFqiS + i] = x[i];
}

// ------------------------------------------------------------------------------------------------ host launchers ---
// What grlx_api_fqi.cpp needs from the kernel symbols above (grlx_fqi.h).  Host code does not live in this unit beyond this block, and
// kernels are appended above it, not inserted: every kernel keeps its instruction stream.

// the instantiated widths of the hidden layer (representation/parameterized/ann:hiddens = [H])
#define FQI_FOR_H(H_, ...)                                           \
  switch (H_)                                                        \
  {                                                                  \
    case 8:  { constexpr int HH = 8;  __VA_ARGS__; } break;          \
    case 16: { constexpr int HH = 16; __VA_ARGS__; } break;          \
    case 20: { constexpr int HH = 20; __VA_ARGS__; } break;          \
    case 32: { constexpr int HH = 32; __VA_ARGS__; } break;          \
    case 64: { constexpr int HH = 64; __VA_ARGS__; } break;          \
    default: return hipErrorInvalidValue;                            \
  }
bool fqi_width_built(int H) { return H == 8 || H == 16 || H == 20 || H == 32 || H == 64; }

hipError_t fqi_epochs_shape(int H, FqiLaunchPlan *plan, int *blocks_per_cu)
{
  FQI_FOR_H(H, plan->blocks_per_replica = FqiShape<HH>::BLOCKS; plan->block_threads = FqiShape<HH>::WAVES * 64;
            return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fqi_epochs_kernel<HH>, FqiShape<HH>::WAVES * 64, 0));
  return hipErrorInvalidValue;
}

hipError_t launch_fqi_init(const FqiParams &F, const uint64_t *r0, hipStream_t stream)
{
  hipLaunchKernelGGL(fqi_init_kernel, dim3((F.P + 127) / 128, F.R), dim3(128), 0, stream, F, r0);
  return hipGetLastError();
}

hipError_t launch_fqi_batch(const FqiParams &F, FqiLaunchPlan &plan, int batches_run, int iterations, int epochs_, hipStream_t stream)
{
  const int n_after = (batches_run + 1) * F.batch_size;
  const int chunks = (n_after + 255) / 256;
  hipLaunchKernelGGL(fqi_generate_kernel, dim3((F.batch_size + 255) / 256, F.R), dim3(256), 0, stream, F);
  hipLaunchKernelGGL(fqi_batch_begin_kernel, dim3((F.R + 63) / 64), dim3(64), 0, stream, F);
  for (int ii = 0; ii < iterations; ++ii)
  {
    hipLaunchKernelGGL(fqi_iter_begin_kernel, dim3((F.R + 63) / 64), dim3(64), 0, stream, F, ii);
    FQI_FOR_H(F.H, hipLaunchKernelGGL(fqi_targets_kernel<HH>, dim3(chunks, F.R), dim3(256), 0, stream, F, ii == 0 ? 1 : 0));
    // the epochs of the iteration: one cooperative launch per group of replicas that fills the chip (16 blocks per replica for [20])
    for (int r0 = 0; r0 < F.R; r0 += plan.replicas_per_launch)
    {
      const int nr = (F.R - r0 < plan.replicas_per_launch) ? F.R - r0 : plan.replicas_per_launch;
      if (hipError_t e = hipMemsetAsync(F.sync + (size_t)r0 * 4, 0, (size_t)nr * 4 * sizeof(unsigned int), stream)) return e;
      FqiParams Fa = F;
      int r_first = r0, epochs = epochs_;
      void *args[] = {&Fa, &r_first, &epochs};
      const dim3 grid(nr * plan.blocks_per_replica), block(plan.block_threads);
      hipError_t le = hipSuccess;
      if (!plan.plain_launch)
      {
        FQI_FOR_H(F.H, le = hipLaunchCooperativeKernel((const void *)fqi_epochs_kernel<HH>, grid, block, args, 0, stream));
        // A device may lend its queue for cooperative launches to one process at a time: while another process holds it (a parent
        // that ran the batch path, the other rank on a shared GPU) the runtime answers hipErrorIllegalState and has launched nothing.
        // The kernel needs nothing of that queue but the residency check, and create() sized the grid to be resident
        // (replicas_per_launch); the spins are bounded either way.  So this context launches the same grid plainly from here on.
        if (le == hipErrorIllegalState)
        {
          (void)hipGetLastError();
          plan.plain_launch = true;
          le = hipSuccess;
        }
      }
      if (plan.plain_launch)      // also GRLX_FQI_NO_COOP=1 (diagnostic): the same grid without the runtime's residency check
      { FQI_FOR_H(F.H, hipLaunchKernelGGL(fqi_epochs_kernel<HH>, grid, block, 0, stream, Fa, r_first, epochs)); }
      if (le != hipSuccess) return le;
    }
  }
  FQI_FOR_H(F.H, hipLaunchKernelGGL(fqi_test_kernel<HH>, dim3((F.R + 63) / 64), dim3(64), 0, stream, F));
  return hipGetLastError();
}

hipError_t launch_fqi_query(const FqiParams &F, int first_replica, int n_replicas, const double *obs, int n_obs, double *q, hipStream_t stream)
{
  const long long pairs = (long long)n_replicas * n_obs;
  FQI_FOR_H(F.H, hipLaunchKernelGGL(fqi_query_kernel<HH>, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, stream, F, first_replica, n_replicas, obs,
                                    n_obs, q));
  return hipGetLastError();
}

hipError_t launch_fqi_evaluate(const FqiParams &F, const FqiEvalArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.n_starts + 63) / 64), (unsigned)rows), block(64);
  if (A.records) { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_kernel<HH, true>), grid, block, 0, stream, F, A)); }
  else { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_kernel<HH, false>), grid, block, 0, stream, F, A)); }
  return hipGetLastError();
}

hipError_t launch_fqi_evaluate_ensemble(const FqiParams &F, const FqiEnsArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.n_starts + 63) / 64), (unsigned)rows), block(64);
  if (A.records) { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_ensemble_kernel<HH, true>), grid, block, 0, stream, F, A)); }
  else { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_ensemble_kernel<HH, false>), grid, block, 0, stream, F, A)); }
  return hipGetLastError();
}

hipError_t launch_fqi_evaluate_sampled(const FqiParams &F, const FqiSampledArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.e.n_starts + 63) / 64), (unsigned)rows), block(64);
  if (A.e.records) { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_sampled_kernel<HH, true>), grid, block, 0, stream, F, A)); }
  else { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_evaluate_sampled_kernel<HH, false>), grid, block, 0, stream, F, A)); }
  return hipGetLastError();
}

// one wave per block, four (group, start state) pairs per wave
hipError_t launch_fqi_evaluate_ensemble_sampled(const FqiParams &F, const FqiEnsSampledArgs &A, int rows, hipStream_t stream)
{
  const dim3 grid((unsigned)((A.e.n_starts + 3) / 4), (unsigned)rows), block(64);
  if (A.e.records) { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_ensemble_sampled_kernel<HH, true>), grid, block, 0, stream, F, A)); }
  else { FQI_FOR_H(F.H, hipLaunchKernelGGL((fqi_ensemble_sampled_kernel<HH, false>), grid, block, 0, stream, F, A)); }
  return hipGetLastError();
}

hipError_t launch_fqi_query_ensemble(const FqiParams &F, int first_replica, int groups, int group_size, const double *obs, int n_obs, double *out,
                                     hipStream_t stream)
{
  const dim3 grid((unsigned)((n_obs + 63) / 64), (unsigned)groups), block(64);
  FQI_FOR_H(F.H, hipLaunchKernelGGL(fqi_query_ensemble_kernel<HH>, grid, block, 0, stream, F, first_replica, group_size, obs, n_obs, out));
  return hipGetLastError();
}

} // namespace grlx
