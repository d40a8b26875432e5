// grlx_lspi.hip -- least-squares policy iteration on the batch path: experiment/batch_learning + predictor/lspi +
// representation/parameterized/linear over projector/rbf/{triangle, gauss}, R independent-seed replicas per GPU.  Reference:
// batch_learning.cpp:88-205, lspi.cpp:110-206, rbf.cpp:99-211, linear.cpp:136-180.  The specification S1-S10 and the deviations D1-D7
// are at the top of grlx_lspi.h; this file restates them for the GPU.
//
// Shape of the work.  A rebuild is A_s = 1e-5 I + Phi^T Phi and b = Phi^T r once, then `iterations` x (greedy choice per transition,
// Phi^T Psi, one dense F x F solve).  With F = 363 and 100,000 transitions the products are M = N = 363, K = 100,000 in f64: they run on
// v_mfma_f64_16x16x4_f64.  Phi and Psi never exist in memory: a block projects 16 transitions at a time into LDS as dense zero-padded
// rows and feeds the matrix instruction's operands from there.  K is split over blocks; the partial tiles are added by a second kernel
// in ascending chunk order, so there is no floating-point atomic and the bytes do not depend on the schedule.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_lspi.h"
#include "grlx_lspi_read.h"

namespace grlx {

typedef double lspi_acc_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------ projection and read ---
// lspi_triangle, lspi_gauss, lspi_gauss_base and lspi_read: grlx_lspi_read.h, shared with the evaluation episodes (grlx_lspi_evaluate.hip)

// the first maximum of the reads over the actions (lspi.cpp:184-195: v > bestv from -infinity); man: how many equal it
__device__ __forceinline__ int lspi_greedy(const LspiParams &L, const double *w, const double *obs, int *man)
{
  double bestv = -__builtin_inf();
  int besta = 0, n = 0;
  for (int k = 0; k < L.A; ++k)
  {
    const double in[kLspiNIn] = {obs[0], obs[1], L.actions[k]};
    const double v = lspi_read(L, w, in);
    if (v > bestv) { bestv = v; besta = k; n = 1; }
    else if (v == bestv) n++;
  }
  if (man) *man = n;
  return besta;
}

// ------------------------------------------------------------------------------------------ init, sampling ---
__global__ void lspi_init_kernel(LspiParams L, const uint64_t *r0)
{
  const int r = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= L.Fp) return;
  double *w = L.w + (size_t)r * 2 * L.Fp;
  const uint64_t x = lcg_next(lcg_jump(r0[r], (uint64_t)k));
  w[k] = k < L.F ? L.init_min + lcg_double(x) * L.init_range : 0.;
  w[L.Fp + k] = w[k];
}

// BatchLearningExperiment::run, the sampling loop (batch_learning.cpp:107-138): fqi_generate_kernel's draws, the store raw (S1)
__global__ __launch_bounds__(256) void lspi_generate_kernel(LspiParams L)
{
  const int r = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= L.batch_size) return;
  const LspiRep &rep = L.rep[r];
  uint64_t x = lcg_jump(rep.TL, 4ull * (uint64_t)s);
  double obs[kLspiD];
#pragma unroll
  for (int i = 0; i < kLspiD; ++i) { x = lcg_next(x); obs[i] = 0 + lcg_double(x) * (1 - 0); }
  x = lcg_next(x);
  double action = 0 + lcg_double(x) * (1 - 0);
  // (the fourth draw is next_action: consumed, never read)
#pragma unroll
  for (int i = 0; i < kLspiD; ++i) obs[i] = L.obs_min[i] + obs[i] * L.obs_range[i];
  action = L.action_min + action * L.action_range;
  double st[kLspiS] = {obs[0] - GRLX_PI, obs[1], 0.};                         // PendulumSwingupTask::invert (pendulum.cpp:147-155)
  double nobs[kLspiD], reward;
  int terminal;
  uint32_t status = 0;
  env_step<GRLX_ENV_PENDULUM, false>(L.env, st, action, nobs, reward, terminal, status);
  const size_t at = (size_t)r * (size_t)L.cap + (size_t)rep.n + (size_t)s;
  L.in[at * kLspiNIn + 0] = obs[0];
  L.in[at * kLspiNIn + 1] = obs[1];
  L.in[at * kLspiNIn + 2] = action;
#pragma unroll
  for (int i = 0; i < kLspiD; ++i) L.next_obs[at * kLspiD + i] = nobs[i];
  L.reward[at] = reward;
  L.absorbing[at] = terminal == 2 ? 1 : 0;
  L.best[at] = 0;
  if (status) atomicOr(&L.rep[r].status, status);
}

__global__ void lspi_batch_begin_kernel(LspiParams L)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= L.R) return;
  LspiRep &rep = L.rep[r];
  rep.TL = lcg_jump(rep.TL, 4ull * (uint64_t)L.batch_size);
  rep.n += L.batch_size;
}

// ------------------------------------------------------------------------------------------ greedy choice ---
// one lane per transition: action_steps projections of the next observation and their reads on the current weights (S8)
__global__ __launch_bounds__(256) void lspi_greedy_kernel(LspiParams L, int n)
{
  const int r = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const size_t at = (size_t)r * (size_t)L.cap + (size_t)s;
  const double obs[kLspiD] = {L.next_obs[at * kLspiD], L.next_obs[at * kLspiD + 1]};
  L.best[at] = lspi_greedy(L, L.w + (size_t)r * 2 * L.Fp, obs, nullptr);
}

// ------------------------------------------------------------------------------------------ accumulation ---
// tile t of a pass's list -> (row tile, column tile).  Pass 0: row-major over the upper triangle, each row followed by its r-tile
// (column tile T); pass 1: row-major over the square.
template <int PASS>
__device__ __forceinline__ void lspi_tile_at(int T, int t, int &ti, int &tj)
{
  if (PASS == 0)
  {
    int i = 0, rem = t;
    while (i < T - 1 && rem >= T + 1 - i) { rem -= T + 1 - i; ++i; }
    ti = i;
    tj = i + rem;
  }
  else
  {
    ti = t / T;
    tj = t - ti * T;
  }
}

// C = X^T Y on v_mfma_f64_16x16x4_f64.  grid (tile groups, K chunks, replicas), 256 threads = 4 waves.
//
// LDS.  A slab is kLspiSlab = 16 rows (transitions) of `pitch` doubles: the features, zero padding up to Fp, and in pass 0 the reward in
// column Fp (the r-tile: b = Phi^T r falls out of the same instruction).  Pass 1 holds a second slab for Psi.  Per slab the block zeroes
// the rows, then 16 threads per transition scatter its projection (triangle: one pair each; gauss: features 16 apart), pruned as S6;
// rows past the chunk's end stay zero, so padding contributes exact zeros.
//
// Operands.  v_mfma_f64_16x16x4_f64 takes A[i][k] from lane i + 16 k and B[k][j] from lane j + 16 k.  With A = X^T both operands are
// read the same way: lane l reads row 4 kk + l / 16 of the slab, column 16 tile + l % 16 -- 16 consecutive doubles per K row.  The
// pitch is 16 (mod 32) doubles, so the two K rows a half-wave reads lie 32 banks apart: the operand reads are conflict-free.
// The accumulator's element v of lane l is C[4 v + l / 16][l % 16].
//
// A wave keeps kLspiTilesPerWave = 8 accumulator tiles (64 VGPRs) over its whole chunk and writes them once, lane-major, to
// partials[replica][chunk][tile][v][lane].
template <int PASS>
__global__ __launch_bounds__(256) void lspi_accumulate_kernel(LspiParams L, int n, int chunk)
{
  extern __shared__ double sh[];
  const int r = blockIdx.z, split = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = L.Fp / 16, pitch = lspi_pitch(L.Fp), NT = lspi_tiles(T, PASS);
  double *sx = sh, *sy = PASS == 0 ? sh : sh + kLspiSlab * pitch;
  const int slab_doubles = (PASS == 0 ? 1 : 2) * kLspiSlab * pitch;

  const int t0 = (blockIdx.x * 4 + wave) * kLspiTilesPerWave;
  int xo[kLspiTilesPerWave], yo[kLspiTilesPerWave];                            // the tiles' operand offsets inside a slab row
  lspi_acc_t acc[kLspiTilesPerWave];
#pragma unroll
  for (int u = 0; u < kLspiTilesPerWave; ++u)
  {
    int ti, tj;
    lspi_tile_at<PASS>(T, t0 + u < NT ? t0 + u : 0, ti, tj);
    xo[u] = (lane >> 4) * pitch + ti * 16 + (lane & 15);
    yo[u] = (lane >> 4) * pitch + tj * 16 + (lane & 15);
    acc[u] = (lspi_acc_t){0., 0., 0., 0.};
  }

  const size_t store = (size_t)r * (size_t)L.cap;
  const int begin = split * chunk, end = min(n, begin + chunk);
  const int row = tid >> 4, part = tid & 15;                                   // of the slab: transition, and which share of its projection
  for (int s0 = begin; s0 < end; s0 += kLspiSlab)
  {
    __syncthreads();                                                           // the previous slab's operand reads are done
    for (int i = tid; i < slab_doubles; i += 256) sh[i] = 0.;
    __syncthreads();
    const int s = s0 + row;
    if (s < end)
    {
      const size_t at = store + (size_t)s;
      const double in[kLspiNIn] = {L.in[at * kLspiNIn], L.in[at * kLspiNIn + 1], L.in[at * kLspiNIn + 2]};
      double nin[kLspiNIn] = {0., 0., 0.};
      bool has_next = false;
      if (PASS == 1)
      {
        has_next = !L.absorbing[at];
        nin[0] = L.next_obs[at * kLspiD];
        nin[1] = L.next_obs[at * kLspiD + 1];
        const int bk = L.best[at];
        double a = L.actions[0];
        for (int k = 1; k < L.A; ++k) a = (k == bk) ? L.actions[k] : a;
        nin[2] = a;
      }
      if (PASS == 0 && part == 8) sx[row * pitch + L.Fp] = L.reward[at];
      if (L.projector == GRLX_RBF_TRIANGLE)
      {
        if (part < 8 || (PASS == 1 && has_next))
        {
          int idx[8];
          double wt[8];
          if (part < 8) lspi_triangle(L, in, idx, wt); else lspi_triangle(L, nin, idx, wt);
          int id = idx[0];
          double w = wt[0];
#pragma unroll
          for (int ii = 1; ii < 8; ++ii)
            if ((part & 7) == ii) { id = idx[ii]; w = wt[ii]; }
          if (__builtin_fabs(w) > 0.00001)
          {
            if (part < 8) sx[row * pitch + id] = w;
            else sy[row * pitch + id] = L.gamma_tau * w;
          }
        }
      }
      else
      {
        double base[kLspiNIn], nbase[kLspiNIn];
        lspi_gauss_base(L, in, base);
        lspi_gauss_base(L, nin, nbase);
        const int s01 = L.steps[0] * L.steps[1];
        for (int f = part; f < L.F; f += 16)
        {
          const int k2 = f / s01, k1 = (f - k2 * s01) / L.steps[0], k0 = f - k2 * s01 - k1 * L.steps[0];
          const double g = lspi_gauss(L, base, k0, k1, k2);
          if (g > 0.00001) sx[row * pitch + f] = g;
          if (PASS == 1 && has_next)
          {
            const double h = lspi_gauss(L, nbase, k0, k1, k2);
            if (h > 0.00001) sy[row * pitch + f] = L.gamma_tau * h;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kLspiSlab / 4; ++kk)
#pragma unroll
      for (int u = 0; u < kLspiTilesPerWave; ++u)
        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(sx[kk * 4 * pitch + xo[u]], sy[kk * 4 * pitch + yo[u]], acc[u], 0, 0, 0);
  }

  double *part_out = L.partials + (size_t)r * L.partials_per_replica + (size_t)split * (size_t)NT * 256;
#pragma unroll
  for (int u = 0; u < kLspiTilesPerWave; ++u)
    if (t0 + u < NT)
    {
      double *p = part_out + (size_t)(t0 + u) * 256;
#pragma unroll
      for (int v = 0; v < 4; ++v) p[v * 64 + lane] = acc[u][v];
    }
}

// the chunks' partial tiles added in ascending chunk order; grid (tiles, replicas), thread = (v, lane) of the accumulator layout.
// Pass 0: A_s = 1e-5 I + sum, the tile mirrored below the diagonal, and b from column 0 of the r-tiles.  Pass 1: A = A_s - sum.
template <int PASS>
__global__ __launch_bounds__(256) void lspi_reduce_kernel(LspiParams L, int splits)
{
  const int t = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int T = L.Fp / 16, NT = lspi_tiles(T, PASS);
  int ti, tj;
  lspi_tile_at<PASS>(T, t, ti, tj);
  const double *p = L.partials + (size_t)r * L.partials_per_replica + (size_t)t * 256 + tid;
  double sum = 0;
  for (int s = 0; s < splits; ++s) sum += p[(size_t)s * (size_t)NT * 256];
  const int i = ti * 16 + 4 * v + (lane >> 4), j = tj * 16 + (lane & 15);
  const size_t m = (size_t)r * (size_t)L.Fp * (size_t)L.Fp;
  if (PASS == 0)
  {
    if (tj == T)
    {
      if ((lane & 15) == 0) L.b[(size_t)r * L.Fp + i] = sum;
      return;
    }
    const double val = (i == j && i < L.F) ? 0.00001 + sum : sum;
    L.As[m + (size_t)i * L.Fp + j] = val;
    if (ti != tj) L.As[m + (size_t)j * L.Fp + i] = val;
  }
  else
    L.Asys[m + (size_t)i * L.Fp + j] = L.As[m + (size_t)i * L.Fp + j] - sum;
}

// ------------------------------------------------------------------------------------------ solve ---
// A w = b by LU with partial pivoting (first largest magnitude, lowest row on equal magnitude), one block of 1024 threads per replica.
// The work copy [A | b] (F rows of F + 1 columns, b riding along as the last column so that the forward substitution is the
// factorisation's own U-row step) lives in global memory / L2; a panel of kPanel columns and the panel's rows of U sit in LDS.
// Right-looking, per panel: (1) the panel's columns below the diagonal into LDS; (2) kPanel pivot steps inside LDS -- block-wide
// arg-max (wave shuffles, then the 16 wave results), row swap, column / pivot, rank-1 update of the panel's remaining columns, one
// thread per row; (3) the panel back, and its row swaps applied to every other column; (4) U12 = L11^-1 A12, one thread per column;
// (5) A22 -= L21 U12 from LDS.  Then the back substitution in blocks of kPanel rows from the bottom: one thread solves the diagonal
// block out of LDS, every row above subtracts the block's contribution.  Last: w[1] = the weights the greedy choice was made on, w[0] = x.
constexpr int kPanel = 16, kPanelPitch = 17;                // odd pitch: a column walk over the panel's rows hits every bank once

__global__ __launch_bounds__(1024) void lspi_solve_kernel(LspiParams L)
{
  extern __shared__ double sh[];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = L.F, N = F + 1, LP = L.LP;
  double *sp = sh;                                          // [F][kPanelPitch]: the panel
  double *su = sp + (size_t)F * kPanelPitch;                // [kPanel][N]: U12 of the panel; later x
  double *red_v = su + (size_t)kPanel * N;                  // [16] wave maxima ...
  int *red_i = (int *)(red_v + 16);                         // ... and their rows
  int *piv = red_i + 16;                                    // [kPanel] pivot rows of the panel (global row numbers)
  double *lu = L.lu + (size_t)r * (size_t)L.Fp * (size_t)LP;
  const double *A = L.Asys + (size_t)r * (size_t)L.Fp * (size_t)L.Fp, *b = L.b + (size_t)r * L.Fp;
  bool bad = false;

  for (int i = wave; i < F; i += 16)
    for (int c = lane; c < N; c += 64) lu[(size_t)i * LP + c] = c < F ? A[(size_t)i * L.Fp + c] : b[i];
  __syncthreads();

  for (int p0 = 0; p0 < F; p0 += kPanel)
  {
    const int pw = min(kPanel, F - p0), m = F - p0, nc = N - p0 - pw;
    for (int e = tid; e < m * kPanel; e += 1024)
    {
      const int i = e >> 4, c = e & 15;
      if (c < pw) sp[i * kPanelPitch + c] = lu[(size_t)(p0 + i) * LP + p0 + c];
    }
    __syncthreads();
    for (int j = 0; j < pw; ++j)
    {
      // block-wide arg-max of |column j| over the rows j ... m - 1 (m <= 1024: one row per thread)
      double bv = -1.;
      int bi = j;
      if (tid >= j && tid < m) { bv = __builtin_fabs(sp[tid * kPanelPitch + j]); bi = tid; if (!(bv >= 0.)) bv = -1.; }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
      {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
      __syncthreads();
      bv = red_v[0]; bi = red_i[0];
#pragma unroll
      for (int k = 1; k < 16; ++k)
      {
        const double ov = red_v[k];
        const int oi = red_i[k];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (bi < j || bi >= m) bi = j;                        // (every lane outside the column reported row j with -1)
      if (tid == 0) piv[j] = p0 + bi;
      if (tid < pw && bi != j)
      {
        const double a = sp[j * kPanelPitch + tid];
        sp[j * kPanelPitch + tid] = sp[bi * kPanelPitch + tid];
        sp[bi * kPanelPitch + tid] = a;
      }
      __syncthreads();
      const double pv = sp[j * kPanelPitch + j];
      if (!(__builtin_fabs(pv) > 0. && __builtin_fabs(pv) < __builtin_inf())) bad = true;      // S9
      if (tid > j && tid < m)
      {
        const double l = sp[tid * kPanelPitch + j] / pv;
        sp[tid * kPanelPitch + j] = l;
        for (int c = j + 1; c < pw; ++c) sp[tid * kPanelPitch + c] -= l * sp[j * kPanelPitch + c];
      }
      __syncthreads();
    }
    // (3) the panel back; its swaps on the columns left and right of it
    for (int e = tid; e < m * kPanel; e += 1024)
    {
      const int i = e >> 4, c = e & 15;
      if (c < pw) lu[(size_t)(p0 + i) * LP + p0 + c] = sp[i * kPanelPitch + c];
    }
    for (int c = tid; c < N - pw; c += 1024)
    {
      const int col = c < p0 ? c : c + pw;
      for (int j = 0; j < pw; ++j)
      {
        const int pr = piv[j];
        if (pr != p0 + j)
        {
          const double a = lu[(size_t)(p0 + j) * LP + col];
          lu[(size_t)(p0 + j) * LP + col] = lu[(size_t)pr * LP + col];
          lu[(size_t)pr * LP + col] = a;
        }
      }
    }
    __syncthreads();
    // (4) U12: forward substitution with the unit lower triangle of the panel, one thread per column
    for (int c = tid; c < nc; c += 1024)
    {
      double x[kPanel];
#pragma unroll
      for (int k = 0; k < kPanel; ++k)
      {
        x[k] = 0.;
        if (k < pw)
        {
          double a = lu[(size_t)(p0 + k) * LP + p0 + pw + c];
#pragma unroll
          for (int q = 0; q < k; ++q) a -= sp[k * kPanelPitch + q] * x[q];
          x[k] = a;
          lu[(size_t)(p0 + k) * LP + p0 + pw + c] = a;
          su[k * N + c] = a;
        }
      }
    }
    __syncthreads();
    // (5) A22 -= L21 U12: a wave per row (the row's L broadcast), lanes over the columns
    for (int i = pw + wave; i < m; i += 16)
      for (int c = lane; c < nc; c += 64)
      {
        double a = lu[(size_t)(p0 + i) * LP + p0 + pw + c];
        for (int k = 0; k < pw; ++k) a -= sp[i * kPanelPitch + k] * su[k * N + c];
        lu[(size_t)(p0 + i) * LP + p0 + pw + c] = a;
      }
    __syncthreads();
  }

  // back substitution: column F of the work copy is y = L^-1 P b
  double *x = su;
  for (int i = tid; i < F; i += 1024) x[i] = lu[(size_t)i * LP + F];
  __syncthreads();
  for (int p0 = (F - 1) / kPanel * kPanel; p0 >= 0; p0 -= kPanel)
  {
    const int pw = min(kPanel, F - p0);
    if (tid < kPanel * kPanel)
    {
      const int i = tid >> 4, c = tid & 15;
      if (i < pw && c < pw) sp[i * kPanelPitch + c] = lu[(size_t)(p0 + i) * LP + p0 + c];
    }
    __syncthreads();
    if (tid == 0)
      for (int i = pw - 1; i >= 0; --i)
      {
        double s = x[p0 + i];
        for (int k = i + 1; k < pw; ++k) s -= sp[i * kPanelPitch + k] * x[p0 + k];
        x[p0 + i] = s / sp[i * kPanelPitch + i];
      }
    __syncthreads();
    for (int i = tid; i < p0; i += 1024)
    {
      double s = x[i];
      for (int k = 0; k < pw; ++k) s -= lu[(size_t)i * LP + p0 + k] * x[p0 + k];
      x[i] = s;
    }
    __syncthreads();
  }
  double *w = L.w + (size_t)r * 2 * L.Fp;
  for (int i = tid; i < F; i += 1024)
  {
    w[L.Fp + i] = w[i];
    w[i] = x[i];
  }
  if (bad && tid == 0) atomicOr(&L.rep[r].status, ST_LSPI_PIVOT);
}

// ------------------------------------------------------------------------------------------ test trial, query ---
// the test trial after a batch (batch_learning.cpp:141-186): agent/fixed + policy/discrete/q on the first maximum (S10, D7); one lane
// per replica
__global__ __launch_bounds__(64) void lspi_test_kernel(LspiParams L)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= L.R) return;
  LspiRep &rep = L.rep[r];
  const double *w = L.w + (size_t)r * 2 * L.Fp;
  uint64_t TL = rep.TL, G = rep.G;
  double x[kLspiS], obs[kLspiD], reward = 0, total = 0;
  int terminal = 0;
  int64_t ties = 0;
  uint32_t status = 0;
  Env<GRLX_ENV_PENDULUM>::start(L.env, 1, TL, G, x);
  Env<GRLX_ENV_PENDULUM>::observe(L.env, x, obs);
  for (int guard = 0; guard < GRLX_MAX_EPISODE_STEPS + 2; ++guard)
  {
    int man = 1;
    const int mai = lspi_greedy(L, w, obs, &man);
    if (terminal) break;
    ties += man > 1;
    double a = L.actions[0];
    for (int k = 1; k < L.A; ++k) a = (k == mai) ? L.actions[k] : a;
    env_step<GRLX_ENV_PENDULUM, false>(L.env, x, a, obs, reward, terminal, status);
    total += reward;
    if (terminal == 2) break;
  }
  if (rep.rows < (uint32_t)L.max_rows)
  {
    const size_t at = (size_t)r * (size_t)L.max_rows + rep.rows;
    L.row_reward[at] = total;
    L.row_batch[at] = rep.batches_done;
    L.row_transitions[at] = rep.batches_done * (int64_t)L.batch_size;
    rep.rows++;
  }
  else
    status |= ST_ROWS_FULL;
  rep.batches_done++;
  rep.ties += ties;
  rep.TL = TL;
  rep.G = G;
  rep.status |= status;
}

// grlx_lspi_query: one thread per (replica, observation), looping over the actions; q[(replica - first_replica) * n_obs + observation][A]
__global__ __launch_bounds__(64) void lspi_query_kernel(LspiParams L, int first_replica, int n_replicas, const double *obs, int n_obs, double *q)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_replicas * n_obs) return;
  const int rl = (int)(i / n_obs), o = (int)(i - (long long)rl * n_obs);
  const double *w = L.w + (size_t)(first_replica + rl) * 2 * L.Fp;
  for (int k = 0; k < L.A; ++k)
  {
    const double in[kLspiNIn] = {obs[(size_t)o * kLspiD], obs[(size_t)o * kLspiD + 1], L.actions[k]};
    q[(size_t)i * L.A + k] = lspi_read(L, w, in);
  }
}

// ------------------------------------------------------------------------------------------ launchers ---
hipError_t launch_lspi_init(const LspiParams &L, const uint64_t *r0, hipStream_t stream)
{
  hipLaunchKernelGGL(lspi_init_kernel, dim3((L.Fp + 127) / 128, L.R), dim3(128), 0, stream, L, r0);
  return hipGetLastError();
}

template <int PASS>
static hipError_t lspi_product(const LspiParams &L, int n, hipStream_t stream)
{
  // (raised once per process, unguarded: the C ABI drives one device from one thread at a time, as every context here assumes)
  static bool sized = false;
  const int T = L.Fp / 16, NT = lspi_tiles(T, PASS), splits = lspi_splits(n), chunk = lspi_chunk(n);
  const size_t lds = (size_t)(PASS == 0 ? 1 : 2) * kLspiSlab * lspi_pitch(L.Fp) * sizeof(double);
  if (!sized)
  { // up to two slabs of kLspiMaxF features: 135,168 bytes of the CU's 160 KB
    constexpr int most = 2 * kLspiSlab * lspi_pitch(lspi_padded(kLspiMaxF)) * (int)sizeof(double);
    if (hipError_t e = hipFuncSetAttribute((const void *)lspi_accumulate_kernel<PASS>, hipFuncAttributeMaxDynamicSharedMemorySize, most)) return e;
    sized = true;
  }
  hipLaunchKernelGGL(lspi_accumulate_kernel<PASS>, dim3((NT + kLspiTilesPerBlock - 1) / kLspiTilesPerBlock, splits, L.R), dim3(256), lds, stream, L, n, chunk);
  hipLaunchKernelGGL(lspi_reduce_kernel<PASS>, dim3(NT, L.R), dim3(256), 0, stream, L, splits);
  return hipGetLastError();
}

static size_t lspi_solve_lds(int F) { return ((size_t)F * kPanelPitch + (size_t)kPanel * (F + 1) + 16) * sizeof(double) + (16 + kPanel) * sizeof(int); }

// the one launch of lspi_solve_kernel: an iteration's (launch_lspi_batch) and the diagnostic's (grlx_lspi_solve_systems)
hipError_t launch_lspi_solve(const LspiParams &L, hipStream_t stream)
{
  static bool sized = false;                               // as in lspi_product: once per process, one device, one calling thread
  if (!sized)
  {
    if (hipError_t e = hipFuncSetAttribute((const void *)lspi_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lspi_solve_lds(kLspiMaxF))) return e;
    sized = true;
  }
  hipLaunchKernelGGL(lspi_solve_kernel, dim3(L.R), dim3(1024), lspi_solve_lds(L.F), stream, L);
  return hipGetLastError();
}

hipError_t launch_lspi_batch(const LspiParams &L, int batches_run, int iterations, hipStream_t stream)
{
  const int n = (batches_run + 1) * L.batch_size;
  hipLaunchKernelGGL(lspi_generate_kernel, dim3((L.batch_size + 255) / 256, L.R), dim3(256), 0, stream, L);
  hipLaunchKernelGGL(lspi_batch_begin_kernel, dim3((L.R + 63) / 64), dim3(64), 0, stream, L);
  if (hipError_t e = lspi_product<0>(L, n, stream)) return e;
  for (int ii = 0; ii < iterations; ++ii)
  {
    hipLaunchKernelGGL(lspi_greedy_kernel, dim3((n + 255) / 256, L.R), dim3(256), 0, stream, L, n);
    if (hipError_t e = lspi_product<1>(L, n, stream)) return e;
    if (hipError_t e = launch_lspi_solve(L, stream)) return e;
  }
  hipLaunchKernelGGL(lspi_test_kernel, dim3((L.R + 63) / 64), dim3(64), 0, stream, L);
  return hipGetLastError();
}

hipError_t launch_lspi_query(const LspiParams &L, int first_replica, int n_replicas, const double *obs, int n_obs, double *q, hipStream_t stream)
{
  const long long pairs = (long long)n_replicas * n_obs;
  hipLaunchKernelGGL(lspi_query_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, stream, L, first_replica, n_replicas, obs, n_obs, q);
  return hipGetLastError();
}

} // namespace grlx
