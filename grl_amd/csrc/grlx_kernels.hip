// grlx_kernels.hip -- hand-written HIP kernels (gfx950) for grl's online-learning hot path.
//
// Layout of the fused rollout kernel
// ----------------------------------
//  * one wavefront (64 lanes) = 4 independent replicas x 16 lanes; lane j of a
//    replica owns tiling j of the hashed tile coding (T = 16).
//  * per-replica scalar work (RK4 integration of the dynamics, reward, RNG,
//    epsilon-greedy) is computed redundantly by the 16 lanes of the replica --
//    the lanes would otherwise idle, and it removes every broadcast.
//  * the eligibility trace lives in registers: lane j keeps, for each of the
//    <= 10 trace entries, the table position and the AUTHORITATIVE weight of tiling j
//    (write-back: stored when the slot leaves the trace; grlx_update.h).
//  * weights live in a per-replica open-addressing table in HBM (64-byte buckets of
//    four entries, grlx_table.h), lazily initialised to the value the reference's
//    8,388,608-draw initialisation gives that slot (LCG jump-ahead, grlx_rng.h).
//  * the TD update of a step is applied one pass later, under the next step's loads.
//  * which instantiation a launch runs is decided in one place: the rows of grlx_kernel_table.h (included last), read by grlx_plan.cpp.
//  * what a trial, a counted step, a tap record and a result row are is the same in every four-replica
//    kernel: grlx_frame.h (included after grlx_update.h, before the first rollout header).
//  * sums over the 16 tilings are taken in the reference's serial order
//    (linear.cpp:147-151) through a 4-way interleaved LDS tile, so Q-values are
//    bit-identical to a scalar run.
//
// Compiled with -ffp-contract=off: the reference's arithmetic is plain IEEE
// double without fused multiply-add (x86-64 baseline); only grlx_math.h fuses.
#include <cstdio>
#include <cstdlib>
#include "grlx_internal.h"
#include "grlx_math.h"
#include "grlx_rng.h"
#include "grlx_tile.h"
#include "grlx_table.h"
#include "grlx_envs.h"
#include "grlx_policy.h"

namespace grlx {


// ------------------------------------------------------- fused rollout -----
// LDS tile shared by the 4 replicas of the wave; index (row*16 + tiling)*4 + group
// makes both the per-lane writes and the 4 simultaneous broadcast reads conflict-free.
#define SHW(row, k, g) sh_w[(((row) * 16 + (k)) << 2) + (g)]


} // namespace grlx

#include "grlx_update.h"
#include "grlx_frame.h"
#include "grlx_env_server.h"
#include "grlx_env_server_wide.h"
#include "grlx_rollout.h"
#include "grlx_rollout_wide.h"
#include "grlx_rollout_ac.h"
#include "grlx_rollout_ac_wide.h"
#include "grlx_rollout_qv.h"
#include "grlx_rollout_acc.h"
#include "grlx_rollout_tgt.h"
#include "grlx_step.h"

namespace grlx {

// ------------------------------------------------------ register poisoning ---
// Every vector register (v0..v255, a0..a255: one wave owns a SIMD's whole file) and the SGPRs a kernel may be given
// are set to `pattern`.  The clobber lists make the compiler declare all of them for this kernel; the writes
// themselves are assembler repeat blocks.
#define GRLX_D10(p) p "0", p "1", p "2", p "3", p "4", p "5", p "6", p "7", p "8", p "9"
#define GRLX_D100(p) GRLX_D10(p "0"), GRLX_D10(p "1"), GRLX_D10(p "2"), GRLX_D10(p "3"), GRLX_D10(p "4"), GRLX_D10(p "5"), GRLX_D10(p "6"), GRLX_D10(p "7"), GRLX_D10(p "8"), GRLX_D10(p "9")
#define GRLX_ALL256(p) GRLX_D10(p), GRLX_D10(p "1"), GRLX_D10(p "2"), GRLX_D10(p "3"), GRLX_D10(p "4"), GRLX_D10(p "5"), GRLX_D10(p "6"), GRLX_D10(p "7"), GRLX_D10(p "8"), GRLX_D10(p "9"), \
  GRLX_D100(p "1"), GRLX_D10(p "20"), GRLX_D10(p "21"), GRLX_D10(p "22"), GRLX_D10(p "23"), GRLX_D10(p "24"), p "250", p "251", p "252", p "253", p "254", p "255"
__global__ __launch_bounds__(64) void poison_registers_kernel(uint32_t pattern)
{
  asm volatile(
      "v_mov_b32 v0, %0\n"
      ".set grlx_i, 0\n"
      ".rept 256\n"
      "  v_accvgpr_write_b32 a[grlx_i], v0\n"
      "  .set grlx_i, grlx_i + 1\n"
      ".endr\n"
      ".set grlx_i, 1\n"
      ".rept 255\n"
      "  v_mov_b32 v[grlx_i], %0\n"
      "  .set grlx_i, grlx_i + 1\n"
      ".endr\n"
      ".set grlx_i, 20\n"
      ".rept 12\n"                      // s20..s31; s32..s34 are the ABI's stack / frame / base pointer registers: not clobbered
      "  s_mov_b32 s[grlx_i], %0\n"
      "  .set grlx_i, grlx_i + 1\n"
      ".endr\n"
      ".set grlx_i, 35\n"
      ".rept 65\n"                      // s35..s99
      "  s_mov_b32 s[grlx_i], %0\n"
      "  .set grlx_i, grlx_i + 1\n"
      ".endr\n"
      :: "s"(pattern) : "memory", GRLX_ALL256("v"), GRLX_ALL256("a"), GRLX_D10("s2"), "s30", "s31", "s35", "s36", "s37", "s38", "s39", GRLX_D10("s4"), GRLX_D10("s5"),
         GRLX_D10("s6"), GRLX_D10("s7"), GRLX_D10("s8"), GRLX_D10("s9"));
}
#undef GRLX_ALL256
#undef GRLX_D100
#undef GRLX_D10

__global__ void set_u32_kernel(uint32_t *p, uint32_t v) { *p = v; }

hipError_t launch_poison_registers(uint32_t pattern, hipStream_t stream)
{ // one wave fills a SIMD; several rounds over the chip's SIMDs so that none is missed
  hipLaunchKernelGGL(poison_registers_kernel, dim3(8192), dim3(64), 0, stream, pattern);
  return hipGetLastError();
}

hipError_t launch_set_u32(uint32_t *p, uint32_t v, hipStream_t stream)
{
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, stream, p, v);
  return hipGetLastError();
}

// -------------------------------------------------- fine-grained kernels ---
// Projector::project, batched: one lane per (row, tiling)
__global__ void project_kernel(TileParams tp, const double *in, int n, uint32_t *out)
{
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int row = gid / tp.T, j = gid % tp.T;
  if (row >= n) return;
  out[(size_t)row * tp.T + j] = tile_slot_generic(tp, in + (size_t)row * tp.D, j);
}

hipError_t launch_project(const TileParams &tp, const double *in_dev, int n, uint32_t *out_dev, hipStream_t stream)
{
  long total = (long)n * tp.T;
  int blocks = (int)((total + 255) / 256);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(project_kernel, dim3(blocks), dim3(256), 0, stream, tp, in_dev, n, out_dev);
  return hipGetLastError();
}

// Does every sin/cos evaluation of one control step get an argument inside its domain (|x| < 2^20)?  The caller of grlx_env_step may
// hand in ANY state; in_domain() looks at step ends only, and a state it accepts can take an RK4 stage beyond 2^20 and come back
// (the cart-pole from |theta| > 2^17: see env_step, grlx_envs.h), where the unchecked psin / pcos return unspecified values.  A
// second pass over the stages of rk4_step -- the same operations on the same values, hence the same stage states -- that looks at
// the arguments and keeps nothing else.  The compass walker integrates itself and is not covered (its own rates carry the angles
// out of in_domain() long before a stage leaves the sine's domain).
template <int ENV>
__device__ bool stage_arguments_in_domain(const DevParams &P, const double *x, double u)
{
  constexpr int S = Env<ENV>::S, SD = S - 1;
  const double h = P.h;
  double xd[S], k1[SD], k2[SD], k3[SD], k4[SD], t[S], next[S];
  for (int i = 0; i < S; ++i) { next[i] = x[i]; t[i] = x[i]; }
  const typename Env<ENV>::Consts ec = Env<ENV>::template consts<false>();
  bool ok = true;
  for (int ii = 0; ii < P.integration_steps; ++ii)
  {
    ok = ok && Env<ENV>::arguments_in_domain(next);
    Env<ENV>::eom(ec, next, u, xd);
    for (int i = 0; i < SD; ++i) { k1[i] = h * xd[i]; t[i] = next[i] + k1[i] / 2; }
    ok = ok && Env<ENV>::arguments_in_domain(t);
    Env<ENV>::eom(ec, t, u, xd);
    for (int i = 0; i < SD; ++i) { k2[i] = h * xd[i]; t[i] = next[i] + k2[i] / 2; }
    ok = ok && Env<ENV>::arguments_in_domain(t);
    Env<ENV>::eom(ec, t, u, xd);
    for (int i = 0; i < SD; ++i) { k3[i] = h * xd[i]; t[i] = next[i] + k3[i]; }
    ok = ok && Env<ENV>::arguments_in_domain(t);
    Env<ENV>::eom(ec, t, u, xd);
    for (int i = 0; i < SD; ++i)
    {
      k4[i] = h * xd[i];
      next[i] = next[i] + div6(k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    }
  }
  return ok;
}

// Environment::step, batched: one lane per environment instance
template <int ENV>
__global__ void env_step_kernel(DevParams P, double *state, const double *action, int n,
                                double *obs, double *reward, int32_t *terminal, uint32_t *err)
{
  constexpr int S = Env<ENV>::S, D = Env<ENV>::D;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x[S], o[D], rw;
  int term;
  for (int k = 0; k < S; ++k) x[k] = state[(size_t)i * S + k];
  uint32_t st = 0;
  if (!Env<ENV>::in_domain(x)) st |= ST_DOMAIN;
  if constexpr (!HasCustomModel<ENV>::value)
    if (!stage_arguments_in_domain<ENV>(P, x, Env<ENV>::actuate(action[i]))) st |= ST_DOMAIN;
  env_step<ENV>(P, x, action[i], o, rw, term, st);
  for (int k = 0; k < S; ++k) state[(size_t)i * S + k] = x[k];
  for (int k = 0; k < D; ++k) obs[(size_t)i * D + k] = o[k];
  reward[i] = rw;
  terminal[i] = term;
  bool bad = st != 0;
  for (int k = 0; k < S; ++k) bad = bad || (x[k] != x[k]);
  if (bad) atomicOr(err, ST_DOMAIN);
}

hipError_t launch_env_step(const DevParams &P, double *state_dev, const double *action_dev, int n,
                           double *obs_dev, double *reward_dev, int32_t *terminal_dev, uint32_t *err_dev, hipStream_t stream)
{
  int blocks = (n + 63) / 64;
  if (blocks == 0) return hipSuccess;
  switch (P.env)
  {
    case GRLX_ENV_PENDULUM:
      hipLaunchKernelGGL(env_step_kernel<GRLX_ENV_PENDULUM>, dim3(blocks), dim3(64), 0, stream, P, state_dev, action_dev, n,
                         obs_dev, reward_dev, terminal_dev, err_dev);
      break;
    case GRLX_ENV_ACROBOT:
      hipLaunchKernelGGL(env_step_kernel<GRLX_ENV_ACROBOT>, dim3(blocks), dim3(64), 0, stream, P, state_dev, action_dev, n,
                         obs_dev, reward_dev, terminal_dev, err_dev);
      break;
    case GRLX_ENV_CART_POLE:
      hipLaunchKernelGGL(env_step_kernel<GRLX_ENV_CART_POLE>, dim3(blocks), dim3(64), 0, stream, P, state_dev, action_dev, n,
                         obs_dev, reward_dev, terminal_dev, err_dev);
      break;
    case GRLX_ENV_COMPASS_WALKER:
      hipLaunchKernelGGL(env_step_kernel<GRLX_ENV_COMPASS_WALKER>, dim3(blocks), dim3(64), 0, stream, P, state_dev, action_dev, n,
                         obs_dev, reward_dev, terminal_dev, err_dev);
      break;
    case GRLX_ENV_CART_POLE_BALANCING:
      hipLaunchKernelGGL(env_step_kernel<GRLX_ENV_CART_POLE_BALANCING>, dim3(blocks), dim3(64), 0, stream, P, state_dev, action_dev, n,
                         obs_dev, reward_dev, terminal_dev, err_dev);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// Representation::read / write / update on rows applied in order (one wave; lane j = tiling j).
// op 0 read, 1 write(target, alpha), 2 update(delta)
__global__ __launch_bounds__(64) void table_op_kernel(DevParams P, int table, int op, const int32_t *replica, const uint32_t *idx, int n,
                                                      const double *arg, double alpha, double *out)
{
  __shared__ double   sh[64];
  __shared__ uint32_t shp[64];
  const int lane = threadIdx.x & 63;
  const int Tn = P.tile.T;
  uint32_t status = 0, inserted = 0, inserted_twin = 0;
  for (int i = 0; i < n; ++i)
  {
    const int r = replica[i];
    const Table tab = table_of(P, table, r);
    const bool act = lane < Tn;
    uint32_t slot = act ? idx[(size_t)i * Tn + lane] : 0u, pos = 0;
    const bool valid = act && slot != 0xFFFFFFFFu;     // invalid_index(): skipped by update (linear.cpp:207)
    double w = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const LinearParams &lp = table == 1 ? P.lin_actor : P.lin;
    if (P.twin_tables)
    {
      const Table other = table_of(P, 1 - table, r);
      const LinearParams &olp = table == 1 ? P.lin : P.lin_actor;
      table_probe(tab, lp, P.states[r], table, valid, slot, pos, w, status, inserted, &other, &olp, &inserted_twin);
    }
    else
      table_probe(tab, lp, P.states[r], table, valid, slot, pos, w, status, inserted);
    sh[lane] = w;
    shp[lane] = valid ? pos : kInvalidPos;
    wave_sync();
    double s = 0;
    for (int k = 0; k < Tn; ++k) s += sh[k];
    s /= Tn;
    s = clampd(s, lp.out_min, lp.out_max);
    if (op == 0)
    {
      if (lane == 0) out[i] = s;
    }
    else
    {
      double d = (op == 1) ? alpha * (arg[i] - s) : arg[i];
      if (valid)
      { // sequential semantics for duplicate slots: c additions, highest lane's value is final
        uint32_t c = 0;
        for (int k = 0; k <= lane; ++k) c += (shp[k] == pos) ? 1u : 0u;
        bool last = true;
        for (int k = lane + 1; k < Tn; ++k) last = last && (shp[k] != pos);
        double v = w;
        for (uint32_t cc = 0; cc < c; ++cc)
          v = lp.limit ? clampd(v + d, lp.out_min, lp.out_max) : v + d;
        if (last) value_store(tab, pos, v);
      }
    }
    wave_sync();
    uint32_t ins = inserted;
    for (int off = 32; off > 0; off >>= 1) ins += __shfl_xor(ins, off, 64);
    if (lane == 0 && ins) P.states[r].n_slots[table] += ins;
    inserted = 0;
    if (P.twin_tables)
    {
      uint32_t it = inserted_twin;
      for (int off = 32; off > 0; off >>= 1) it += __shfl_xor(it, off, 64);
      if (lane == 0 && it) P.states[r].n_slots[1 - table] += it;
      inserted_twin = 0;
    }
    // sticky status of the replica this row worked on (not of the first row's)
    uint32_t st = status;
    for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off, 64);
    if (lane == 0 && st) atomicOr(&P.states[r].status, st);
    status = 0;
  }
}

hipError_t launch_table_op(const DevParams &P, int table, int op, const int32_t *replica_dev, const uint32_t *idx_dev, int n,
                           const double *arg_dev, double alpha, double *out_dev, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(table_op_kernel, dim3(1), dim3(64), 0, stream, P, table, op, replica_dev, idx_dev, n, arg_dev, alpha, out_dev);
  return hipGetLastError();
}

// current weight of reference slots (lazy value when the slot was never touched; no insertion)
__global__ void get_weights_kernel(DevParams P, int table, int replica, const uint32_t *slots, int n, double *out)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Table tab = table_of(P, table, replica);
  uint32_t slot = slots[i], pos;
  out[i] = table_peek(tab, slot, pos) ? value_load(tab, pos) : initial_weight(P.states[replica], table, table == 1 ? P.lin_actor : P.lin, slot);
}

// {action: load}: replicas [first, first+count) take `image` as the initial value of every slot of
// `table` and forget what they had learned in it (their sparse tables are cleared by the caller)
__global__ void set_lazy_base_kernel(DevParams P, int table, int first, int count, const double *image)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  ReplicaState &rs = P.states[first + i];
  rs.lazy_base[table] = image;
  rs.n_slots[table] = 0u;
}

hipError_t launch_set_lazy_base(const DevParams &P, int table, int first, int count, const double *image_dev, hipStream_t stream)
{
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(set_lazy_base_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, P, table, first, count, image_dev);
  return hipGetLastError();
}

// dense export of a table: out[slot] for every reference slot (grid-stride)
__global__ void export_weights_kernel(DevParams P, int table, int replica, double *out)
{
  const Table tab = table_of(P, table, replica);
  const LinearParams &lp = table == 1 ? P.lin_actor : P.lin;
  const uint32_t memory = (uint32_t)(table == 1 ? P.tile_actor.memory : P.tile.memory);
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < memory; slot += gridDim.x * blockDim.x)
  {
    uint32_t pos;
    out[slot] = table_peek(tab, slot, pos) ? value_load(tab, pos) : initial_weight(P.states[replica], table, lp, slot);
  }
}

hipError_t launch_export_weights(const DevParams &P, int table, int replica, double *out_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(export_weights_kernel, dim3(2048), dim3(256), 0, stream, P, table, replica, out_dev);
  return hipGetLastError();
}

hipError_t launch_get_weights(const DevParams &P, int table, int replica, const uint32_t *slots_dev, int n, double *out_dev, hipStream_t stream)
{
  int blocks = (n + 255) / 256;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(get_weights_kernel, dim3(blocks), dim3(256), 0, stream, P, table, replica, slots_dev, n, out_dev);
  return hipGetLastError();
}

__global__ void math_kernel(int op, const double *x, const double *y, int n, double *out)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = x[i], r;
  switch (op)
  {
    case 0: r = psin_checked(v); break;
    case 1: r = pcos_checked(v); break;
    case 2: r = plog(v); break;
    case 3: r = pfmod(v, y[i]); break;
    case 5: r = div6(v); break;
    case 6: r = psin_s(v, sin_consts<false>()); break;       // small-angle-aware forms (whole waves of small arguments take the short path)
    case 7: r = pcos_s(v, sin_consts<false>()); break;
    case 8: { double sn, cs; psincos_s(v, sin_consts<false>(), sn, cs); r = sn + cs; break; }
    // the forms the rollout kernels and the environment servers call, with their constants: unchecked, the host refuses |x| >= 2^20
    case 9: r = psin<false>(v, sin_consts<true>()); break;
    case 10: r = psin<true>(v, sin_consts<kPinAdditive>()); break;       // the served pendulum's: sign by integer add
    case 11: r = pcos(v, sin_consts<true>()); break;
    case 12: { double sn, cs; psincos(v, sin_consts<true>(), sn, cs); r = sn + cs; break; }
    case 13: r = pexp(v); break;
    default: r = __builtin_sqrt(v); break;
  }
  out[i] = r;
}

hipError_t launch_math(int op, const double *x, const double *y, int n, double *out, hipStream_t stream)
{
  int blocks = (n + 255) / 256;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(math_kernel, dim3(blocks), dim3(256), 0, stream, op, x, y, n, out);
  return hipGetLastError();
}

__global__ void rand48_at_kernel(uint64_t x0, const uint64_t *skip, int n, double *out)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = lcg_double(lcg_next(lcg_jump(x0, skip[i])));
}

hipError_t launch_rand48_at(uint64_t x0, const uint64_t *skip, int n, double *out, hipStream_t stream)
{
  int blocks = (n + 255) / 256;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(rand48_at_kernel, dim3(blocks), dim3(256), 0, stream, x0, skip, n, out);
  return hipGetLastError();
}

// learning-curve statistics over the replicas of this GPU: one block per row, fixed-order tree
__global__ __launch_bounds__(256) void curve_stats_kernel(DevParams P, int first, double *out)
{
  __shared__ double s1[256], s2[256];
  const int row = first + blockIdx.x;
  __shared__ double s3[256];
  double a = 0, b = 0, n = 0;
  for (int r = threadIdx.x; r < P.n_replicas; r += 256)
    if ((uint32_t)row < P.states[r].rows)          // rows are ragged when replicas stop at a steps budget (grlx_run_steps)
    {
      double v = P.row_reward[(size_t)row * P.n_replicas + r];
      a += v;
      b += v * v;
      n += 1;
    }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  s3[threadIdx.x] = n;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
    {
      s1[threadIdx.x] += s1[threadIdx.x + off];
      s2[threadIdx.x] += s2[threadIdx.x + off];
      s3[threadIdx.x] += s3[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0)
  {
    out[blockIdx.x * 3 + 0] = s1[0];
    out[blockIdx.x * 3 + 1] = s2[0];
    out[blockIdx.x * 3 + 2] = s3[0];
  }
}

hipError_t launch_curve_stats(const DevParams &P, int first, int count, double *out_dev, hipStream_t stream)
{
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(curve_stats_kernel, dim3(count), dim3(256), 0, stream, P, first, out_dev);
  return hipGetLastError();
}

// ... over groups of group_size consecutive replicas (the repetitions of one point of a sweep): one block per (row, group); every
// thread accumulates strided over its group, then the same tree.  out[row][group][3]; block = row * n_groups + group
__global__ __launch_bounds__(256) void curve_stats_grouped_kernel(DevParams P, int first, int group_size, double *out)
{
  __shared__ double s1[256], s2[256], s3[256];
  const int n_groups = P.n_replicas / group_size;
  const int row = first + (int)(blockIdx.x / (unsigned)n_groups);
  const int r0 = (int)(blockIdx.x % (unsigned)n_groups) * group_size;
  double a = 0, b = 0, n = 0;
  for (int k = threadIdx.x; k < group_size; k += 256)
  {
    const int r = r0 + k;
    if (r < P.n_replicas && (uint32_t)row < P.states[r].rows)
    {
      double v = P.row_reward[(size_t)row * P.n_replicas + r];
      a += v;
      b += v * v;
      n += 1;
    }
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  s3[threadIdx.x] = n;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
    {
      s1[threadIdx.x] += s1[threadIdx.x + off];
      s2[threadIdx.x] += s2[threadIdx.x + off];
      s3[threadIdx.x] += s3[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0)
  {
    const size_t at = (size_t)blockIdx.x * 3;
    out[at + 0] = s1[0];
    out[at + 1] = s2[0];
    out[at + 2] = s3[0];
  }
}

hipError_t launch_curve_stats_grouped(const DevParams &P, int first, int count, int group_size, double *out_dev, hipStream_t stream)
{
  if (count == 0) return hipSuccess;
  if (group_size < 1 || P.n_replicas % group_size != 0) return hipErrorInvalidValue;
  const long long blocks = (long long)count * (P.n_replicas / group_size);
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(curve_stats_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, P, first, group_size, out_dev);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void step_counts_kernel(DevParams P, uint64_t *out)
{
  __shared__ unsigned long long a[256], b[256], c[256];
  unsigned long long la = 0, lb = 0, lc = 0;
  for (int r = threadIdx.x; r < P.n_replicas; r += 256)
  {
    la += (unsigned long long)P.states[r].ss;
    lb += P.states[r].test_steps;
    lc |= P.states[r].status;
  }
  a[threadIdx.x] = la; b[threadIdx.x] = lb; c[threadIdx.x] = lc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off)
    {
      a[threadIdx.x] += a[threadIdx.x + off];
      b[threadIdx.x] += b[threadIdx.x + off];
      c[threadIdx.x] |= c[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = a[0]; out[1] = b[0]; out[2] = c[0]; }
}

hipError_t launch_step_counts(const DevParams &P, uint64_t *out_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(step_counts_kernel, dim3(1), dim3(256), 0, stream, P, out_dev);
  return hipGetLastError();
}

// ------------------------------------------------------------ table growth ---
__global__ __launch_bounds__(256) void max_load_kernel(DevParams P, int n_tables, uint32_t *out)
{
  __shared__ uint32_t m[256];
  uint32_t v = 0;
  for (int r = threadIdx.x; r < P.n_replicas; r += 256)
    for (int t = 0; t < n_tables; ++t) v = max(v, P.states[r].n_slots[t]);
  m[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off) m[threadIdx.x] = max(m[threadIdx.x], m[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = m[0];
}

hipError_t launch_max_load(const DevParams &P, int n_tables, uint32_t *out_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(max_load_kernel, dim3(1), dim3(256), 0, stream, P, n_tables, out_dev);
  return hipGetLastError();
}

// One wave per (table, replica): the 64 lanes walk the old buckets and claim ways of the new table with a compare-and-swap
// on the key word (the new table is at most a quarter full, probes are short).  Key word (slot, creating tiling, shared bit),
// claim word and value move unchanged; only the position changes.
__global__ __launch_bounds__(64) void rehash_kernel(DevParams P, int n_tables, Entry *new_tables, uint32_t new_logC, uint32_t *remap)
{
  const int r = blockIdx.x % P.n_replicas, table = blockIdx.x / P.n_replicas;
  if (table >= n_tables) return;
  // twin tables keep the same slot at the same position: table 0's placement decides, table 1's entries follow it
  const bool twin = P.twin_tables != 0 && n_tables == 2;
  if (twin && table == 1) return;
  const Table ot = table_of(P, table, r);
  const Table ot2 = table_of(P, twin ? 1 : table, r);
  Table nt2 = ot2;
  nt2.base = reinterpret_cast<Bucket *>(new_tables + ((((size_t)(twin ? 1 : table)) * (size_t)P.n_replicas + (size_t)r) << new_logC));
  nt2.bmask = (1u << (new_logC - 2)) - 1u;
  nt2.shift = 32u - (new_logC - 2);
  Table nt;
  nt.base = reinterpret_cast<Bucket *>(new_tables + (((size_t)table * (size_t)P.n_replicas + (size_t)r) << new_logC));
  nt.bmask = (1u << (new_logC - 2)) - 1u;
  nt.shift = 32u - (new_logC - 2);
  uint32_t *map = (remap && table == 0) ? remap + ((size_t)r << P.logC) : nullptr;
  const uint32_t n_buckets = 1u << (P.logC - 2);
  for (uint32_t b = threadIdx.x; b < n_buckets; b += 64)
  {
    const Bucket ob = ot.base[b];
    for (int way = 0; way < 4; ++way)
    {
      const uint32_t kw = ob.key[way];
      if (map) map[b * 4 + way] = kInvalidPos;
      if ((kw & kKeyMask) == 0u) continue;
      uint32_t nb = table_home(nt, (kw & kKeyMask) - 1u);
      uint32_t at = kInvalidPos;
      for (int it = 0; it < kMaxProbe && at == kInvalidPos; ++it)
      {
        for (int w = 0; w < 4; ++w)
          if (atomicCAS(&nt.base[nb].key[w], 0u, kw) == 0u) { at = (nb << 2) | (uint32_t)w; break; }
        if (at == kInvalidPos) nb = (nb + 1u) & nt.bmask;
      }
      if (at == kInvalidPos) { atomicOr(&P.states[r].status, ST_TABLE_FULL); continue; }
      nt.base[at >> 2].aux[at & 3u] = ob.aux[way];
      nt.base[at >> 2].val[at & 3u] = ob.val[way];
      if (twin)
      {
        nt2.base[at >> 2].key[at & 3u] = kw;
        nt2.base[at >> 2].aux[at & 3u] = ot2.base[b].aux[way];
        nt2.base[at >> 2].val[at & 3u] = ot2.base[b].val[way];
      }
      if (map) map[b * 4 + way] = at;
    }
  }
}

// setParams() on a table whose entries must stay where they are (twin tables): every existing entry takes the image's value of its slot
__global__ __launch_bounds__(64) void reload_entries_kernel(DevParams P, int table, int first_replica, const double *image)
{
  const int r = first_replica + blockIdx.x;
  const Table t = table_of(P, table, r);
  const uint32_t n_buckets = 1u << (P.logC - 2);
  for (uint32_t b = threadIdx.x; b < n_buckets; b += 64)
    for (int way = 0; way < 4; ++way)
    {
      const uint32_t kw = t.base[b].key[way] & kKeyMask;
      if (kw != 0u) t.base[b].val[way] = image[kw - 1u];
    }
}

hipError_t launch_reload_entries(const DevParams &P, int table, int first_replica, int n_replicas, const double *image_dev, hipStream_t stream)
{
  if (n_replicas <= 0) return hipSuccess;
  hipLaunchKernelGGL(reload_entries_kernel, dim3(n_replicas), dim3(64), 0, stream, P, table, first_replica, image_dev);
  return hipGetLastError();
}

hipError_t launch_rehash(const DevParams &P, int n_tables, Entry *new_tables, uint32_t new_logC, uint32_t *remap_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(rehash_kernel, dim3(P.n_replicas * n_tables), dim3(64), 0, stream, P, n_tables, new_tables, new_logC, remap_dev);
  return hipGetLastError();
}

// positions kept outside the tables: the actor-critic's persisted critic trace and the target network's values
__global__ __launch_bounds__(64) void remap_positions_kernel(DevParams P, const uint32_t *remap, uint32_t new_logC, double *new_tvals)
{
  const int r = blockIdx.x;
  const uint32_t *map = remap + ((size_t)r << P.logC);
  if (P.trace_state)
  {
    uint32_t *ts = P.trace_state + (size_t)r * 16 * kMaxTrace * 2;
    for (int k = threadIdx.x; k < 16 * kMaxTrace; k += 64)
    {
      const uint32_t pos = ts[k * 2];
      if (pos != kInvalidPos) ts[k * 2] = map[pos & ((1u << P.logC) - 1u)];
    }
  }
  if (P.tvals && new_tvals)
  {
    const double *otv = P.tvals + ((size_t)r << P.logC);
    double *ntv = new_tvals + ((size_t)r << new_logC);
    for (uint32_t p = threadIdx.x; p < (1u << P.logC); p += 64)
      if (map[p] != kInvalidPos) ntv[map[p]] = otv[p];
  }
}

hipError_t launch_remap_positions(const DevParams &P, const uint32_t *remap_dev, uint32_t new_logC, double *new_tvals, hipStream_t stream)
{
  hipLaunchKernelGGL(remap_positions_kernel, dim3(P.n_replicas), dim3(64), 0, stream, P, remap_dev, new_logC, new_tvals);
  return hipGetLastError();
}

} // namespace grlx

#include "grlx_kernel_table.h"      // last: every rollout kernel is instantiated by its row
