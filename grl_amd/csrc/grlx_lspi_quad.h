// grlx_lspi_quad.h -- the device helpers of the LSPI context's episode kernels (grlx_lspi_evaluate.hip, grlx_lspi_evaluate_sampled.hip):
// the quad's exchange, findmax over the action slots, what a lane keeps about its actions, the box of the Gauss walk and the quad's reads.
// Included after grlx_math.h, grlx_lspi_read.h and grlx_lspi_evaluate.h.  Every function is inlined: the kernels of
// grlx_lspi_evaluate.hip, which carried these lines themselves, keep their instructions.
#pragma once

namespace grlx {

// ------------------------------------------------------------------------------------------ the quad ---
// v of lane SRC of the caller's quad, in every lane of it (v_mov_b32 with quad_perm:[SRC, SRC, SRC, SRC], twice)
template <int SRC>
__device__ __forceinline__ double quad_bcast(double v)
{
  constexpr int ctrl = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  int lo = (int)(unsigned)b, hi = (int)(unsigned)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// all[k] = own[k / 4] of lane k % 4: the values of all action slots, in every lane of the quad.  Every lane of the quad must be here.
__device__ __forceinline__ void quad_exchange(const double (&own)[kLspiOwn], double (&all)[kMaxActions])
{
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o)
  {
    all[4 * o + 0] = quad_bcast<0>(own[o]);
    all[4 * o + 1] = quad_bcast<1>(own[o]);
    all[4 * o + 2] = quad_bcast<2>(own[o]);
    all[4 * o + 3] = quad_bcast<3>(own[o]);
  }
}

// findmax (grlx_episode.h) over the first A of kMaxActions values, A uniform: the first maximum, the number of maxima, the maximum
__device__ __forceinline__ void lspi_findmax(const double (&v)[kMaxActions], int A, int &mai, int &man, double &best)
{
  mai = 0; man = 1;
  best = v[0];
#pragma unroll
  for (int a = 1; a < kMaxActions; ++a)
    if (a < A)
    {
      if (v[a] > best) { best = v[a]; mai = a; man = 1; }
      else if (v[a] == best) man++;
    }
}

__device__ __forceinline__ double lspi_action_of(const LspiParams &L, int k)
{
  double action = L.actions[0];
#pragma unroll
  for (int a = 1; a < kMaxActions; ++a) action = (k == a) ? L.actions[a] : action;
  return action;
}

// ------------------------------------------------------------------------------------------ the lane's actions ---
// what a lane keeps about the action slots it owns (actions a + 4 o below action_steps), formed once before the loop
template <int PROJ> struct LspiActs;
template <> struct LspiActs<GRLX_RBF_TRIANGLE> {
  bool   has[kLspiOwn];
  int    off[kLspiOwn];                    // cell of the action dimension x its stride
  double d[kLspiOwn], omd[kLspiOwn];       // dist of the action dimension, and 1 - dist
};
template <> struct LspiActs<GRLX_RBF_GAUSS> {
  bool   has[kLspiOwn];
  double base2[kLspiOwn];                  // lspi_gauss_base's third component
  int    lo2[kLspiOwn], hi2[kLspiOwn];     // lspi_box of the action dimension
  double rad;
};

// the radius lspi_box takes from the context's bound (below): on the device, and on the host where a launcher sizes what holds a box
__host__ __device__ inline double lspi_box_radius(double cutoff_distsq) { return sqrt(cutoff_distsq) * (1 + 1e-9) + 1e-9; }

// The range [lo, hi] of k outside which |base + k| < sqrt(cutoff_distsq) cannot hold, clamped to the grid (lo > hi: nothing is kept).
// rad is that root widened by 1e-9, relatively and absolutely: a kept function has fl(d * d) < cutoff_distsq for d = fl(base + k), so
// |base + k| < root (1 + 2^-53) + ulp(base) / 2, and |base| stays below 2^17 / delta < 2^20, whose ulp is 2^-32; forming -base -+ rad
// errs by as much again.  Both are far inside the widening, and floor / ceil only move the bounds further out.
__device__ __forceinline__ void lspi_box(double base, double rad, int steps, int &lo, int &hi)
{
  const double top = (double)(steps - 1);
#ifdef GRLX_LSPI_EVAL_FULL_WALK
  base = -0.5 * top; rad = top;            // measurement build: every k of the grid
#endif
  lo = (int)fmin(fmax(floor(-base - rad), 0.), top + 1);
  hi = (int)fmax(fmin(ceil(-base + rad), top), -1.);
}

template <int PROJ>
__device__ __forceinline__ void lspi_acts(const LspiParams &L, int a, LspiActs<PROJ> &act)
{
  if constexpr (PROJ == GRLX_RBF_GAUSS) act.rad = lspi_box_radius(L.cutoff_distsq);
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o)
  {
    const int k = a + kLspiQuad * o;
    act.has[o] = k < L.A;
    const double ak = lspi_action_of(L, k);
    if constexpr (PROJ == GRLX_RBF_TRIANGLE)
    { // lspi_triangle's dd = 2
      const double gridpos = fmin(fmax((ak - L.in_min[2]) / L.delta[2], 0.), L.top[2]);
      const int v = (int)gridpos;
      act.off[o] = v * L.stride[2];
      act.d[o] = gridpos - v;
      act.omd[o] = 1 - act.d[o];
    }
    else
    { // lspi_gauss_base's dd = 2
      act.base2[o] = (L.in_min[2] - ak) / L.delta[2];
      lspi_box(act.base2[o], act.rad, L.steps[2], act.lo2[o], act.hi2[o]);
    }
  }
}

// ------------------------------------------------------------------------------------------ the reads ---
// q[o] = the read of S5 at (obs, the lane's action o) on the weights w; slots the lane does not own stay 0.  w: LDS (the single
// policy) or global (a member of a group).
template <int PROJ>
__device__ __forceinline__ void lspi_quad_reads(const LspiParams &L, const LspiActs<PROJ> &act, const double (&obs)[kLspiD], const double *w,
                                                double (&q)[kLspiOwn])
{
#pragma unroll
  for (int o = 0; o < kLspiOwn; ++o) q[o] = 0;
  if constexpr (PROJ == GRLX_RBF_TRIANGLE)
  {
    // lspi_triangle's dd = 0, 1 and the products over them, once for all actions
    int index = 0;
    double dist[kLspiD];
#pragma unroll
    for (int dd = 0; dd < kLspiD; ++dd)
    {
      const double gridpos = fmin(fmax((obs[dd] - L.in_min[dd]) / L.delta[dd], 0.), L.top[dd]);
      const int v = (int)gridpos;
      index += v * L.stride[dd];
      dist[dd] = gridpos - v;
    }
    double c[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
    {
      double p = 1;
#pragma unroll
      for (int dd = 0; dd < kLspiD; ++dd) p *= (ii & (1 << dd)) ? dist[dd] : (1 - dist[dd]);
      c[ii] = p;
    }
#pragma unroll
    for (int o = 0; o < kLspiOwn; ++o)
      if (act.has[o])
      {
#pragma unroll
        for (int ii = 0; ii < 8; ++ii)
        {
          const int id = index + act.off[o] + ((ii & 1) ? L.stride[0] : 0) + ((ii & 2) ? L.stride[1] : 0) + ((ii & 4) ? L.stride[2] : 0);
          const double wt = c[ii & 3] * ((ii & 4) ? act.d[o] : act.omd[o]);
          q[o] += w[id] * wt;
        }
      }
  }
  else
  {
    int lo0, hi0, lo1, hi1;
    const double b0 = (L.in_min[0] - obs[0]) / L.delta[0], b1 = (L.in_min[1] - obs[1]) / L.delta[1];      // lspi_gauss_base's dd = 0, 1
    lspi_box(b0, act.rad, L.steps[0], lo0, hi0);
    lspi_box(b1, act.rad, L.steps[1], lo1, hi1);
    const int s0 = L.steps[0], s01 = L.steps[0] * L.steps[1];
#pragma unroll
    for (int o = 0; o < kLspiOwn; ++o)
      if (act.has[o])
      {
        const double base[kLspiNIn] = {b0, b1, act.base2[o]};
        for (int k2 = act.lo2[o]; k2 <= act.hi2[o]; ++k2)
          for (int k1 = lo1; k1 <= hi1; ++k1)
            for (int k0 = lo0; k0 <= hi0; ++k0)
            {
              const double g = lspi_gauss(L, base, k0, k1, k2);
              if (g >= 0.) q[o] += w[k2 * s01 + k1 * s0 + k0] * g;
            }
      }
  }
}

// behind an episode's end: all-zero bits up to max_steps, a quarter per lane
template <int R>
__device__ __forceinline__ void lspi_record_zeros(double *rec, int a, int steps, int max_steps)
{
  for (size_t k = (size_t)steps * R + (size_t)a; k < (size_t)max_steps * R; k += kLspiQuad) rec[k] = 0.;
}

} // namespace grlx
