// grlx_lspi_read.h -- the projection and the read of the LSPI context's representation (S3-S5, D2-D5 of grlx_lspi.h), as device
// functions: what grlx_lspi.hip (the greedy choice, the accumulation, the test trial, the query) and grlx_lspi_evaluate.hip (the
// evaluation episodes, whose quad kernels are held to these bits) both include, after grlx_math.h and grlx_lspi.h.
#pragma once

namespace grlx {

// TriangleRBFProjector::project (rbf.cpp:99-150): the base cell and the 8 (index, weight) pairs in the reference's ii order (S3)
__device__ __forceinline__ void lspi_triangle(const LspiParams &L, const double (&in)[kLspiNIn], int (&idx)[8], double (&wt)[8])
{
  int index = 0;
  double dist[kLspiNIn];
#pragma unroll
  for (int dd = 0; dd < kLspiNIn; ++dd)
  {
    const double gridpos = fmin(fmax((in[dd] - L.in_min[dd]) / L.delta[dd], 0.), L.top[dd]);
    const int v = (int)gridpos;
    index += v * L.stride[dd];
    dist[dd] = gridpos - v;
  }
#pragma unroll
  for (int ii = 0; ii < 8; ++ii)
  {
    int diff = 0;
    double w = 1;
#pragma unroll
    for (int dd = 0; dd < kLspiNIn; ++dd)
    {
      const bool edge = (ii & (1 << dd)) > 0;
      diff += edge * L.stride[dd];
      w *= edge ? dist[dd] : (1 - dist[dd]);
    }
    idx[ii] = index + diff;
    wt[ii] = w;
  }
}

// GaussianRBFProjector::project (rbf.cpp:173-211) at basis function (k0, k1, k2), deviations D2-D5: its weight, or a negative number
// where the cutoff drops it (a kept weight is an exponential: never negative)
__device__ __forceinline__ double lspi_gauss(const LspiParams &L, const double (&base)[kLspiNIn], int k0, int k1, int k2)
{
  const double d0 = base[0] + k0, d1 = base[1] + k1, d2 = base[2] + k2;
  const double distsq = d0 * d0 + d1 * d1 + d2 * d2;
  if (!(distsq < L.cutoff_distsq)) return -1.;
  return pexp(-distsq / L.sigmasq);
}
__device__ __forceinline__ void lspi_gauss_base(const LspiParams &L, const double (&in)[kLspiNIn], double (&base)[kLspiNIn])
{
#pragma unroll
  for (int dd = 0; dd < kLspiNIn; ++dd) base[dd] = (L.in_min[dd] - in[dd]) / L.delta[dd];
}

// LinearRepresentation::read over the unpruned projection (S5)
__device__ __forceinline__ double lspi_read(const LspiParams &L, const double *w, const double (&in)[kLspiNIn])
{
  double q = 0;
  if (L.projector == GRLX_RBF_TRIANGLE)
  {
    int idx[8];
    double wt[8];
    lspi_triangle(L, in, idx, wt);
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) q += w[idx[ii]] * wt[ii];
  }
  else
  {
    double base[kLspiNIn];
    lspi_gauss_base(L, in, base);
    int f = 0;
    for (int k2 = 0; k2 < L.steps[2]; ++k2)
      for (int k1 = 0; k1 < L.steps[1]; ++k1)
        for (int k0 = 0; k0 < L.steps[0]; ++k0, ++f)
        {
          const double g = lspi_gauss(L, base, k0, k1, k2);
          if (g >= 0.) q += w[f] * g;
        }
  }
  return q;
}

} // namespace grlx
