// grlx_softmax.h -- the softmax distribution of the batch path's sampled ensembles (fqi_ensemble_sampled_kernel in grlx_fqi.hip,
// lspi_ensemble_sampled_kernel in grlx_lspi_evaluate_sampled.hip): the members' under GRLX_MEMBER_SOFTMAX and the combined one over the
// integer scores.  Included after grlx_math.h (pexp).
#pragma once

namespace grlx {

// SoftmaxSampler::distribution (softmax.cpp:65-110) over the first NA of v[] at temperature t, as include/grlx.h restates it; entries
// behind NA come out 0.  NA is a kernel argument: every branch on it is scalar.
__device__ __forceinline__ void batch_softmax(const double (&v)[kMaxActions], int NA, double t, double (&d)[kMaxActions])
{
  double p[kMaxActions], e[kMaxActions];
  double maxp = -0x1.fffffffffffffp+1023;                 // -DBL_MAX
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a)
  {
    p[a] = v[a] / t;
    if (a < NA) maxp = (maxp < p[a]) ? p[a] : maxp;
  }
  const double minp = maxp + (-100), center = (maxp + minp) / 2.0;
  double sum = 0;
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a)
  {
    e[a] = 0.0;
    if (a < NA)
    {
      const bool kept = p[a] > minp;
      e[a] = kept ? pexp(p[a] - center) : 0.0;
      sum = kept ? sum + e[a] : sum;
    }
  }
#pragma unroll
  for (int a = 0; a < kMaxActions; ++a) d[a] = (a < NA && p[a] > minp) ? e[a] / sum : 0.0;
}

} // namespace grlx
