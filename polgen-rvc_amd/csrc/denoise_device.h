// The pointwise rules of noise reduction, one text for the kernels and the host twins of stage 15 (denoise.hip) and stage 16
// (denoise_live.hip).  Every rounding is written out: the file that includes this one has contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

namespace rvcx {

__host__ __device__ inline float dn_level(float s) { return 10.f * log10f(s + 1e-20f); }
__host__ __device__ inline float dn_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__host__ __device__ inline float dn_mask0(float l, double mu, double sd, float n_std, float knee) {
  const double thr = mu + (double)n_std * sd;
  return dn_sigmoid((float)(((double)l - thr) / (double)knee));
}
__host__ __device__ inline float dn_mask1(double A, double b, float thresh_mult, float slope) {
  const double r = (A - b) / (b + 1e-10);
  return dn_sigmoid((float)((r - (double)thresh_mult) * (double)slope));
}
__host__ __device__ inline float dn_gain(float strength, float m) { return 1.f - strength * (1.f - m); }
// the weights of the indices i + d, |d| <= h, that lie in 0 .. n - 1
__host__ __device__ inline int dn_weight_sum(long i, long n, int h) {
  const long lo = -(long)h > -i ? -(long)h : -i, hi = (long)h < n - 1 - i ? (long)h : n - 1 - i;
  int s = 0;
  for (long d = lo; d <= hi; ++d) s += h + 1 - (int)(d < 0 ? -d : d);
  return s;
}

}  // namespace rvcx
