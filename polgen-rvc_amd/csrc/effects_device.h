// Post-production: the single-rounding arithmetic and the per-sample step functions that every effects translation unit
// shares (effects.hip: the one-shot kernels and the host twins; effects_live.hip: the board inside a live session).  One
// definition of each step is what makes "bit for bit" between them a statement about order alone.
#pragma once
#include <cmath>

#include "effects.h"

// every rounding below is written out: nothing may be fused behind the source's back, on either side
#pragma clang fp contract(off)

namespace rvcx {

// ---- single-rounding arithmetic shared by host and device ----------------------------------------------------------------
// With contraction off (above) a product, a difference, fmaf and sqrtf are each ONE IEEE operation rounded to nearest on
// both sides: __fmaf_rn is v_fma_f32 on the device, sqrtf the correctly rounded sequence (HIP's default; the other __f*_rn
// intrinsics are not used: without OCML_BASIC_ROUNDED_OPERATIONS __fsqrt_rn is the approximate native root).
#if defined(__HIP_DEVICE_COMPILE__)
#define FX_FMA(a, b, c) __fmaf_rn((a), (b), (c))
#else
#define FX_FMA(a, b, c) fmaf((a), (b), (c))
#endif
#define FX_MUL(a, b) ((a) * (b))
#define FX_SUB(a, b) ((a) - (b))
#define FX_SQRT(a) sqrtf((a))

__host__ __device__ inline float fx_bq_step(const FxBiquad& q, float x, float& s1, float& s2) {
  const float y = FX_FMA(q.b0, x, s1);
  s1 = FX_FMA(q.b1, x, FX_FMA(-q.a1, y, s2));
  s2 = FX_FMA(q.b2, x, FX_MUL(-q.a2, y));
  return y;
}

// e[n] = a + c (e[n-1] - a), a = |x| or x^2, c the attack constant while a > e[n-1]
__host__ __device__ inline float fx_follow_step(float x, float e, int square, float c_att, float c_rel) {
  const float a = square ? FX_MUL(x, x) : fabsf(x);
  const float c = a > e ? c_att : c_rel;
  return FX_FMA(c, FX_SUB(e, a), a);
}

__host__ __device__ inline float fx_gain(float e, int gate, float thr, float expo) {
  if (gate) return e > thr ? 1.f : powf(e / thr, expo);
  return e < thr ? 1.f : powf(e / thr, expo);
}

__host__ __device__ inline int16_t fx_mix_sample(int v, int i, double gv, double gi) {
  double a = floor((double)v * gv), b = floor((double)i * gi);
  a = a < -32768.0 ? -32768.0 : a > 32767.0 ? 32767.0 : a;
  b = b < -32768.0 ? -32768.0 : b > 32767.0 ? 32767.0 : b;
  const int t = (int)a + (int)b;
  return (int16_t)(t < -32768 ? -32768 : t > 32767 ? 32767 : t);
}

// w[n]: the delay line d read at n - tau(n), linear interpolation, zero in front of sample 0
// (Line: anything indexable by a global sample index -- a row, or a session's ring)
template <typename Line>
__host__ __device__ inline float fx_chorus_tap(const FxChorus& c, const Line& d, long n) {
  const double m = c.centre + c.dep10 * sin(c.w * (double)n);
  const double pos = (double)n - c.srk * (m < 1.0 ? 1.0 : m);
  const double fl = floor(pos);
  const long i0 = (long)fl;
  const float fr = (float)(pos - fl);
  const float d0 = i0 >= 0 ? d[i0] : 0.f, d1 = i0 + 1 >= 0 ? d[i0 + 1] : 0.f;
  return FX_FMA(fr, FX_SUB(d1, d0), d0);
}

}  // namespace rvcx
