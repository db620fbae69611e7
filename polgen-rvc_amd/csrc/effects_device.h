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

// ---- stages 9 - 12 ---------------------------------------------------------------------------------------------------------------
// one sample through the shelf and the high-pass of the K-weighting filter, in double; st: the four states
__host__ __device__ inline double fx_kw_step(const FxKWeight& k, double x, double* st) {
  const double v = fma(k.sb0, x, st[0]);
  st[0] = fma(k.sb1, x, fma(-k.sa1, v, st[1]));
  st[1] = fma(k.sb2, x, -k.sa2 * v);
  const double y = fma(k.hb0, v, st[2]);
  st[2] = fma(k.hb1, v, fma(-k.ha1, y, st[3]));
  st[3] = fma(k.hb2, v, -k.ha2 * y);
  return y;
}

// z of a block from four hop sums per channel (s: the first of the four), channels in order; h: samples per hop
__host__ __device__ inline double fx_block_z(const double* s, long stride, int C, long h) {
  double z = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* q = s + (long)c * stride;
    z += ((q[0] + q[1]) + q[2]) + q[3];
  }
  return z / (4.0 * (double)h);
}
__host__ __device__ inline double fx_lufs(double z) { return -0.691 + 10.0 * log10(z); }

// one phase of the interpolator at a sample: w[0] = x[n + 12] ... w[-23] = x[n - 11], taps j = 0 .. 23 in that order
__host__ __device__ inline float fx_tp_phase(const float* w, const float* h) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < kTpTaps; ++j) acc = FX_FMA(w[-j], h[j], acc);
  return acc;
}

// u = 1 - g rounded UP: the smallest float32 with 1 - u <= g.  Rounding to nearest can leave 1 - u above g by 2^-25 once
// g < 0.5; with this u the limiter's bound s[n] <= r[n] holds in float32 as it does in exact arithmetic (1 - u is exact
// for u >= 0.5, and for u < 0.5 the difference 1 - g was exact to begin with).
__host__ __device__ inline float fx_one_minus_up(float g) {
  const float u = FX_SUB(1.f, g);
  return FX_SUB(1.f, u) > g ? nextafterf(u, 2.f) : u;
}

__host__ __device__ inline int16_t fx_pcm16(float y) {
  const float v = rintf(FX_MUL(32768.f, y));
  return (int16_t)(v < -32768.f ? -32768.f : v > 32767.f ? 32767.f : v);
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
