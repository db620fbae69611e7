// One frame of the formant stages on the device (include/rvcx.h stage 17, and stage 19 on the live grid): what formant.hip and
// formant_live.hip share, so that the chain of a frame exists once.  A 256-lane workgroup takes the frame through everything in
// LDS and registers: window, stage 13's transform, A2 with the frame's maximum, L, the iterations + 1 lifts, warp, gain, the two
// energy sums, Y = (g s) D, the inverse transform and the window.  Every rounding is written out (formant.h: contraction is off in
// whichever file includes this one).
//
// LDS: the N float pairs of the transform, nothing else.  A lane keeps its bins k = lane + 256 j, j < KPT, of D, L and E in
// registers, and its kept quefrencies q = lane + 256 i, i < CPT: the caller instantiates the body for the largest N it launches
// (256 KPT >= nb, 256 CPT > nc), so a stage with small transforms does not carry the registers of one with large ones.  The
// scratch of the two reductions lies in the same buffer, between barriers, while it holds nothing.
//
// SRC: the frame may have a source frame.  The log spectra of the frame and of its source frame are both real and even, and so
// are their cepstra: they travel as the real and the imaginary part of ONE complex sequence through every lift, so a source
// costs one more transform per frame (its analysis), not 2 (iterations + 1) + 1, and when the last lift ends a[k] = (E[k], Es[k])
// is what the warp gathers from.  Without SRC the imaginary part is zero going into every lift.
#pragma once
#include "fft_device.h"
#include "formant.h"

namespace rvcx {

struct FmFrameArgs {
  FxStretchGeom g;
  FxFormantValues v;
  int nc;
  double limit;                          // max_gain_db ln(10) / 20
  const float* w;
  const float2* tw;
};
struct FmFrameTaps {                     // this frame's rows (nb values each, s one), each optional
  float2* D = nullptr;
  float* E = nullptr;
  float* Es = nullptr;
  float* g = nullptr;
  float* s = nullptr;
};

__device__ __forceinline__ unsigned fm_brev(int i, int logN) { return __brev((unsigned)i) >> (32 - logN); }

// the largest value of a workgroup; scratch: 4 floats of LDS that hold nothing (barriers on both sides)
__device__ __forceinline__ float fm_block_max(float v, float* scratch) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const float m = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
  __syncthreads();
  return m;
}

// window and transform of one frame: a[k] = D[k] in natural order.  sample(i, v): the frame's sample i into v, false where the
// signal has none (the frame then holds 0 there)
template <typename Sample>
__device__ __forceinline__ void fm_frame_forward(float2* a, Sample sample, const FmFrameArgs& q) {
  for (int i = threadIdx.x; i < q.g.N; i += 256) {
    float x = 0.f;
    const float v = sample(i, x) ? q.w[i] * x : 0.f;
    a[fm_brev(i, q.g.logN)] = make_float2(v, 0.f);
  }
  fft_lds(a, q.tw, q.g.N, q.g.logN);
}

// out: the N windowed samples of the frame.  with_src (SRC only): this frame has a source, read through sample_src
template <int KPT, int CPT, bool SRC, typename Sample, typename SampleSrc>
__device__ __forceinline__ void fm_frame_body(float2* a, const FmFrameArgs& q, Sample sample, SampleSrc sample_src, bool with_src,
                                              const FmFrameTaps& taps, float* __restrict__ out) {
  const int N = q.g.N, nb = q.g.nb, logN = q.g.logN, tid = threadIdx.x;
  float* scratch = reinterpret_cast<float*>(a);
  with_src = SRC && with_src;

  float dre[KPT], dim[KPT], L[KPT], Ls[KPT], E[KPT];
  // ---- the item's frame: D, A2, L
  fm_frame_forward(a, sample, q);
  float top = 0.f;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + 256 * j;
    const float2 z = k < nb ? a[k] : make_float2(0.f, 0.f);
    dre[j] = z.x, dim[j] = z.y;
    top = fmaxf(top, fm_a2(z.x, z.y));
    if (taps.D && k < nb) taps.D[k] = z;
  }
  top = fm_block_max(top, scratch);
  {
    const float eps = fm_eps(top);
#pragma unroll
    for (int j = 0; j < KPT; ++j) L[j] = fm_log(fm_a2(dre[j], dim[j]), eps), Ls[j] = 0.f;
  }
  // ---- the source's frame: Ls
  if (SRC && with_src) {
    fm_frame_forward(a, sample_src, q);
    float a2s[KPT];
    float tops = 0.f;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + 256 * j;
      const float2 z = k < nb ? a[k] : make_float2(0.f, 0.f);
      a2s[j] = fm_a2(z.x, z.y);
      tops = fmaxf(tops, a2s[j]);
    }
    tops = fm_block_max(tops, scratch);
    const float eps = fm_eps(tops);
#pragma unroll
    for (int j = 0; j < KPT; ++j) Ls[j] = fm_log(a2s[j], eps);
  }
  // ---- the true envelope: V_0 = L, E = lift(V_i), V_{i+1} = max(L, E); the source rides in the imaginary part
  {
    float V[KPT], Vs[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) V[j] = L[j], Vs[j] = Ls[j];
    const float inv = 1.f / (float)N;
    const int nc = q.nc;
    for (int it = 0; it <= q.v.iterations; ++it) {
      // (the barrier that ended the last transform, or fm_block_max, lies between the last reads of a and these writes)
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int k = tid + 256 * j;
        if (k < nb) {
          const float2 z = make_float2(V[j], SRC ? Vs[j] : 0.f);
          a[fm_brev(k, logN)] = z;
          if (k != 0 && k != N / 2) a[fm_brev(N - k, logN)] = z;
        }
      }
      fft_lds(a, q.tw, N, logN);                        // N c[q]: the inverse of a real even sequence is its forward over N
      float2 c[CPT];
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int qq = tid + 256 * i;
        const float2 z = qq <= nc ? a[qq] : make_float2(0.f, 0.f);
        c[i] = make_float2(z.x * inv, z.y * inv);
      }
      __syncthreads();
      for (int i = tid; i < N; i += 256) a[i] = make_float2(0.f, 0.f);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int qq = tid + 256 * i;
        if (qq <= nc) {                                 // c[N - q] = c[q]: the lifted cepstrum is even by construction
          a[fm_brev(qq, logN)] = c[i];
          if (qq != 0) a[fm_brev(N - qq, logN)] = c[i];
        }
      }
      fft_lds(a, q.tw, N, logN);
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int k = tid + 256 * j;
        const float2 e = k < nb ? a[k] : make_float2(0.f, 0.f);
        E[j] = e.x;
        V[j] = fmaxf(L[j], e.x), Vs[j] = fmaxf(Ls[j], e.y);
      }
      if (it < q.v.iterations) __syncthreads();
    }
  }
  // ---- warp, gain and the energy sums; a[i] = (E[i], Es[i]) stays untouched until every lane has gathered
  float gn[KPT];
  double e0 = 0.0, e1 = 0.0;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + 256 * j;
    gn[j] = 1.f;
    if (k < nb) {
      const float W = with_src ? fm_warp([&](int i) { return a[i].y; }, k, nb, (double)q.v.ratio)
                               : fm_warp([&](int i) { return a[i].x; }, k, nb, (double)q.v.ratio);
      gn[j] = fm_gain(W, E[j], q.v.amount, q.limit);
      fm_energy(fm_a2(dre[j], dim[j]), gn[j], k == 0 || k == nb - 1, e0, e1);
      if (taps.E) taps.E[k] = E[j];
      if (taps.Es) taps.Es[k] = with_src ? a[k].y : a[k].x;
      if (taps.g) taps.g[k] = gn[j];
    }
  }
  float sc = 1.f;
  __syncthreads();
  if (q.v.keep_energy) {      // partial p over the bins k = p mod 256 in ascending k, then the partials in ascending p
    double* part = reinterpret_cast<double*>(a);          // 512 doubles = 4 KiB <= 8 N bytes (N >= 512)
    part[tid] = e0, part[256 + tid] = e1;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int p = 0; p < 256; ++p) s0 += part[p], s1 += part[256 + p];
    sc = fm_scale(s0, s1);
    __syncthreads();
  }
  if (taps.s && tid == 0) *taps.s = sc;
  // ---- Y = (g s) D, x = Re(F(conj Y)) / N with the forward transform F (conj Y at k, Y at N - k), the window
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + 256 * j;
    if (k < nb) {
      const float gs = gn[j] * sc;
      const bool edge = k == 0 || k == N / 2;
      const float re = gs * dre[j], im = edge ? 0.f : gs * dim[j];
      a[fm_brev(k, logN)] = make_float2(re, -im);
      if (!edge) a[fm_brev(N - k, logN)] = make_float2(re, im);
    }
  }
  fft_lds(a, q.tw, N, logN);
  const float inv = 1.f / (float)N;
  for (int i = tid; i < N; i += 256) out[i] = (a[i].x * inv) * q.w[i];
}

}  // namespace rvcx
