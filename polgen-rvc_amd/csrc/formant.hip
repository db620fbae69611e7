// Formant shift and envelope transfer (include/rvcx.h stage 17).  Every step is continuous in the spectrum (a maximum, a
// linear warp, a clamp), so no decision can fall the other way between float32 and float64.
//
// Kernels (256 lanes; one row = one channel of one item):
//   formant_frame_kernel   one workgroup per frame, everything in LDS and registers: window, stage 13's transform, A2 with the
//                          frame's maximum, L, the iterations + 1 lifts, warp, gain, the two energy sums, Y = (g s) D, the inverse
//                          transform and the window.  It writes the N windowed samples of the frame (and the taps when asked).
//   formant_ola_kernel     one lane per output sample (fft_device.h: ola_gather)
// LDS: the N float pairs of the transform, nothing else (64 KiB at N = 8192).  A lane keeps its bins k = lane + 256 j of D, L and
// E in registers.  The log spectra of the frame and of its source frame are both real and even, and so are their cepstra: they
// travel as the real and the imaginary part of ONE complex sequence through every lift, so a source costs one more transform
// per frame (its analysis), not 2 (iterations + 1) + 1, and when the last lift ends a[k] = (E[k], Es[k]) is what the warp gathers
// from.  The
// scratch of the two reductions lies in the same buffer, between barriers, while it holds nothing.
// Every index is bounded by the row's own T = len[r] / H + 1; nothing of a row is read or written beyond its frame T - 1.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "common.h"
#include "formant.h"

// A2, eps, L, W, g and the energy terms are defined with every rounding written out
#pragma clang fp contract(off)

#include "fft_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;

__device__ __forceinline__ unsigned brev_n(int i, int logN) { return __brev((unsigned)i) >> (32 - logN); }

// the largest value of a workgroup; scratch: 4 floats of LDS that hold nothing (barriers on both sides)
__device__ __forceinline__ float block_max(float v, float* scratch) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const float m = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
  __syncthreads();
  return m;
}

// window and transform of the frame t of one signal: a[k] = D[k] in natural order
__device__ __forceinline__ void frame_forward(float2* a, const float* __restrict__ x, long n, long t, const FxStretchGeom& g,
                                              const float* __restrict__ w, const float2* __restrict__ tw) {
  for (int i = threadIdx.x; i < g.N; i += 256) {
    const long src = t * g.H - g.N / 2 + i;
    const float v = (src >= 0 && src < n) ? w[i] * x[src] : 0.f;
    a[brev_n(i, g.logN)] = make_float2(v, 0.f);
  }
  fft_lds(a, tw, g.N, g.logN);
}

__global__ __launch_bounds__(256) void formant_frame_kernel(const FxFormantDev d) {
  extern __shared__ float2 a[];
  const FxStretchGeom g = d.g;
  const int r = blockIdx.y, N = g.N, nb = g.nb, logN = g.logN, tid = threadIdx.x;
  const long t = blockIdx.x, n = d.len[r];
  if (t >= n / g.H + 1) return;
  const bool with_src = d.src != nullptr && d.has_src[r] != 0;
  const bool tap = r == 0;
  const size_t tbase = (size_t)t * nb;
  float* scratch = reinterpret_cast<float*>(a);

  float dre[kFormantKpt], dim[kFormantKpt], L[kFormantKpt], Ls[kFormantKpt], E[kFormantKpt];
  // ---- the item's frame: D, A2, L
  frame_forward(a, d.x + (size_t)r * d.ld, n, t, g, d.w, d.tw);
  float top = 0.f;
#pragma unroll
  for (int j = 0; j < kFormantKpt; ++j) {
    const int k = tid + 256 * j;
    const float2 z = k < nb ? a[k] : make_float2(0.f, 0.f);
    dre[j] = z.x, dim[j] = z.y;
    top = fmaxf(top, fm_a2(z.x, z.y));
    if (tap && d.taps.D && k < nb) d.taps.D[tbase + k] = z;
  }
  top = block_max(top, scratch);
  {
    const float eps = fm_eps(top);
#pragma unroll
    for (int j = 0; j < kFormantKpt; ++j) L[j] = fm_log(fm_a2(dre[j], dim[j]), eps), Ls[j] = 0.f;
  }
  // ---- the source's frame: Ls
  if (with_src) {
    frame_forward(a, d.src + (size_t)r * d.ld, n, t, g, d.w, d.tw);
    float a2s[kFormantKpt];
    float tops = 0.f;
#pragma unroll
    for (int j = 0; j < kFormantKpt; ++j) {
      const int k = tid + 256 * j;
      const float2 z = k < nb ? a[k] : make_float2(0.f, 0.f);
      a2s[j] = fm_a2(z.x, z.y);
      tops = fmaxf(tops, a2s[j]);
    }
    tops = block_max(tops, scratch);
    const float eps = fm_eps(tops);
#pragma unroll
    for (int j = 0; j < kFormantKpt; ++j) Ls[j] = fm_log(a2s[j], eps);
  }
  // ---- the true envelope: V_0 = L, E = lift(V_i), V_{i+1} = max(L, E); the source rides in the imaginary part
  {
    float V[kFormantKpt], Vs[kFormantKpt];
#pragma unroll
    for (int j = 0; j < kFormantKpt; ++j) V[j] = L[j], Vs[j] = Ls[j];
    const float inv = 1.f / (float)N;
    const int nc = d.nc;
    for (int it = 0; it <= d.v.iterations; ++it) {
      // (the barrier that ended the last transform, or block_max, lies between the last reads of a and these writes)
#pragma unroll
      for (int j = 0; j < kFormantKpt; ++j) {
        const int k = tid + 256 * j;
        if (k < nb) {
          const float2 z = make_float2(V[j], Vs[j]);
          a[brev_n(k, logN)] = z;
          if (k != 0 && k != N / 2) a[brev_n(N - k, logN)] = z;
        }
      }
      fft_lds(a, d.tw, N, logN);                        // N c[q]: the inverse of a real even sequence is its forward over N
      float2 c[kFormantCpt];
#pragma unroll
      for (int i = 0; i < kFormantCpt; ++i) {
        const int q = tid + 256 * i;
        const float2 z = q <= nc ? a[q] : make_float2(0.f, 0.f);
        c[i] = make_float2(z.x * inv, z.y * inv);
      }
      __syncthreads();
      for (int i = tid; i < N; i += 256) a[i] = make_float2(0.f, 0.f);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kFormantCpt; ++i) {
        const int q = tid + 256 * i;
        if (q <= nc) {                                  // c[N - q] = c[q]: the lifted cepstrum is even by construction
          a[brev_n(q, logN)] = c[i];
          if (q != 0) a[brev_n(N - q, logN)] = c[i];
        }
      }
      fft_lds(a, d.tw, N, logN);
#pragma unroll
      for (int j = 0; j < kFormantKpt; ++j) {
        const int k = tid + 256 * j;
        const float2 e = k < nb ? a[k] : make_float2(0.f, 0.f);
        E[j] = e.x;
        V[j] = fmaxf(L[j], e.x), Vs[j] = fmaxf(Ls[j], e.y);
      }
      if (it < d.v.iterations) __syncthreads();
    }
  }
  // ---- warp, gain and the energy sums; a[i] = (E[i], Es[i]) stays untouched until every lane has gathered
  float gn[kFormantKpt];
  double e0 = 0.0, e1 = 0.0;
#pragma unroll
  for (int j = 0; j < kFormantKpt; ++j) {
    const int k = tid + 256 * j;
    gn[j] = 1.f;
    if (k < nb) {
      const float W = with_src ? fm_warp([&](int i) { return a[i].y; }, k, nb, (double)d.v.ratio)
                               : fm_warp([&](int i) { return a[i].x; }, k, nb, (double)d.v.ratio);
      gn[j] = fm_gain(W, E[j], d.v.amount, d.limit);
      fm_energy(fm_a2(dre[j], dim[j]), gn[j], k == 0 || k == nb - 1, e0, e1);
      if (tap) {
        if (d.taps.E) d.taps.E[tbase + k] = E[j];
        if (d.taps.Es) d.taps.Es[tbase + k] = with_src ? a[k].y : a[k].x;
        if (d.taps.g) d.taps.g[tbase + k] = gn[j];
      }
    }
  }
  float sc = 1.f;
  __syncthreads();
  if (d.v.keep_energy) {      // partial p over the bins k = p mod 256 in ascending k, then the partials in ascending p
    double* part = reinterpret_cast<double*>(a);          // 512 doubles = 4 KiB <= 8 N bytes (N >= 512)
    part[tid] = e0, part[256 + tid] = e1;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int p = 0; p < 256; ++p) s0 += part[p], s1 += part[256 + p];
    sc = fm_scale(s0, s1);
    __syncthreads();
  }
  if (tap && d.taps.s && tid == 0) d.taps.s[t] = sc;
  // ---- Y = (g s) D, x = Re(F(conj Y)) / N with the forward transform F (conj Y at k, Y at N - k), the window
#pragma unroll
  for (int j = 0; j < kFormantKpt; ++j) {
    const int k = tid + 256 * j;
    if (k < nb) {
      const float gs = gn[j] * sc;
      const bool edge = k == 0 || k == N / 2;
      const float re = gs * dre[j], im = edge ? 0.f : gs * dim[j];
      a[brev_n(k, logN)] = make_float2(re, -im);
      if (!edge) a[brev_n(N - k, logN)] = make_float2(re, im);
    }
  }
  fft_lds(a, d.tw, N, logN);
  float* out = d.fr + ((size_t)r * d.Tf + t) * N;
  const float inv = 1.f / (float)N;
  for (int i = tid; i < N; i += 256) out[i] = (a[i].x * inv) * d.w[i];
}

__global__ __launch_bounds__(256) void formant_ola_kernel(const FxFormantDev d, float* __restrict__ y, long ld_y) {
  const int r = blockIdx.y, N = d.g.N, H = d.g.H;
  const long n = d.len[r], m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  y[(size_t)r * ld_y + m] = ola_gather(d.fr + (size_t)r * d.Tf * N, 0, (size_t)N, d.w, m, n / H + 1, N, H);
}

}  // namespace

void launch_formant(const FxFormantDev& d, float* y, long ld_y, hipStream_t s, hipEvent_t* ev) {
  RVCX_CHECK(d.g.N >= 512 && d.g.N <= 8192 && d.g.nb <= 256 * kFormantKpt, "formant: geometry out of range");
  RVCX_CHECK(d.nc >= 1 && d.nc <= d.g.N / 8 && d.nc < 256 * kFormantCpt, "formant: quefrency out of range");
  RVCX_CHECK(d.v.iterations >= 0 && d.v.iterations <= kFormantMaxIter, "formant: iterations out of range");
  RVCX_CHECK(d.R >= 1 && d.R <= 65535, "formant: more rows than one launch takes");
  hipLaunchKernelGGL(formant_frame_kernel, dim3((unsigned)d.Tf, (unsigned)d.R), dim3(256), (size_t)d.g.N * sizeof(float2), s, d);
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(formant_ola_kernel, dim3((unsigned)cdiv64(d.ld, 256), (unsigned)d.R), dim3(256), 0, s, d, y, ld_y);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------
namespace {

using cplx = std::complex<double>;

struct HostPlan {
  FxStretchGeom g;
  std::vector<float> w;
  std::vector<cplx> tw;
  explicit HostPlan(int N) {
    g.N = N, g.H = N / 4, g.nb = N / 2 + 1, g.logN = 0;
    while ((1 << g.logN) < N) ++g.logN;
    std::vector<float2> twf;
    fx_stretch_tables(N, w, twf);
    tw.resize((size_t)N / 2);
    for (int k = 0; k < N / 2; ++k) tw[k] = cplx(std::cos(2.0 * kPi * k / N), -std::sin(2.0 * kPi * k / N));
  }
};

// E of one frame: the transforms in double, E rounded to float32 after every lift
void envelope_host(const HostPlan& P, const float* L, int nc, int iterations, float* E) {
  const int N = P.g.N, nb = P.g.nb;
  std::vector<float> V(L, L + nb);
  std::vector<cplx> buf((size_t)N);
  std::vector<double> c((size_t)nc + 1);
  for (int it = 0; it <= iterations; ++it) {
    for (int k = 0; k < nb; ++k) {
      buf[k] = cplx((double)V[k], 0.0);
      if (k != 0 && k != N / 2) buf[N - k] = buf[k];
    }
    fft_host(buf, P.tw);
    for (int q = 0; q <= nc; ++q) c[q] = buf[q].real() / (double)N;
    std::fill(buf.begin(), buf.end(), cplx(0.0, 0.0));
    for (int q = 0; q <= nc; ++q) {
      buf[q] = cplx(c[q], 0.0);
      if (q != 0) buf[N - q] = buf[q];
    }
    fft_host(buf, P.tw);
    for (int k = 0; k < nb; ++k) {
      E[k] = (float)buf[k].real();
      V[k] = E[k] > L[k] ? E[k] : L[k];
    }
  }
}

// D (nb float pairs), A2 and L of the frame t of one signal
void analyse_frame(const HostPlan& P, const float* x, long n, long t, std::vector<cplx>& buf, float* D, float* A2, float* L) {
  const int N = P.g.N, H = P.g.H, nb = P.g.nb;
  for (int i = 0; i < N; ++i) {
    const long src = t * H - N / 2 + i;
    buf[i] = (src >= 0 && src < n) ? cplx((double)P.w[i] * (double)x[src], 0.0) : cplx(0.0, 0.0);
  }
  fft_host(buf, P.tw);
  float top = 0.f;
  for (int k = 0; k < nb; ++k) {
    D[2 * k] = (float)buf[k].real(), D[2 * k + 1] = (float)buf[k].imag();
    A2[k] = fm_a2(D[2 * k], D[2 * k + 1]);
    top = std::max(top, A2[k]);
  }
  const float eps = fm_eps(top);
  for (int k = 0; k < nb; ++k) L[k] = fm_log(A2[k], eps);
}

}  // namespace

void fx_formant_envelope_host(const float* L, int N, int nc, int iterations, float* E) {
  const HostPlan P(N);
  envelope_host(P, L, nc, iterations, E);
}

void fx_formant_host(const float* x, long n, const float* src, int sr, const FxFormantValues& v, float* y, float* D_out,
                     float* E_out, float* Es_out, float* g_out, float* s_out) {
  const HostPlan P(fx_stretch_geom(sr).N);
  const int N = P.g.N, H = P.g.H, nb = P.g.nb;
  const long T = fx_stretch_T(n, H);
  const int nc = (int)fx_formant_nc(v.quefrency_ms, sr);
  const double limit = fx_formant_limit(v.max_gain_db);
  std::vector<float> D((size_t)nb * 2), Ds((size_t)nb * 2), A2((size_t)nb), A2s((size_t)nb), L((size_t)nb), E((size_t)nb),
      Es((size_t)nb), g((size_t)nb);
  std::vector<double> num((size_t)n, 0.0), den((size_t)n, 0.0);
  std::vector<cplx> buf((size_t)N);
  for (long t = 0; t < T; ++t) {
    analyse_frame(P, x, n, t, buf, D.data(), A2.data(), L.data());
    envelope_host(P, L.data(), nc, v.iterations, E.data());
    if (src) {
      analyse_frame(P, src, n, t, buf, Ds.data(), A2s.data(), L.data());
      envelope_host(P, L.data(), nc, v.iterations, Es.data());
    } else {
      Es = E;
    }
    double part0[256] = {0}, part1[256] = {0};
    for (int k = 0; k < nb; ++k) {
      const float W = fm_warp([&](int i) { return Es[(size_t)i]; }, k, nb, (double)v.ratio);
      g[k] = fm_gain(W, E[k], v.amount, limit);
      fm_energy(A2[k], g[k], k == 0 || k == nb - 1, part0[k & 255], part1[k & 255]);
    }
    float sc = 1.f;
    if (v.keep_energy) {
      double s0 = 0.0, s1 = 0.0;
      for (int p = 0; p < 256; ++p) s0 += part0[p], s1 += part1[p];
      sc = fm_scale(s0, s1);
    }
    const size_t at = (size_t)t * nb;
    if (D_out) std::copy(D.begin(), D.end(), D_out + at * 2);
    if (E_out) std::copy(E.begin(), E.end(), E_out + at);
    if (Es_out) std::copy(Es.begin(), Es.end(), Es_out + at);
    if (g_out) std::copy(g.begin(), g.end(), g_out + at);
    if (s_out) s_out[t] = sc;
    std::fill(buf.begin(), buf.end(), cplx(0.0, 0.0));
    for (int k = 0; k < nb; ++k) {
      const float gs = g[k] * sc;
      const bool edge = k == 0 || k == N / 2;
      const cplx Y((double)gs * (double)D[2 * k], edge ? 0.0 : (double)gs * (double)D[2 * k + 1]);
      buf[k] = std::conj(Y);
      if (!edge) buf[N - k] = Y;
    }
    fft_host(buf, P.tw);
    for (int i = 0; i < N; ++i) {
      const long s = t * H - N / 2 + i;
      if (s < 0 || s >= n) continue;
      num[s] += (double)P.w[i] * (buf[i].real() / N);
      den[s] += (double)P.w[i] * (double)P.w[i];
    }
  }
  for (long s = 0; s < n; ++s) y[s] = den[s] > 1e-8 ? (float)(num[s] / den[s]) : 0.f;
}

}  // namespace rvcx
