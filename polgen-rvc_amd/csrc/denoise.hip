// Noise reduction (include/rvcx.h stage 15): a soft spectral gate.  The gate decision is a sigmoid on a smoothed level, so
// it is continuous in the spectrum; every sum that could depend on a tile or chunk border is taken in a fixed order.
//
// Kernels (256 lanes; one row = one channel of one item or noise clip):
//   denoise_fft_kernel     one workgroup per frame: window, stage 13's transform in LDS, epilogue D (items) and A2 (no fma)
//   denoise_smooth_kernel  one workgroup per tile of kDenoiseTileT x kDenoiseTileK outputs: A2 with its halo in LDS, the
//                          frequency triangle, then the time triangle, each sum in ascending index order over the indices
//                          inside the grid, divided by the weights of those indices
//   denoise_stats_kernel   mode 0, one lane per (row, bin): mean and deviation of the level over the profile frames, two
//                          passes in double, partial sums over kDenoiseStatChunk frames added in chunk order
//   denoise_mask0_kernel   mode 0, one workgroup per frame: m from S, mu and sd
//   denoise_floor_kernel   mode 1, one lane per (row, bin): f forward, then b and m backward, in double
//   denoise_ifft_kernel    one workgroup per frame: g from m, Y = g D, the Hermitian spectrum, the transform, the window;
//                          the N samples go where the frame's D was
//   denoise_ola_kernel     one lane per output sample (fft_device.h: ola_gather)
// Every index is bounded by the row's own T = len[r] / H + 1; nothing of a row is read or written beyond its frame T - 1.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "common.h"
#include "denoise.h"

// A2, S, l, m and g are defined with every rounding written out
#pragma clang fp contract(off)

#include "denoise_device.h"   // the pointwise rules, one text for the kernels and the host twins
#include "fft_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int kDenoiseAhead = 8;          // frames the floor kernel fetches at once
static_assert(kDenoiseTileK == 64, "the smoothing kernel gives a lane to each bin of a tile row");

__device__ __forceinline__ long rows_T(const FxDenoiseRows& q, int r, int H) { return (long)q.len[r] / H + 1; }

__global__ __launch_bounds__(256) void denoise_fft_kernel(const FxStretchGeom g, const float* __restrict__ w,
                                                          const float2* __restrict__ tw, const FxDenoiseRows q) {
  extern __shared__ float2 a[];
  const int r = blockIdx.y, N = g.N, H = g.H, nb = g.nb, logN = g.logN;
  const long t = blockIdx.x, n = q.len[r];
  if (t >= n / H + 1) return;
  const size_t base = ((size_t)r * q.Tf + t) * nb;
  const float* __restrict__ x = q.x + (size_t)r * q.ld;
  for (int i = threadIdx.x; i < N; i += 256) {
    const long src = t * H - N / 2 + i;
    const float v = (src >= 0 && src < n) ? w[i] * x[src] : 0.f;
    a[__brev((unsigned)i) >> (32 - logN)] = make_float2(v, 0.f);
  }
  fft_lds(a, tw, N, logN);
  for (int k = threadIdx.x; k < nb; k += 256) {
    const float2 z = a[k];
    if (q.D) q.D[base + k] = z;
    q.A2[base + k] = __fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y));
  }
}

__global__ __launch_bounds__(256) void denoise_smooth_kernel(const int nb, const int H, const int nf, const int nt,
                                                             const FxDenoiseRows q) {
  extern __shared__ float sm[];
  const int r = blockIdx.z, k0 = blockIdx.x * kDenoiseTileK;
  const long t0 = (long)blockIdx.y * kDenoiseTileT, T = rows_T(q, r, H);
  if (t0 >= T) return;
  const int ht = kDenoiseTileT + 2 * nt, wk = kDenoiseTileK + 2 * nf;
  float* a2 = sm;                            // ht x wk: A2 with its halo, 0 outside the grid (never summed)
  float* F = sm + ht * wk;                   // ht x kDenoiseTileK: the frequency pass
  // a wave per tile row, a lane per bin of it (kDenoiseTileK == 64): no index is divided
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ src = q.A2 + (size_t)r * q.Tf * nb;
  for (int tt = wave; tt < ht; tt += 4) {
    const long t = t0 - nt + tt;
    const bool row_ok = t >= 0 && t < T;
    for (int kk = lane; kk < wk; kk += 64) {
      const int k = k0 - nf + kk;
      a2[tt * wk + kk] = (row_ok && k >= 0 && k < nb) ? src[(size_t)t * nb + k] : 0.f;
    }
  }
  __syncthreads();
  const int k = k0 + lane;
  const int klo = max(-nf, -k), khi = min(nf, nb - 1 - k);
  for (int tt = wave; tt < ht; tt += 4) {
    float s = 0.f;
    if (k < nb) {
      const float* row = a2 + tt * wk + lane + nf;
      for (int dk = klo; dk <= khi; ++dk) s = __fadd_rn(s, __fmul_rn((float)(nf + 1 - abs(dk)), row[dk]));
    }
    F[tt * kDenoiseTileK + lane] = s;
  }
  __syncthreads();
  if (k >= nb) return;
  float* __restrict__ dst = q.S + (size_t)r * q.Tf * nb;
  const int wsum_k = dn_weight_sum(k, nb, nf);
  for (int tt = wave; tt < kDenoiseTileT; tt += 4) {
    const long t = t0 + tt;
    if (t >= T) break;
    const int lo = (int)max(-(long)nt, -t), hi = (int)min((long)nt, T - 1 - t);
    float s = 0.f;
    for (int dt = lo; dt <= hi; ++dt)
      s = __fadd_rn(s, __fmul_rn((float)(nt + 1 - abs(dt)), F[(tt + nt + dt) * kDenoiseTileK + lane]));
    dst[(size_t)t * nb + k] = s / (float)(dn_weight_sum(t, T, nt) * wsum_k);
  }
}

__global__ __launch_bounds__(256) void denoise_stats_kernel(const FxDenoiseDev d) {
  const int r = blockIdx.y, nb = d.g.nb, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const int p = d.prof[r];
  const FxDenoiseRows& q = p < 0 ? d.it : d.nz;
  const int pr = p < 0 ? r : p;
  const long Tp = rows_T(q, pr, d.g.H);
  const float* __restrict__ S = q.S + (size_t)pr * q.Tf * nb + k;
  double tot = 0.0;
  for (long c0 = 0; c0 < Tp; c0 += kDenoiseStatChunk) {
    double part = 0.0;
    for (long t = c0; t < min(c0 + kDenoiseStatChunk, Tp); ++t) part += (double)dn_level(S[(size_t)t * nb]);
    tot += part;
  }
  const double mean = tot / (double)Tp;
  tot = 0.0;
  for (long c0 = 0; c0 < Tp; c0 += kDenoiseStatChunk) {
    double part = 0.0;
    for (long t = c0; t < min(c0 + kDenoiseStatChunk, Tp); ++t) {
      const double e = (double)dn_level(S[(size_t)t * nb]) - mean;
      part += e * e;
    }
    tot += part;
  }
  d.mu[(size_t)r * nb + k] = mean;
  d.sd[(size_t)r * nb + k] = sqrt(tot / (double)Tp);
}

__global__ __launch_bounds__(256) void denoise_mask0_kernel(const FxDenoiseDev d) {
  const int r = blockIdx.y, nb = d.g.nb;
  const long t = blockIdx.x;
  if (t >= rows_T(d.it, r, d.g.H)) return;
  const size_t base = ((size_t)r * d.it.Tf + t) * nb;
  for (int k = threadIdx.x; k < nb; k += 256)
    d.it.A2[base + k] = dn_mask0(dn_level(d.it.S[base + k]), d.mu[(size_t)r * nb + k], d.sd[(size_t)r * nb + k], d.v.n_std, d.v.knee_db);
}

__global__ __launch_bounds__(256) void denoise_floor_kernel(const FxDenoiseDev d) {
  const int r = blockIdx.y, nb = d.g.nb, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const long T = rows_T(d.it, r, d.g.H);
  const size_t base = (size_t)r * d.it.Tf * nb + k;
  const float* __restrict__ S = d.it.S + base;
  double* __restrict__ f = d.f + base;
  float* __restrict__ m = d.it.A2 + base;
  const double c = d.c, omc = 1.0 - c;
  // The recurrences are serial in t, the loads are not: kDenoiseAhead frames are fetched at once and then walked in order,
  // so that a row of few lanes (one mono clip: nb lanes) does not pay a memory latency per frame.  The arithmetic and its
  // order are those of the plain loop.
  double run = (double)sqrtf(S[0]);                       // f[-1] = A[0]
  for (long t0 = 0; t0 < T; t0 += kDenoiseAhead) {
    float sv[kDenoiseAhead];
#pragma unroll
    for (int i = 0; i < kDenoiseAhead; ++i) sv[i] = t0 + i < T ? S[(size_t)(t0 + i) * nb] : 0.f;
#pragma unroll
    for (int i = 0; i < kDenoiseAhead; ++i)
      if (t0 + i < T) {
        run = omc * (double)sqrtf(sv[i]) + c * run;
        f[(size_t)(t0 + i) * nb] = run;
      }
  }
  for (long t1 = T - 1; t1 >= 0; t1 -= kDenoiseAhead) {     // b[T] = f[T - 1]
    float sv[kDenoiseAhead];
    double fv[kDenoiseAhead];
#pragma unroll
    for (int i = 0; i < kDenoiseAhead; ++i) {
      sv[i] = t1 - i >= 0 ? S[(size_t)(t1 - i) * nb] : 0.f;
      fv[i] = t1 - i >= 0 ? f[(size_t)(t1 - i) * nb] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kDenoiseAhead; ++i)
      if (t1 - i >= 0) {
        run = omc * fv[i] + c * run;
        if (d.b) d.b[base + (size_t)(t1 - i) * nb] = run;
        m[(size_t)(t1 - i) * nb] = dn_mask1((double)sqrtf(sv[i]), run, d.v.thresh_mult, d.v.slope);
      }
  }
}

__global__ __launch_bounds__(256) void denoise_ifft_kernel(const FxDenoiseDev d) {
  extern __shared__ float2 a[];
  const int r = blockIdx.y, N = d.g.N, nb = d.g.nb, logN = d.g.logN;
  const long t = blockIdx.x;
  if (t >= rows_T(d.it, r, d.g.H)) return;
  const size_t base = ((size_t)r * d.it.Tf + t) * nb;
  for (int k = threadIdx.x; k < nb; k += 256) {
    const float gk = dn_gain(d.v.strength, d.it.A2[base + k]);
    const float2 z = d.it.D[base + k];
    const bool edge = k == 0 || k == N / 2;               // irfft ignores the imaginary part of the two real bins
    const float re = gk * z.x, im = edge ? 0.f : gk * z.y;
    // x = Re(F(conj Y)) / N with the forward transform F: conj Y at k, Y at N - k
    a[__brev((unsigned)k) >> (32 - logN)] = make_float2(re, -im);
    if (!edge) a[__brev((unsigned)(N - k)) >> (32 - logN)] = make_float2(re, im);
  }
  fft_lds(a, d.tw, N, logN);                              // (its barriers lie between the reads of D above and the writes below)
  float* out = reinterpret_cast<float*>(d.it.D + base);   // N floats inside the frame's own nb pairs (2 nb = N + 2)
  const float inv = 1.f / (float)N;
  for (int i = threadIdx.x; i < N; i += 256) out[i] = (a[i].x * inv) * d.w[i];
}

__global__ __launch_bounds__(256) void denoise_ola_kernel(const FxDenoiseDev d, float* __restrict__ y, long ld_y) {
  const int r = blockIdx.y, N = d.g.N, H = d.g.H;
  const long n = d.it.len[r], m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  const float* fr = reinterpret_cast<const float*>(d.it.D + (size_t)r * d.it.Tf * d.g.nb);
  y[(size_t)r * ld_y + m] = ola_gather(fr, 0, (size_t)2 * d.g.nb, d.w, m, n / H + 1, N, H);
}

size_t smooth_lds_bytes(int nf, int nt) {
  return (size_t)(kDenoiseTileT + 2 * nt) * (size_t)(2 * kDenoiseTileK + 2 * nf) * sizeof(float);
}

void launch_rows_fft(const FxDenoiseDev& d, const FxDenoiseRows& q, hipStream_t s) {
  if (q.R < 1) return;
  hipLaunchKernelGGL(denoise_fft_kernel, dim3((unsigned)q.Tf, (unsigned)q.R), dim3(256), (size_t)d.g.N * sizeof(float2), s, d.g, d.w,
                     d.tw, q);
}

void launch_rows_smooth(const FxDenoiseDev& d, const FxDenoiseRows& q, hipStream_t s) {
  if (q.R < 1) return;
  const dim3 grid((unsigned)cdiv64(d.g.nb, kDenoiseTileK), (unsigned)cdiv64(q.Tf, kDenoiseTileT), (unsigned)q.R);
  hipLaunchKernelGGL(denoise_smooth_kernel, grid, dim3(256), smooth_lds_bytes(d.nf, d.nt), s, d.g.nb, d.g.H, d.nf, d.nt, q);
}

}  // namespace

size_t fx_denoise_row_bytes(const FxStretchGeom& g, long Tf, int mode, bool item, bool want_b) {
  const size_t bins = (size_t)Tf * g.nb;
  if (!item) return bins * 8;
  return bins * (16 + (mode == 1 ? 8 : 0) + (want_b ? 8 : 0)) + (size_t)g.nb * 16;
}

void launch_denoise_analysis(const FxDenoiseDev& d, hipStream_t s, hipEvent_t* ev) {
  RVCX_CHECK(d.g.N <= 8192 && d.nf >= 0 && d.nf <= kDenoiseMaxNf && d.nt >= 0 && d.nt <= kDenoiseMaxNt, "denoise: geometry out of range");
  RVCX_CHECK(d.it.R <= 65535 && d.nz.R <= 65535 && cdiv64(std::max(d.it.Tf, d.nz.Tf), kDenoiseTileT) <= 65535,
             "denoise: more rows or frames than one launch takes");
  RVCX_CHECK(smooth_lds_bytes(d.nf, d.nt) <= 64 * 1024, "denoise: smoothing tile exceeds the LDS of a workgroup");
  launch_rows_fft(d, d.it, s);
  launch_rows_fft(d, d.nz, s);
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  launch_rows_smooth(d, d.it, s);
  launch_rows_smooth(d, d.nz, s);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
}

void launch_denoise_mask(const FxDenoiseDev& d, hipStream_t s, hipEvent_t* ev) {
  const dim3 lanes((unsigned)cdiv64(d.g.nb, 256), (unsigned)d.it.R), frames((unsigned)d.it.Tf, (unsigned)d.it.R);
  if (d.v.mode == 0) {
    hipLaunchKernelGGL(denoise_stats_kernel, lanes, dim3(256), 0, s, d);
    if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(denoise_mask0_kernel, frames, dim3(256), 0, s, d);
  } else {
    hipLaunchKernelGGL(denoise_floor_kernel, lanes, dim3(256), 0, s, d);
    if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  }
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
}

void launch_denoise_synthesis(const FxDenoiseDev& d, float* y, long ld_y, hipStream_t s, hipEvent_t* ev) {
  hipLaunchKernelGGL(denoise_ifft_kernel, dim3((unsigned)d.it.Tf, (unsigned)d.it.R), dim3(256), (size_t)d.g.N * sizeof(float2), s, d);
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(denoise_ola_kernel, dim3((unsigned)cdiv64(d.it.ld, 256), (unsigned)d.it.R), dim3(256), 0, s, d, y, ld_y);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------
void fx_denoise_smooth_host(const float* A2, long T, int nb, int nf, int nt, float* S) {
  std::vector<float> F((size_t)T * nb);
  for (long t = 0; t < T; ++t)
    for (int k = 0; k < nb; ++k) {
      const int lo = std::max(-nf, -k), hi = std::min(nf, nb - 1 - k);
      float s = 0.f;
      for (int dk = lo; dk <= hi; ++dk) {
        const float term = (float)(nf + 1 - std::abs(dk)) * A2[(size_t)t * nb + k + dk];
        s = s + term;
      }
      F[(size_t)t * nb + k] = s;
    }
  for (long t = 0; t < T; ++t) {
    const int lo = (int)std::max(-(long)nt, -t), hi = (int)std::min((long)nt, T - 1 - t);
    for (int k = 0; k < nb; ++k) {
      float s = 0.f;
      for (int dt = lo; dt <= hi; ++dt) {
        const float term = (float)(nt + 1 - std::abs(dt)) * F[(size_t)(t + dt) * nb + k];
        s = s + term;
      }
      S[(size_t)t * nb + k] = s / (float)(dn_weight_sum(t, T, nt) * dn_weight_sum(k, nb, nf));
    }
  }
}

namespace {

using cplx = std::complex<double>;

struct HostPlan {
  FxStretchGeom g;
  std::vector<float> w;
  std::vector<cplx> tw;
  explicit HostPlan(int sr) : g(fx_stretch_geom(sr)) {
    std::vector<float2> twf;
    fx_stretch_tables(g.N, w, twf);
    tw.resize((size_t)g.N / 2);
    for (int k = 0; k < g.N / 2; ++k) tw[k] = cplx(std::cos(2.0 * kPi * k / g.N), -std::sin(2.0 * kPi * k / g.N));
  }
};

// D (T, nb) float pairs and S (T, nb) of one signal
void analyse_host(const HostPlan& P, const float* x, long n, int nf, int nt, std::vector<float>& D, std::vector<float>& S) {
  const int N = P.g.N, H = P.g.H, nb = P.g.nb;
  const long T = fx_stretch_T(n, H);
  D.assign((size_t)T * nb * 2, 0.f);
  S.assign((size_t)T * nb, 0.f);
  std::vector<float> A2((size_t)T * nb);
  std::vector<cplx> buf((size_t)N);
  for (long t = 0; t < T; ++t) {
    for (int i = 0; i < N; ++i) {
      const long src = t * H - N / 2 + i;
      buf[i] = (src >= 0 && src < n) ? cplx((double)P.w[i] * (double)x[src], 0.0) : cplx(0.0, 0.0);
    }
    fft_host(buf, P.tw);
    for (int k = 0; k < nb; ++k) {
      const size_t at = (size_t)t * nb + k;
      const float re = (float)buf[k].real(), im = (float)buf[k].imag();
      D[at * 2] = re, D[at * 2 + 1] = im;
      const float rr = re * re, ii = im * im;
      A2[at] = rr + ii;
    }
  }
  fx_denoise_smooth_host(A2.data(), T, nb, nf, nt, S.data());
}

}  // namespace

void fx_denoise_host(const float* x, long n, const float* noise, long n_noise, int sr, const FxDenoiseValues& v, float* y,
                     float* D_out, float* S_out, double* mu_out, double* sd_out, double* b_out, float* m_out) {
  const HostPlan P(sr);
  const int N = P.g.N, H = P.g.H, nb = P.g.nb;
  const long T = fx_stretch_T(n, H);
  const int nf = (int)fx_denoise_nf(v.freq_smooth_hz, N, sr), nt = (int)fx_denoise_nt(v.time_smooth_ms, sr, H);
  std::vector<float> D, S, m((size_t)T * nb);
  analyse_host(P, x, n, nf, nt, D, S);
  if (v.mode == 0) {
    std::vector<float> Dn, Sn;
    if (noise) analyse_host(P, noise, n_noise, nf, nt, Dn, Sn);
    const std::vector<float>& Sp = noise ? Sn : S;
    const long Tp = noise ? fx_stretch_T(n_noise, H) : T;
    for (int k = 0; k < nb; ++k) {
      double mean = 0.0, var = 0.0;
      for (int pass = 0; pass < 2; ++pass) {
        double tot = 0.0;
        for (long c0 = 0; c0 < Tp; c0 += kDenoiseStatChunk) {
          double part = 0.0;
          for (long t = c0; t < std::min<long>(c0 + kDenoiseStatChunk, Tp); ++t) {
            const double l = (double)dn_level(Sp[(size_t)t * nb + k]);
            part += pass == 0 ? l : (l - mean) * (l - mean);
          }
          tot += part;
        }
        (pass == 0 ? mean : var) = tot / (double)Tp;
      }
      const double sd = std::sqrt(var);
      if (mu_out) mu_out[k] = mean;
      if (sd_out) sd_out[k] = sd;
      for (long t = 0; t < T; ++t) m[(size_t)t * nb + k] = dn_mask0(dn_level(S[(size_t)t * nb + k]), mean, sd, v.n_std, v.knee_db);
    }
  } else {
    const double c = fx_denoise_c(H, sr, v.time_constant_s), omc = 1.0 - c;
    std::vector<double> f((size_t)T);
    for (int k = 0; k < nb; ++k) {
      double run = (double)sqrtf(S[k]);
      for (long t = 0; t < T; ++t) {
        run = omc * (double)sqrtf(S[(size_t)t * nb + k]) + c * run;
        f[t] = run;
      }
      for (long t = T - 1; t >= 0; --t) {
        run = omc * f[t] + c * run;
        if (b_out) b_out[(size_t)t * nb + k] = run;
        m[(size_t)t * nb + k] = dn_mask1((double)sqrtf(S[(size_t)t * nb + k]), run, v.thresh_mult, v.slope);
      }
    }
  }
  if (D_out) std::copy(D.begin(), D.end(), D_out);
  if (S_out) std::copy(S.begin(), S.end(), S_out);
  if (m_out) std::copy(m.begin(), m.end(), m_out);
  // synthesis and overlap-add in double
  std::vector<double> num((size_t)n, 0.0), den((size_t)n, 0.0);
  std::vector<cplx> buf((size_t)N);
  for (long t = 0; t < T; ++t) {
    std::fill(buf.begin(), buf.end(), cplx(0.0, 0.0));
    for (int k = 0; k < nb; ++k) {
      const size_t at = (size_t)t * nb + k;
      const double gk = (double)dn_gain(v.strength, m[at]);
      const bool edge = k == 0 || k == N / 2;
      const cplx Y(gk * (double)D[at * 2], edge ? 0.0 : gk * (double)D[at * 2 + 1]);
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
