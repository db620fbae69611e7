// Formant shift and envelope transfer (include/rvcx.h stage 17).  Every step is continuous in the spectrum (a maximum, a
// linear warp, a clamp), so no decision can fall the other way between float32 and float64.
//
// Kernels (256 lanes; one row = one channel of one item):
//   formant_frame_kernel   one workgroup per frame, everything in LDS and registers (formant_device.h: fm_frame_body, shared with
//                          the live stage).  It writes the N windowed samples of the frame (and the taps when asked).
//   formant_ola_kernel     one lane per output sample (fft_device.h: ola_gather)
// LDS: the N float pairs of the transform, nothing else (64 KiB at N = 8192).
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
#include "formant_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;

__global__ __launch_bounds__(256) void formant_frame_kernel(const FxFormantDev d) {
  extern __shared__ float2 a[];
  const FxStretchGeom g = d.g;
  const int r = blockIdx.y, nb = g.nb;
  const long t = blockIdx.x, n = d.len[r];
  if (t >= n / g.H + 1) return;
  const bool with_src = d.src != nullptr && d.has_src[r] != 0;
  const size_t tbase = (size_t)t * nb;
  FmFrameTaps taps;
  if (r == 0) {
    if (d.taps.D) taps.D = d.taps.D + tbase;
    if (d.taps.E) taps.E = d.taps.E + tbase;
    if (d.taps.Es) taps.Es = d.taps.Es + tbase;
    if (d.taps.g) taps.g = d.taps.g + tbase;
    if (d.taps.s) taps.s = d.taps.s + t;
  }
  const FmFrameArgs q{g, d.v, d.nc, d.limit, d.w, d.tw};
  const long j0 = t * g.H - g.N / 2;
  const float* __restrict__ x = d.x + (size_t)r * d.ld;
  const float* __restrict__ xs = d.src ? d.src + (size_t)r * d.ld : nullptr;
  // sample i of frame t of a row: nothing in front of sample 0 or behind the row's last one
  auto own = [&](int i, float& v) {
    const long src = j0 + i;
    if (src < 0 || src >= n) return false;
    v = x[src];
    return true;
  };
  auto other = [&](int i, float& v) {
    const long src = j0 + i;
    if (src < 0 || src >= n) return false;
    v = xs[src];
    return true;
  };
  fm_frame_body<kFormantKpt, kFormantCpt, true>(a, q, own, other, with_src, taps, d.fr + ((size_t)r * d.Tf + t) * g.N);
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
