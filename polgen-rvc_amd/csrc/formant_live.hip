// Live formant shift (include/rvcx.h stage 19): stage 17 without a source on stage 16's causal grid.  A frame depends on its own
// N samples alone, so the frames a step completes do not wait for one another: they run side by side, one workgroup each, and a
// second launch adds them to the sums in ascending frame order.  (Stage 16 walks its frames inside one workgroup because its
// floor is a recurrence; here that would put 2 (iterations + 1) + 2 dependent transforms per frame on the path of a step.)
//
// Kernels (256 lanes):
//   fm_live_frames_kernel  grid (frames the step completes, S).  One frame through stage 17's chain (formant_device.h) in LDS and
//                          registers, instantiated for N <= 4096; its samples come from the FIFO of the set being read or from
//                          the block.  It writes the N windowed samples of the frame into the step's scratch.
//   fm_live_finish_kernel  one workgroup per stream.  A lane owns the positions p = lane + 256 m of the N + B sums of the step: the
//                          old tail, plus the step's frames that cover p in ascending t, in float32.  It emits the block (divided
//                          by the window sum, or the delayed input when the stage is off), writes the new tail and moves the FIFO
//                          into the set being written.  No position meets another lane: no barrier, no atomics.
// Bounds: a frame this step completes starts behind sample n0 - N and ends at or before n0 + B, so every sample read lies in the
// FIFO or the block, and there are at most B / H + 1 of them (fm_live_step checks the frame range it hands over).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "common.h"
#include "formant_live.h"

// A2, eps, L, W, g and the energy terms are defined with every rounding written out
#pragma clang fp contract(off)

#include "fft_device.h"
#include "formant_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;

struct FmLiveArgs {
  FmFrameArgs q;
  long B, n0, c0, c1, slots;             // block, samples received before this step, frames [c0, c1), frames of scratch per stream
  int off;
  const float* x;
  long ldx;
  float* y;
  long ldy;
  const float* st_old;
  float* st_new;
  float* fr;
  FmLiveTaps taps;
};

// sample j of stream s, n0 - N <= j < n0 + B: the FIFO holds the N samples in front of the block (zeros in front of sample 0)
__device__ __forceinline__ float fm_live_sample(const FmLiveArgs& p, const float* __restrict__ so, const float* __restrict__ x,
                                                long j) {
  return j < p.n0 ? so[j - (p.n0 - p.q.g.N)] : x[j - p.n0];
}

__global__ __launch_bounds__(256) void fm_live_frames_kernel(const FmLiveArgs p) {
  extern __shared__ float2 a[];                        // N pairs
  const int N = p.q.g.N, nb = p.q.g.nb;
  const size_t s = blockIdx.y;
  const long f = blockIdx.x, t = p.c0 + f;
  if (t >= p.c1) return;
  const float* __restrict__ so = p.st_old + s * (size_t)(2 * N);
  const float* __restrict__ x = p.x + s * p.ldx;
  const long j0 = t * p.q.g.H - N / 2;
  auto sample = [&](int i, float& v) {
    v = fm_live_sample(p, so, x, j0 + i);
    return true;
  };
  FmFrameTaps taps;
  if (t < p.taps.T) {
    const size_t at = s * (size_t)p.taps.T + (size_t)t;
    if (p.taps.E) taps.E = p.taps.E + at * nb;
    if (p.taps.g) taps.g = p.taps.g + at * nb;
    if (p.taps.s) taps.s = p.taps.s + at;
  }
  fm_frame_body<kFmLiveKpt, kFmLiveCpt, false>(a, p.q, sample, sample, false, taps, p.fr + (s * (size_t)p.slots + (size_t)f) * N);
}

__global__ __launch_bounds__(256) void fm_live_finish_kernel(const FmLiveArgs p) {
  const int N = p.q.g.N, H = p.q.g.H, tid = threadIdx.x;
  const size_t s = blockIdx.x;
  const long B = p.B, n0 = p.n0;
  const float* __restrict__ so = p.st_old + s * (size_t)(2 * N);
  float* sn = p.st_new + s * (size_t)(2 * N);
  const float* __restrict__ x = p.x + s * p.ldx;
  const float* __restrict__ fr = p.fr + s * (size_t)p.slots * N;

  for (long i = tid; i < N; i += 256) sn[i] = fm_live_sample(p, so, x, n0 + B - N + i);
  for (long pos = tid; pos < N + B; pos += 256) {
    const long j = n0 - N + pos;                       // the sample this sum belongs to
    float v = pos < N ? so[N + pos] : 0.f;
    // the step's frames that cover j: 0 <= j + N / 2 - t H < N, in ascending t
    long t = p.c0;
    if (j - N / 2 + 1 > p.c0 * H) t = (j - N / 2 + H) / H;
    for (; t < p.c1; ++t) {
      const long i = j + N / 2 - t * H;
      if (i < 0) break;
      if (i >= N) continue;                            // (never: the start above)
      v = __fadd_rn(v, fr[(size_t)(t - p.c0) * N + i]);
    }
    if (pos < B) {
      float out = 0.f;
      if (j >= 0) out = p.off ? fm_live_sample(p, so, x, j) : (float)((double)v / dn_live_den(p.q.w, j, N, H));
      p.y[s * p.ldy + pos] = out;
    } else {
      sn[N + pos - B] = v;
    }
  }
}

}  // namespace

void fm_live_step(const FmLive& d, const float* x, long ldx, int cur, uint64_t step, float* y, long ldy, hipStream_t s,
                  const FmLiveTaps* taps) {
  const int N = d.g.N, H = d.g.H;
  RVCX_CHECK(d.S >= 1 && d.S <= 65535 && d.B >= 1, "formant_live: streams or block out of range");
  RVCX_CHECK(N >= 512 && N <= 4096 && d.g.nb <= 256 * kFmLiveKpt && H * 4 == N, "formant_live: geometry out of range");
  RVCX_CHECK(d.nc >= 1 && d.nc <= N / 8 && d.nc < 256 * kFmLiveCpt, "formant_live: quefrency out of range");
  RVCX_CHECK(d.v.iterations >= 0 && d.v.iterations <= kFormantMaxIter, "formant_live: iterations out of range");
  RVCX_CHECK(step <= (uint64_t)(((int64_t)1 << 62) / d.B), "formant_live: the sample index leaves 2^62");
  FmLiveArgs p{};
  p.q = FmFrameArgs{d.g, d.v, d.nc, fx_formant_limit(d.v.max_gain_db), d.w, d.tw};
  p.B = d.B, p.n0 = (long)step * d.B, p.slots = fm_live_slots(d), p.off = fm_live_off(d.v) ? 1 : 0;
  p.c0 = dn_live_frames(p.n0, N, H), p.c1 = dn_live_frames(p.n0 + d.B, N, H);
  // what the kernels' indices rest on: frame c0 starts behind n0 - N, frame c1 - 1 ends at or before n0 + B, and the step's
  // frames fit the scratch
  RVCX_CHECK(p.c1 >= p.c0 && p.c1 - p.c0 < p.slots &&
                 (p.c1 == p.c0 || (p.c0 * H - N / 2 > p.n0 - N && (p.c1 - 1) * H + N / 2 <= p.n0 + d.B)),
             "formant_live: frame range");
  p.x = x, p.ldx = ldx, p.y = y, p.ldy = ldy;
  p.st_old = d.state[cur], p.st_new = d.state[cur ^ 1], p.fr = d.fr;
  if (taps) p.taps = *taps;
  if (p.c1 > p.c0)
    hipLaunchKernelGGL(fm_live_frames_kernel, dim3((unsigned)(p.c1 - p.c0), (unsigned)d.S), dim3(256), (size_t)N * sizeof(float2), s,
                       p);
  hipLaunchKernelGGL(fm_live_finish_kernel, dim3((unsigned)d.S), dim3(256), 0, s, p);
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------
void fm_live_host(const float* x, long n, int sr, const FxFormantValues& v, float* y, float* D_out, float* E_out, float* g_out,
                  float* s_out) {
  using cplx = std::complex<double>;
  const FxStretchGeom G = dn_live_geom(sr);
  const int N = G.N, H = G.H, nb = G.nb;
  std::vector<float> w;
  std::vector<cplx> tw((size_t)N / 2);
  {
    std::vector<float2> twf;
    fx_stretch_tables(N, w, twf);
    for (int k = 0; k < N / 2; ++k) tw[k] = cplx(std::cos(2.0 * kPi * k / N), -std::sin(2.0 * kPi * k / N));
  }
  const long T = dn_live_frames(n, N, H);
  const int nc = (int)fx_formant_nc(v.quefrency_ms, sr);
  const double limit = fx_formant_limit(v.max_gain_db);
  std::vector<float> D((size_t)nb * 2), A2((size_t)nb), L((size_t)nb), E((size_t)nb), g((size_t)nb);
  std::vector<double> num((size_t)n, 0.0);
  std::vector<cplx> buf((size_t)N);
  for (long t = 0; t < T; ++t) {
    for (int i = 0; i < N; ++i) {
      const long src = t * H - N / 2 + i;
      buf[i] = src >= 0 ? cplx((double)w[i] * (double)x[src], 0.0) : cplx(0.0, 0.0);
    }
    fft_host(buf, tw);
    float top = 0.f;
    for (int k = 0; k < nb; ++k) {
      D[2 * k] = (float)buf[k].real(), D[2 * k + 1] = (float)buf[k].imag();
      A2[k] = fm_a2(D[2 * k], D[2 * k + 1]);
      top = std::max(top, A2[k]);
    }
    const float eps = fm_eps(top);
    for (int k = 0; k < nb; ++k) L[k] = fm_log(A2[k], eps);
    fx_formant_envelope_host(L.data(), N, nc, v.iterations, E.data());
    double part0[256] = {0}, part1[256] = {0};
    for (int k = 0; k < nb; ++k) {
      const float W = fm_warp([&](int i) { return E[(size_t)i]; }, k, nb, (double)v.ratio);
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
    fft_host(buf, tw);
    for (int i = 0; i < N; ++i) {
      const long j = t * H - N / 2 + i;
      if (j < 0 || j >= n) continue;
      num[j] += (double)w[i] * (buf[i].real() / N);
    }
  }
  for (long i = 0; i < std::min<long>(n, N); ++i) y[i] = 0.f;
  if (fm_live_off(v)) {                                     // the delayed input, bit for bit
    for (long i = N; i < n; ++i) y[i] = x[i - N];
    return;
  }
  // sample j leaves at j + N, once every frame that covers it is complete
  for (long j = 0; j + N < n; ++j) y[j + N] = (float)(num[j] / dn_live_den(w.data(), j, N, H));
}

}  // namespace rvcx
