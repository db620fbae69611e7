// Live noise reduction (include/rvcx.h stage 16): stage 15's soft spectral gate made causal, so that a live-stream session can
// run it inside a step.  The time triangle covers the past side only, the adaptive floor runs forward only, and every sum is
// taken in ascending frame order from state the stream carries, so the result does not depend on how the signal is cut.
//
// Kernels (256 lanes):
//   dn_live_kernel        one workgroup per stream and step.  It moves the state into the set it writes, then takes the frames
//                         this step completes in order: window from the FIFO and the block, stage 13's transform in LDS, A2, the
//                         frequency triangle from LDS, the time triangle from the ring, floor or profile, mask and gain, the
//                         Hermitian spectrum, the transform again, the window, the sums.  Then it emits the block, divided by
//                         the window sum.  A lane owns the bins k = lane + 256 j: ring, floor and the frame's D never meet
//                         another lane.
//   dn_live_stats_kernel  mode 0 at open, one lane per bin: stage 15's statistics of the clip's level
// Bounds: a frame this step completes starts behind sample n0 - N and ends at or before n0 + B, so every index into the sums
// lies in 0 .. N + B - 1 and every sample read in the FIFO or the block (dn_live_step checks the frame range it hands over).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "common.h"
#include "denoise_live.h"

// A2, S, f, m and g are defined with every rounding written out
#pragma clang fp contract(off)

#include "denoise_device.h"
#include "fft_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;

struct DnLiveArgs {
  int N, H, nb, logN, nf, nt;
  DnLiveValues v;                      // mode 2: analysis alone (the noise clip at open): S is tapped, nothing else is formed
  long B, n0, c0, c1;                  // block, samples received before this step, frames [c0, c1) to take
  const float* x;
  long ldx;
  float* y;
  long ldy;
  const float* st_old;
  float* st_new;
  long per_stream, off_tail, off_ring, off_f;
  float* acc;
  const float* w;
  const float2* tw;
  const double* mu;
  const double* sd;
  DnLiveTaps taps;
};

// the weights of the frames t + dt, -nt <= dt <= 0, that exist
__host__ __device__ inline int dn_live_wt(long t, int nt) {
  const long lo = -(long)nt > -t ? -(long)nt : -t;
  int s = 0;
  for (long dt = lo; dt <= 0; ++dt) s += nt + 1 + (int)dt;
  return s;
}

__global__ __launch_bounds__(256) void dn_live_kernel(const DnLiveArgs q) {
  extern __shared__ float2 a[];                        // N pairs, then A2 of the frame (nb floats)
  const int N = q.N, H = q.H, nb = q.nb, logN = q.logN, nf = q.nf, nt = q.nt, tid = threadIdx.x;
  float* a2 = reinterpret_cast<float*>(a + N);
  const size_t s = blockIdx.x;
  const long B = q.B, n0 = q.n0;
  const float* __restrict__ so = q.st_old + s * q.per_stream;
  float* sn = q.st_new + s * q.per_stream;
  const float* __restrict__ x = q.x + s * q.ldx;
  float* acc = q.acc + s * (size_t)(N + B);
  float* ring = sn + q.off_ring;
  double* f = reinterpret_cast<double*>(sn + q.off_f);
  // sample j of the stream, n0 - N <= j < n0 + B: the FIFO holds the N samples in front of the block
  auto sample = [&](long j) -> float { return j < n0 ? so[j - (n0 - N)] : x[j - n0]; };

  // the state moves into the set this step writes
  for (long i = tid; i < N; i += 256) {
    sn[i] = sample(n0 + B - N + i);
    acc[i] = so[q.off_tail + i];
  }
  for (long i = tid; i < B; i += 256) acc[N + i] = 0.f;
  for (long i = tid; i < (long)nt * nb; i += 256) ring[i] = so[q.off_ring + i];
  {
    const double* fo = reinterpret_cast<const double*>(so + q.off_f);
    for (int k = tid; k < nb; k += 256) f[k] = fo[k];
  }
  __syncthreads();

  const float inv = 1.f / (float)N;
  for (long t = q.c0; t < q.c1; ++t) {
    const long j0 = t * H - N / 2;
    for (int i = tid; i < N; i += 256) {
      const float v = q.w[i] * sample(j0 + i);
      a[__brev((unsigned)i) >> (32 - logN)] = make_float2(v, 0.f);
    }
    fft_lds(a, q.tw, N, logN);
    float2 D[kDnLiveLaneBins];
#pragma unroll
    for (int j = 0; j < kDnLiveLaneBins; ++j) {
      const int k = tid + 256 * j;
      if (k < nb) {
        const float2 z = a[k];
        D[j] = z;
        a2[k] = __fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y));
      }
    }
    __syncthreads();
    const int wt_sum = dn_live_wt(t, nt);
    const int tlo = (int)(-(long)nt > -t ? -(long)nt : -t);
#pragma unroll
    for (int j = 0; j < kDnLiveLaneBins; ++j) {
      const int k = tid + 256 * j;
      if (k >= nb) continue;
      const int klo = max(-nf, -k), khi = min(nf, nb - 1 - k);
      float F = 0.f;
      for (int dk = klo; dk <= khi; ++dk) F = __fadd_rn(F, __fmul_rn((float)(nf + 1 - abs(dk)), a2[k + dk]));
      float sum = 0.f;
      for (int dt = tlo; dt < 0; ++dt)
        sum = __fadd_rn(sum, __fmul_rn((float)(nt + 1 + dt), ring[(size_t)((t + dt) % nt) * nb + k]));
      sum = __fadd_rn(sum, __fmul_rn((float)(nt + 1), F));
      if (nt > 0) ring[(size_t)(t % nt) * nb + k] = F;          // over frame t - nt, which this lane has just read
      const float Sv = sum / (float)(wt_sum * dn_weight_sum(k, nb, nf));
      const size_t tap = q.taps.T > 0 && t < q.taps.T ? (s * (size_t)q.taps.T + (size_t)t) * nb + k : 0;
      if (q.taps.S && t < q.taps.T) q.taps.S[tap] = Sv;
      if (q.v.mode == 2) continue;
      float m;
      if (q.v.mode == 1) {
        const double A = (double)sqrtf(Sv), fp = t == 0 ? A : f[k];
        const double c = A >= fp ? q.v.c_up : q.v.c_dn;
        const double fn = (1.0 - c) * A + c * fp;
        f[k] = fn;
        if (q.taps.f && t < q.taps.T) q.taps.f[tap] = fn;
        m = dn_mask1(A, fn, q.v.thresh_mult, q.v.slope);
      } else {
        m = dn_mask0(dn_level(Sv), q.mu[k], q.sd[k], q.v.n_std, q.v.knee_db);
      }
      if (q.taps.m && t < q.taps.T) q.taps.m[tap] = m;
      const float gk = dn_gain(q.v.strength, m);
      const bool edge = k == 0 || k == N / 2;                   // irfft ignores the imaginary part of the two real bins
      D[j] = make_float2(gk * D[j].x, edge ? 0.f : gk * D[j].y);
    }
    if (q.v.mode == 2) {
      __syncthreads();                                          // a2 is free for the next frame
      continue;
    }
    // x = Re(F(conj Y)) / N with the forward transform F: conj Y at k, Y at N - k.  Every a[k] was read in front of the barrier
    // above, and fft_lds opens with one.
#pragma unroll
    for (int j = 0; j < kDnLiveLaneBins; ++j) {
      const int k = tid + 256 * j;
      if (k >= nb) continue;
      a[__brev((unsigned)k) >> (32 - logN)] = make_float2(D[j].x, -D[j].y);
      if (k != 0 && k != N / 2) a[__brev((unsigned)(N - k)) >> (32 - logN)] = make_float2(D[j].x, D[j].y);
    }
    fft_lds(a, q.tw, N, logN);
    float* dst = acc + (j0 - n0 + N);
    for (int i = tid; i < N; i += 256) dst[i] = __fadd_rn(dst[i], (a[i].x * inv) * q.w[i]);
    __syncthreads();                                            // a is free, the sums are visible to the lanes of the next frame
  }

  if (q.v.mode == 2) return;
  for (long i = tid; i < B; i += 256) {
    const long j = n0 - N + i;
    float out = 0.f;
    if (j >= 0) out = q.v.strength == 0.f ? sample(j) : (float)((double)acc[i] / dn_live_den(q.w, j, N, H));
    q.y[s * q.ldy + i] = out;
  }
  for (int i = tid; i < N; i += 256) sn[q.off_tail + i] = acc[B + i];
}

__global__ __launch_bounds__(256) void dn_live_stats_kernel(const float* __restrict__ S, const long Tp, const int nb,
                                                            double* __restrict__ mu, double* __restrict__ sd) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  S += k;
  double tot = 0.0;
  for (long c0 = 0; c0 < Tp; c0 += kDnLiveStatChunk) {
    double part = 0.0;
    for (long t = c0; t < min(c0 + (long)kDnLiveStatChunk, Tp); ++t) part += (double)dn_level(S[(size_t)t * nb]);
    tot += part;
  }
  const double mean = tot / (double)Tp;
  tot = 0.0;
  for (long c0 = 0; c0 < Tp; c0 += kDnLiveStatChunk) {
    double part = 0.0;
    for (long t = c0; t < min(c0 + (long)kDnLiveStatChunk, Tp); ++t) {
      const double e = (double)dn_level(S[(size_t)t * nb]) - mean;
      part += e * e;
    }
    tot += part;
  }
  mu[k] = mean;
  sd[k] = sqrt(tot / (double)Tp);
}

}  // namespace

void dn_live_layout(DnLive& d) {
  const long N = d.g.N, nb = d.g.nb;
  d.off_tail = N;
  d.off_ring = 2 * N;
  d.off_f = 2 * N + (((long)d.nt * nb + 1) & ~1L);      // doubles: an even number of floats from an 8-byte aligned start
  d.per_stream = d.off_f + 2 * nb;                      // (even: every stream's f is aligned too)
}

void dn_live_step(const DnLive& d, const float* x, long ldx, int cur, uint64_t step, float* y, long ldy, hipStream_t s,
                  const DnLiveTaps* taps) {
  const int N = d.g.N, H = d.g.H;
  RVCX_CHECK(d.S >= 1 && d.S <= 65535 && d.B >= 1, "denoise_live: streams or block out of range");
  RVCX_CHECK(N >= 512 && N <= 4096 && d.g.nb <= 256 * kDnLiveLaneBins && d.nf >= 0 && d.nf <= kDnLiveMaxNf && d.nt >= 0 &&
                 d.nt <= kDnLiveMaxNt,
             "denoise_live: geometry out of range");
  RVCX_CHECK(step <= (uint64_t)(((int64_t)1 << 62) / d.B), "denoise_live: the sample index leaves 2^62");
  RVCX_CHECK(d.v.mode == 1 || d.v.mode == 2 || (d.v.mode == 0 && d.mu && d.sd), "denoise_live: mode 0 without a profile");
  DnLiveArgs q{};
  q.N = N, q.H = H, q.nb = d.g.nb, q.logN = d.g.logN, q.nf = d.nf, q.nt = d.nt, q.v = d.v;
  q.B = d.B, q.n0 = (long)step * d.B;
  q.c0 = dn_live_frames(q.n0, N, H), q.c1 = dn_live_frames(q.n0 + d.B, N, H);
  // what the kernel's indices rest on: frame c0 starts behind n0 - N, frame c1 - 1 ends at or before n0 + B
  RVCX_CHECK(q.c1 >= q.c0 && (q.c1 == q.c0 || (q.c0 * H - N / 2 > q.n0 - N && (q.c1 - 1) * H + N / 2 <= q.n0 + d.B)),
             "denoise_live: frame range");
  q.x = x, q.ldx = ldx, q.y = y, q.ldy = ldy;
  q.st_old = d.state[cur], q.st_new = d.state[cur ^ 1];
  q.per_stream = d.per_stream, q.off_tail = d.off_tail, q.off_ring = d.off_ring, q.off_f = d.off_f;
  q.acc = d.acc, q.w = d.w, q.tw = d.tw, q.mu = d.mu, q.sd = d.sd;
  if (taps) q.taps = *taps;
  const size_t lds = (size_t)N * sizeof(float2) + (size_t)d.g.nb * sizeof(float);
  hipLaunchKernelGGL(dn_live_kernel, dim3((unsigned)d.S), dim3(256), lds, s, q);
}

void launch_dn_live_stats(const float* S, long Tp, int nb, double* mu, double* sd, hipStream_t s) {
  RVCX_CHECK(Tp >= 1 && nb >= 1, "denoise_live: a profile needs a frame");
  hipLaunchKernelGGL(dn_live_stats_kernel, dim3((unsigned)cdiv64(nb, 256)), dim3(256), 0, s, S, Tp, nb, mu, sd);
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------
namespace {

using cplx = std::complex<double>;

struct HostTables {
  FxStretchGeom g;
  std::vector<float> w;
  std::vector<cplx> tw;
  explicit HostTables(int sr) : g(dn_live_geom(sr)) {
    std::vector<float2> twf;
    fx_stretch_tables(g.N, w, twf);
    tw.resize((size_t)g.N / 2);
    for (int k = 0; k < g.N / 2; ++k) tw[k] = cplx(std::cos(2.0 * kPi * k / g.N), -std::sin(2.0 * kPi * k / g.N));
  }
};

// D (T, nb) float pairs and S (T, nb) of the T frames complete in x[0 .. n)
void analyse_live_host(const HostTables& P, const float* x, long n, int nf, int nt, std::vector<float>& D, std::vector<float>& S) {
  const int N = P.g.N, H = P.g.H, nb = P.g.nb;
  const long T = dn_live_frames(n, N, H);
  D.assign((size_t)T * nb * 2, 0.f);
  S.assign((size_t)T * nb, 0.f);
  std::vector<float> F((size_t)T * nb);
  std::vector<cplx> buf((size_t)N);
  for (long t = 0; t < T; ++t) {
    for (int i = 0; i < N; ++i) {
      const long src = t * H - N / 2 + i;
      buf[i] = src >= 0 ? cplx((double)P.w[i] * (double)x[src], 0.0) : cplx(0.0, 0.0);
    }
    fft_host(buf, P.tw);
    std::vector<float> A2((size_t)nb);
    for (int k = 0; k < nb; ++k) {
      const size_t at = (size_t)t * nb + k;
      const float re = (float)buf[k].real(), im = (float)buf[k].imag();
      D[at * 2] = re, D[at * 2 + 1] = im;
      const float rr = re * re, ii = im * im;
      A2[k] = rr + ii;
    }
    for (int k = 0; k < nb; ++k) {
      const int lo = std::max(-nf, -k), hi = std::min(nf, nb - 1 - k);
      float s = 0.f;
      for (int dk = lo; dk <= hi; ++dk) {
        const float term = (float)(nf + 1 - std::abs(dk)) * A2[k + dk];
        s = s + term;
      }
      F[(size_t)t * nb + k] = s;
    }
    const int lo = (int)std::max(-(long)nt, -t), wt = dn_live_wt(t, nt);
    for (int k = 0; k < nb; ++k) {
      float s = 0.f;
      for (int dt = lo; dt <= 0; ++dt) {
        const float term = (float)(nt + 1 + dt) * F[(size_t)(t + dt) * nb + k];
        s = s + term;
      }
      S[(size_t)t * nb + k] = s / (float)(wt * dn_weight_sum(k, nb, nf));
    }
  }
}

}  // namespace

void dn_live_profile_host(const float* clip, long n, const DnLiveHostPlan& P, double* mu, double* sd) {
  const HostTables Tb(P.sr);
  const int nb = Tb.g.nb;
  std::vector<float> D, S;
  analyse_live_host(Tb, clip, n, P.nf, P.nt, D, S);
  const long Tp = dn_live_frames(n, Tb.g.N, Tb.g.H);
  for (int k = 0; k < nb; ++k) {
    double mean = 0.0, var = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      double tot = 0.0;
      for (long c0 = 0; c0 < Tp; c0 += kDnLiveStatChunk) {
        double part = 0.0;
        for (long t = c0; t < std::min<long>(c0 + kDnLiveStatChunk, Tp); ++t) {
          const double l = (double)dn_level(S[(size_t)t * nb + k]);
          part += pass == 0 ? l : (l - mean) * (l - mean);
        }
        tot += part;
      }
      (pass == 0 ? mean : var) = tot / (double)Tp;
    }
    mu[k] = mean;
    sd[k] = std::sqrt(var);
  }
}

void dn_live_host(const float* x, long n, const DnLiveHostPlan& P, const double* mu, const double* sd, float* y, float* D_out,
                  float* S_out, double* f_out, float* m_out) {
  const HostTables Tb(P.sr);
  const int N = Tb.g.N, H = Tb.g.H, nb = Tb.g.nb;
  const long T = dn_live_frames(n, N, H);
  const DnLiveValues& v = P.v;
  std::vector<float> D, S, m((size_t)T * nb);
  analyse_live_host(Tb, x, n, P.nf, P.nt, D, S);
  if (v.mode == 0) {
    for (long t = 0; t < T; ++t)
      for (int k = 0; k < nb; ++k) m[(size_t)t * nb + k] = dn_mask0(dn_level(S[(size_t)t * nb + k]), mu[k], sd[k], v.n_std, v.knee_db);
  } else {
    for (int k = 0; k < nb; ++k) {
      double run = 0.0;
      for (long t = 0; t < T; ++t) {
        const double A = (double)sqrtf(S[(size_t)t * nb + k]), fp = t == 0 ? A : run;
        const double c = A >= fp ? v.c_up : v.c_dn;
        run = (1.0 - c) * A + c * fp;
        if (f_out) f_out[(size_t)t * nb + k] = run;
        m[(size_t)t * nb + k] = dn_mask1(A, run, v.thresh_mult, v.slope);
      }
    }
  }
  if (D_out) std::copy(D.begin(), D.end(), D_out);
  if (S_out) std::copy(S.begin(), S.end(), S_out);
  if (m_out) std::copy(m.begin(), m.end(), m_out);
  for (long i = 0; i < std::min<long>(n, N); ++i) y[i] = 0.f;
  if (v.strength == 0.f) {                                  // the delayed input, bit for bit
    for (long i = N; i < n; ++i) y[i] = x[i - N];
    return;
  }
  // synthesis and overlap-add in double; sample j leaves at j + N, once every frame that covers it is complete
  std::vector<double> num((size_t)n, 0.0);
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
    fft_host(buf, Tb.tw);
    for (int i = 0; i < N; ++i) {
      const long j = t * H - N / 2 + i;
      if (j < 0 || j >= n) continue;
      num[j] += (double)Tb.w[i] * (buf[i].real() / N);
    }
  }
  for (long j = 0; j + N < n; ++j) y[j + N] = (float)(num[j] / dn_live_den(Tb.w.data(), j, N, H));
}

}  // namespace rvcx
