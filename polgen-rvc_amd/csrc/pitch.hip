// Time stretch and pitch shift (include/rvcx.h stages 13 and 14): a phase-locked vocoder whose frame-to-frame recurrence runs
// on integer phases (units of 2^-32 turn), so that it is an exact, associative scan -- chunk, segment, batch and grouping
// change no bit.
//
// Kernels (256 lanes unless noted; one row = one channel of one item in blockIdx.y):
//   stretch_fft_kernel      one workgroup per analysis frame: window, N-point radix-2 transform in LDS (bit-reversed load,
//                           twiddles from the host's double table), epilogue D, A2 (no fma), TH
//   stretch_own_kernel      one wave per frame: peak flags, nearest peak below and above by a segmented scan over 64 lanes
//   stretch_compose_kernel  one workgroup per chunk of output frames: the chunk's maps R -> R o par + off composed in LDS
//   stretch_carry_kernel    one workgroup per row: chunk prefixes from the segment's first R, sequentially over chunks
//   stretch_apply_kernel    one workgroup per chunk: R_j of every frame from the chunk's prefix
//   stretch_ifft_kernel     one workgroup per output frame: M_j, the angle, the Hermitian spectrum, the same transform, window
//   stretch_ola_kernel      one lane per output sample: the frames that cover it in ascending j, divided by the window sum
// Every index is bounded by the row's own T and J (formed from len[r] in the kernel): frames T and T + 1 are written as zero
// frames with own = identity, and a step j -> j + 1 is taken only while j + 1 < J, so t_{j+1} <= T - 1 and t_j + 1 <= T.
#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstring>

#include "common.h"
#include "pitch.h"

// A2 and M are defined with every rounding written out
#pragma clang fp contract(off)

#include "fft_device.h"

namespace rvcx {

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxNb = 4097;

__device__ __forceinline__ long row_T(const FxStretchDev& d, int r) { return (long)d.len[r] / d.g.H + 1; }
__device__ __forceinline__ long row_J(const FxStretchDev& d, long T) { return (T * d.P + d.Q - 1) / d.Q; }

__global__ __launch_bounds__(256) void stretch_fft_kernel(const FxStretchDev d, const float* __restrict__ rows) {
  extern __shared__ float2 a[];
  const int r = blockIdx.y, N = d.g.N, H = d.g.H, nb = d.g.nb, logN = d.g.logN;
  const long t = blockIdx.x, n = d.len[r], T = n / H + 1;
  if (t >= T + 2) return;
  const size_t base = ((size_t)r * d.Tf + t) * nb;
  if (t >= T) {                              // frames T and T + 1 are all zero
    for (int k = threadIdx.x; k < nb; k += 256) {
      if (d.D) d.D[base + k] = make_float2(0.f, 0.f);
      d.A2[base + k] = 0.f;
      d.TH[base + k] = 0u;
    }
    return;
  }
  const float* __restrict__ x = rows + (size_t)r * d.ld;
  for (int i = threadIdx.x; i < N; i += 256) {
    const long src = t * H - N / 2 + i;
    const float v = (src >= 0 && src < n) ? d.w[i] * x[src] : 0.f;
    a[__brev((unsigned)i) >> (32 - logN)] = make_float2(v, 0.f);
  }
  fft_lds(a, d.tw, N, logN);
  for (int k = threadIdx.x; k < nb; k += 256) {
    const float2 z = a[k];
    const float a2 = __fadd_rn(__fmul_rn(z.x, z.x), __fmul_rn(z.y, z.y));
    if (d.D) d.D[base + k] = z;
    d.A2[base + k] = a2;
    d.TH[base + k] = a2 == 0.f ? 0u : (uint32_t)(int64_t)rint((double)atan2f(z.y, z.x) * (2147483648.0 / kPi));
  }
}

__global__ __launch_bounds__(64) void stretch_own_kernel(const FxStretchDev d) {
  __shared__ float a2[kMaxNb];
  __shared__ int lo_s[kMaxNb];
  __shared__ int s_last[64], s_first[64];
  const int r = blockIdx.y, nb = d.g.nb, lane = threadIdx.x;
  const long t = blockIdx.x;
  if (t >= row_T(d, r) + 2) return;
  const size_t base = ((size_t)r * d.Tf + t) * nb;
  for (int k = lane; k < nb; k += 64) a2[k] = d.A2[base + k];
  __syncthreads();
  auto peak = [&](int k) {                   // a neighbour outside 0 .. nb - 1 counts as smaller
    const float v = a2[k];
    return v > 0.f && (k < 1 || v > a2[k - 1]) && (k < 2 || v > a2[k - 2]) && (k + 1 >= nb || v >= a2[k + 1]) &&
           (k + 2 >= nb || v >= a2[k + 2]);
  };
  const int seg = (nb + 63) / 64, k0 = min(nb, lane * seg), k1 = min(nb, k0 + seg);
  int last = -1, first = INT_MAX;
  for (int k = k0; k < k1; ++k)
    if (peak(k)) {
      last = k;
      if (first == INT_MAX) first = k;
    }
  s_last[lane] = last, s_first[lane] = first;
  __syncthreads();
  int run = -1, above = INT_MAX;
  for (int l = 0; l < lane; ++l) run = max(run, s_last[l]);
  for (int l = lane + 1; l < 64; ++l) above = min(above, s_first[l]);
  for (int k = k0; k < k1; ++k) {            // the nearest peak at or below k
    if (peak(k)) run = k;
    lo_s[k] = run;
  }
  for (int k = k1 - 1; k >= k0; --k) {       // the nearest peak at or above k; equal distance: the lower one
    if (peak(k)) above = k;
    const int lo = lo_s[k];
    int o;
    if (lo < 0) o = above == INT_MAX ? k : above;
    else o = (above == INT_MAX || k - lo <= above - k) ? lo : above;
    d.own[base + k] = o;
  }
}

// the map of step j -> j + 1 at bin k: R_{j+1}[k] = R_j[q] + dl
struct StretchStep {
  const int* own_j;          // own[t_j]
  const int* own_j1;         // own[t_{j+1}]
  const uint32_t* th_a;      // TH[t_j + 1]
  const uint32_t* th_b;      // TH[t_{j+1}]
  __device__ __forceinline__ StretchStep(const FxStretchDev& d, int r, long j) {
    const long tj = j * d.Q / d.P, tj1 = (j + 1) * d.Q / d.P;
    const size_t row = (size_t)r * d.Tf * d.g.nb;
    own_j = d.own + row + (size_t)tj * d.g.nb;
    own_j1 = d.own + row + (size_t)tj1 * d.g.nb;
    th_a = d.TH + row + (size_t)(tj + 1) * d.g.nb;
    th_b = d.TH + row + (size_t)tj1 * d.g.nb;
  }
  __device__ __forceinline__ void at(int k, int& q, uint32_t& dl) const {
    const int p = own_j1[k];
    q = own_j[p];
    dl = th_a[p] - th_b[p];
  }
};

__global__ __launch_bounds__(256) void stretch_compose_kernel(const FxStretchDev d, long s0) {
  __shared__ int par_s[kMaxNb];
  __shared__ uint32_t off_s[kMaxNb];
  const int r = blockIdx.y, c = blockIdx.x, nb = d.g.nb, nch = gridDim.x;
  const long J = row_J(d, row_T(d, r));
  const long j0 = s0 + (long)c * d.Lc, j1 = min(j0 + d.Lc, s0 + d.S);
  for (int k = threadIdx.x; k < nb; k += 256) par_s[k] = k, off_s[k] = 0u;
  __syncthreads();
  for (long j = j0; j < j1 && j + 1 < J; ++j) {
    const StretchStep st(d, r, j);
    int np[kStretchKpt];
    uint32_t no[kStretchKpt];
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) {
        int q;
        uint32_t dl;
        st.at(k, q, dl);
        np[i] = par_s[q], no[i] = off_s[q] + dl;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) par_s[k] = np[i], off_s[k] = no[i];
    }
    __syncthreads();
  }
  const size_t o = ((size_t)r * nch + c) * nb;
  for (int k = threadIdx.x; k < nb; k += 256) d.par[o + k] = par_s[k], d.off[o + k] = off_s[k];
}

__global__ __launch_bounds__(256) void stretch_carry_kernel(const FxStretchDev d, int nch) {
  __shared__ uint32_t cur[kMaxNb];
  const int r = blockIdx.x, nb = d.g.nb;
  uint32_t* rs = d.Rstart + (size_t)r * (nch + 1) * nb;
  for (int k = threadIdx.x; k < nb; k += 256) rs[k] = cur[k] = d.Rcarry[(size_t)r * nb + k];
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const size_t o = ((size_t)r * nch + c) * nb;
    uint32_t v[kStretchKpt];
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) v[i] = cur[d.par[o + k]] + d.off[o + k];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) rs[(size_t)(c + 1) * nb + k] = cur[k] = v[i];
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < nb; k += 256) d.Rcarry[(size_t)r * nb + k] = cur[k];
}

__global__ __launch_bounds__(256) void stretch_apply_kernel(const FxStretchDev d, long s0) {
  __shared__ uint32_t cur[kMaxNb];
  const int r = blockIdx.y, c = blockIdx.x, nb = d.g.nb, nch = gridDim.x;
  const long J = row_J(d, row_T(d, r));
  const long j0 = s0 + (long)c * d.Lc, j1 = min(j0 + d.Lc, s0 + d.S);
  const uint32_t* rs = d.Rstart + ((size_t)r * (nch + 1) + c) * nb;
  for (int k = threadIdx.x; k < nb; k += 256) cur[k] = rs[k];
  __syncthreads();
  for (long j = j0; j < j1 && j < J; ++j) {
    uint32_t* out = d.Rseg + ((size_t)r * d.S + (j - s0)) * nb;
    for (int k = threadIdx.x; k < nb; k += 256) out[k] = cur[k];
    if (!(j + 1 < j1 && j + 1 < J)) break;
    const StretchStep st(d, r, j);
    uint32_t v[kStretchKpt];
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) {
        int q;
        uint32_t dl;
        st.at(k, q, dl);
        v[i] = cur[q] + dl;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kStretchKpt; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nb) cur[k] = v[i];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void stretch_ifft_kernel(const FxStretchDev d, long s0) {
  extern __shared__ float2 a[];
  const int r = blockIdx.y, N = d.g.N, nb = d.g.nb, logN = d.g.logN;
  const long j = s0 + blockIdx.x;
  if (j >= row_J(d, row_T(d, r))) return;
  const long jq = j * d.Q, tj = jq / d.P;
  const float f = (float)((double)(jq - tj * d.P) / (double)d.P), omf = 1.f - f;
  const size_t base = ((size_t)r * d.Tf + tj) * nb;
  const uint32_t* __restrict__ Rj = d.Rseg + ((size_t)r * d.S + blockIdx.x) * nb;
  for (int k = threadIdx.x; k < nb; k += 256) {
    const float M = __fadd_rn(__fmul_rn(omf, sqrtf(d.A2[base + k])), __fmul_rn(f, sqrtf(d.A2[base + nb + k])));
    const uint32_t phi = Rj[k] + d.TH[base + k];
    float sn, cs;
    sincospif((float)(int32_t)phi * 4.656612873077393e-10f, &sn, &cs);      // (int32) phi / 2^31 half turns
    const bool edge = k == 0 || k == N / 2;           // irfft ignores the imaginary part of the two real bins
    const float re = M * cs, im = edge ? 0.f : M * sn;
    // x = Re(F(conj X)) / N with the forward transform F: conj X at k, X at N - k
    a[__brev((unsigned)k) >> (32 - logN)] = make_float2(re, -im);
    if (!edge) a[__brev((unsigned)(N - k)) >> (32 - logN)] = make_float2(re, im);
  }
  fft_lds(a, d.tw, N, logN);
  float* out = d.fr + ((size_t)r * (d.S + 3) + blockIdx.x + 3) * N;
  const float inv = 1.f / (float)N;
  for (int i = threadIdx.x; i < N; i += 256) out[i] = (a[i].x * inv) * d.w[i];
}

__global__ __launch_bounds__(256) void stretch_ola_kernel(const FxStretchDev d, long s0, float* __restrict__ y, long ld_y) {
  const int r = blockIdx.y, N = d.g.N, H = d.g.H;
  const long n = d.len[r], J = row_J(d, n / H + 1), ns = (n * d.P + d.Q / 2) / d.Q, s1 = s0 + d.S;
  if (s0 > 0 && s0 >= J) return;                      // the row ended in an earlier segment
  // the segment completes the samples [s0 H - N/2, s1 H - N/2), the row's last segment everything up to ns; with segments
  // shorter than two frames the lower end lies below sample 0 and is clamped (those samples do not exist)
  const long m = max(0L, s0 * H - N / 2) + (long)blockIdx.x * 256 + threadIdx.x;
  const long m1 = s1 >= J ? ns : min(ns, s1 * H - N / 2);
  if (m < 0 || m >= m1) return;
  y[(size_t)r * ld_y + m] = ola_gather(d.fr + (size_t)r * (d.S + 3) * N, 3 - s0, (size_t)N, d.w, m, J, N, H);
}

}  // namespace

long fx_pitch_P(int sr, double semitones) { return (long)std::floor((double)sr * std::pow(2.0, semitones / 12.0) + 0.5); }

void fx_stretch_tables(int N, std::vector<float>& w, std::vector<float2>& tw) {
  w.resize((size_t)N);
  tw.resize((size_t)N / 2);
  for (int i = 0; i < N; ++i) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * i / N));
  for (int k = 0; k < N / 2; ++k) tw[k] = make_float2((float)std::cos(2.0 * kPi * k / N), (float)-std::sin(2.0 * kPi * k / N));
}

size_t fx_stretch_row_bytes(const FxStretchGeom& g, long Tf, int S, int Lc, bool want_D) {
  const size_t nb = (size_t)g.nb, nch = (size_t)(S + Lc - 1) / Lc;
  return (size_t)Tf * nb * (want_D ? 20 : 12) + (size_t)S * nb * 4 + nb * 4 + nch * nb * 8 + (nch + 1) * nb * 4 +
         (size_t)(S + 6) * g.N * 4;
}

void launch_stretch_analysis(const FxStretchDev& d, const float* rows, hipStream_t s, hipEvent_t* ev) {
  RVCX_CHECK(d.g.nb <= kMaxNb && d.g.N <= 8192, "stretch: frame too long");
  const dim3 grid((unsigned)d.Tf, (unsigned)d.R);
  hipLaunchKernelGGL(stretch_fft_kernel, grid, dim3(256), (size_t)d.g.N * sizeof(float2), s, d, rows);
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(stretch_own_kernel, grid, dim3(64), 0, s, d);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
}

void launch_stretch_segment(const FxStretchDev& d, long s0, float* y, long ld_y, hipStream_t s, hipEvent_t* ev) {
  const int nch = (d.S + d.Lc - 1) / d.Lc, N = d.g.N;
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(stretch_compose_kernel, dim3(nch, d.R), dim3(256), 0, s, d, s0);
  hipLaunchKernelGGL(stretch_carry_kernel, dim3(d.R), dim3(256), 0, s, d, nch);
  hipLaunchKernelGGL(stretch_apply_kernel, dim3(nch, d.R), dim3(256), 0, s, d, s0);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
  hipLaunchKernelGGL(stretch_ifft_kernel, dim3(d.S, d.R), dim3(256), (size_t)N * sizeof(float2), s, d, s0);
  if (ev) RVCX_HIP(hipEventRecord(ev[2], s));
  const long span = (long)d.S * d.g.H + N;       // samples a segment can complete (the last one runs to the row's end)
  hipLaunchKernelGGL(stretch_ola_kernel, dim3((unsigned)cdiv64(span, 256), d.R), dim3(256), 0, s, d, s0, y, ld_y);
  // the last three frames move to the front for the next segment (by way of tmp3: the two ranges overlap when S < 3)
  const size_t three = (size_t)3 * N * sizeof(float), pitch = (size_t)(d.S + 3) * N * sizeof(float);
  RVCX_HIP(hipMemcpy2DAsync(d.tmp3, three, d.fr + (size_t)d.S * N, pitch, three, d.R, hipMemcpyDeviceToDevice, s));
  RVCX_HIP(hipMemcpy2DAsync(d.fr, pitch, d.tmp3, three, three, d.R, hipMemcpyDeviceToDevice, s));
  if (ev) RVCX_HIP(hipEventRecord(ev[3], s));
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------
namespace {

using cplx = std::complex<double>;

}  // namespace

void fx_stretch_own_host(const float* A2, int nb, int32_t* own) {
  auto peak = [&](int k) {
    const float v = A2[k];
    return v > 0.f && (k < 1 || v > A2[k - 1]) && (k < 2 || v > A2[k - 2]) && (k + 1 >= nb || v >= A2[k + 1]) &&
           (k + 2 >= nb || v >= A2[k + 2]);
  };
  std::vector<int> lo((size_t)nb);
  int run = -1;
  for (int k = 0; k < nb; ++k) {
    if (peak(k)) run = k;
    lo[k] = run;
  }
  int above = INT_MAX;
  for (int k = nb - 1; k >= 0; --k) {
    if (peak(k)) above = k;
    if (lo[k] < 0) own[k] = above == INT_MAX ? k : above;
    else own[k] = (above == INT_MAX || k - lo[k] <= above - k) ? lo[k] : above;
  }
}

void fx_stretch_host(const float* x, long n, int sr, long P, long Q, float* y, float* D_out, int32_t* own_out, uint32_t* TH_out,
                     uint32_t* R_out) {
  const FxStretchGeom g = fx_stretch_geom(sr);
  const int N = g.N, H = g.H, nb = g.nb;
  const long T = fx_stretch_T(n, H), J = fx_stretch_J(T, P, Q), ns = fx_stretch_len(n, P, Q), Tf = T + 2;
  std::vector<float> w;
  std::vector<float2> twf;
  fx_stretch_tables(N, w, twf);
  std::vector<cplx> tw((size_t)N / 2);
  for (int k = 0; k < N / 2; ++k) tw[k] = cplx(std::cos(2.0 * kPi * k / N), -std::sin(2.0 * kPi * k / N));
  std::vector<float> A((size_t)Tf * nb, 0.f), A2((size_t)nb);
  std::vector<uint32_t> TH((size_t)Tf * nb, 0u);
  std::vector<int32_t> own((size_t)Tf * nb);
  std::vector<cplx> buf((size_t)N);
  if (D_out) std::memset(D_out, 0, (size_t)Tf * nb * 2 * sizeof(float));
  for (long t = 0; t < Tf; ++t) {
    const size_t base = (size_t)t * nb;
    if (t < T) {
      for (int i = 0; i < N; ++i) {
        const long src = t * H - N / 2 + i;
        buf[i] = (src >= 0 && src < n) ? cplx((double)w[i] * (double)x[src], 0.0) : cplx(0.0, 0.0);
      }
      fft_host(buf, tw);
      for (int k = 0; k < nb; ++k) {
        const float re = (float)buf[k].real(), im = (float)buf[k].imag();
        if (D_out) D_out[(base + k) * 2] = re, D_out[(base + k) * 2 + 1] = im;
        const float rr = re * re, ii = im * im;
        A2[k] = rr + ii;
        A[base + k] = sqrtf(A2[k]);
        TH[base + k] = A2[k] == 0.f ? 0u : (uint32_t)(int64_t)std::rint((double)atan2f(im, re) * (2147483648.0 / kPi));
      }
    } else {
      std::fill(A2.begin(), A2.end(), 0.f);
    }
    fx_stretch_own_host(A2.data(), nb, own.data() + base);
  }
  if (own_out) std::copy(own.begin(), own.end(), own_out);
  if (TH_out) std::copy(TH.begin(), TH.end(), TH_out);
  // output frames: the recurrence on R, the synthesis and the overlap-add in double
  std::vector<uint32_t> R((size_t)nb, 0u), Rn((size_t)nb);
  std::vector<double> num((size_t)ns + 1, 0.0), den((size_t)ns + 1, 0.0);
  for (long j = 0; j < J; ++j) {
    const long jq = j * Q, tj = jq / P;
    const double f = (double)(jq - tj * P) / (double)P;
    if (R_out) std::copy(R.begin(), R.end(), R_out + (size_t)j * nb);
    const size_t base = (size_t)tj * nb;
    std::fill(buf.begin(), buf.end(), cplx(0.0, 0.0));
    for (int k = 0; k < nb; ++k) {
      const double M = (1.0 - f) * (double)A[base + k] + f * (double)A[base + nb + k];
      const double ang = (double)(int32_t)(R[k] + TH[base + k]) * (kPi / 2147483648.0);
      const bool edge = k == 0 || k == N / 2;
      const cplx X(M * std::cos(ang), edge ? 0.0 : M * std::sin(ang));
      buf[k] = std::conj(X);
      if (!edge) buf[N - k] = X;
    }
    fft_host(buf, tw);
    for (int i = 0; i < N; ++i) {
      const long m = j * H - N / 2 + i;
      if (m < 0 || m >= ns) continue;
      num[m] += (double)w[i] * (buf[i].real() / N);
      den[m] += (double)w[i] * (double)w[i];
    }
    if (j + 1 < J) {
      const long tj1 = (j + 1) * Q / P;
      const int32_t* oj = own.data() + (size_t)tj * nb;
      const int32_t* oj1 = own.data() + (size_t)tj1 * nb;
      const uint32_t* tha = TH.data() + (size_t)(tj + 1) * nb;
      const uint32_t* thb = TH.data() + (size_t)tj1 * nb;
      for (int k = 0; k < nb; ++k) {
        const int p = oj1[k];
        Rn[k] = R[oj[p]] + (tha[p] - thb[p]);
      }
      R.swap(Rn);
    }
  }
  for (long m = 0; m < ns; ++m) y[m] = den[m] > 1e-8 ? (float)(num[m] / den[m]) : 0.f;
}

}  // namespace rvcx
