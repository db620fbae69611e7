// What the spectral stages share (pitch.hip: stages 13 and 14, denoise.hip: stage 15): the radix-2 transform in LDS, its double
// twin on the host, and the gather of the overlap-add.  Every rounding is written out, so contraction is off from here on in
// whichever file includes this one.
#pragma once
#include <hip/hip_runtime.h>
#include <complex>
#include <vector>

#pragma clang fp contract(off)

namespace rvcx {

// in place on a[0 .. N) in LDS, input in bit-reversed order: decimation in time, e^(-2 pi i ..) twiddles (256 lanes)
__device__ __forceinline__ void fft_lds(float2* a, const float2* __restrict__ tw, int N, int logN) {
  for (int st = 0; st < logN; ++st) {
    const int half = 1 << st;
    __syncthreads();
    for (int b = threadIdx.x; b < N / 2; b += 256) {
      const int pos = b & (half - 1), i0 = ((b >> st) << (st + 1)) + pos, i1 = i0 + half;
      const float2 w = tw[pos << (logN - 1 - st)];
      const float2 u = a[i0], v = a[i1];
      const float tx = w.x * v.x - w.y * v.y, ty = w.x * v.y + w.y * v.x;
      a[i0] = make_float2(u.x + tx, u.y + ty);
      a[i1] = make_float2(u.x - tx, u.y - ty);
    }
  }
  __syncthreads();
}

// sample m of an overlap-add of J windowed frames of N samples, hop H, frame j centred at j H: the frames that cover m in
// ascending j, divided by the window sum (in double); 0 where that sum is <= 1e-8.  Frame j lies at fr[(j + joff) stride].
__device__ __forceinline__ float ola_gather(const float* __restrict__ fr, long joff, size_t stride, const float* __restrict__ w,
                                            long m, long J, int N, int H) {
  const long jlo = max(0L, (m - N / 2 + H) / H), jhi = min(J - 1, (m + N / 2) / H);
  float num = 0.f;
  double den = 0.0;
  for (long j = jlo; j <= jhi; ++j) {
    const long i = m + N / 2 - j * H;
    if (i < 0 || i >= N) continue;                    // (never: the bounds of jlo and jhi)
    num += fr[(size_t)(j + joff) * stride + i];
    den += (double)w[i] * (double)w[i];
  }
  return den > 1e-8 ? (float)((double)num / den) : 0.f;
}

// forward transform in double, in place, natural order in and out; tw[k] = e^(-2 pi i k / N), k < N / 2
inline void fft_host(std::vector<std::complex<double>>& a, const std::vector<std::complex<double>>& tw) {
  using cplx = std::complex<double>;
  const int N = (int)a.size();
  int logN = 0;
  while ((1 << logN) < N) ++logN;
  for (int i = 0; i < N; ++i) {
    int j = 0;
    for (int b = 0; b < logN; ++b) j |= ((i >> b) & 1) << (logN - 1 - b);
    if (j > i) std::swap(a[i], a[j]);
  }
  for (int st = 0; st < logN; ++st) {
    const int half = 1 << st;
    for (int b = 0; b < N / 2; ++b) {
      const int pos = b & (half - 1), i0 = ((b >> st) << (st + 1)) + pos, i1 = i0 + half;
      const cplx t = tw[(size_t)pos << (logN - 1 - st)] * a[i1];
      a[i1] = a[i0] - t;
      a[i0] += t;
    }
  }
}

}  // namespace rvcx
