// Live-stream sessions: the rolling 16 kHz context and SOLA (synchronised overlap-add) on the device.
//
// SOLA aligns the synthesized tail of one step with the carry of the step before: the offset d in [0, Ls] that maximises the
// normalised cross-correlation of y[d .. d + Lx) with the carry, then a sin^2 cross-fade (rvcx.h, rvcx_op_sola).  The work is
// (Ls + 1) x Lx multiply-adds per stream and step (481 x 2400 at 48 kHz, 50 ms cross-fade, 10 ms search): one wave per offset,
// lane-strided partial sums in a fixed order, a butterfly reduction.  Both sums of an offset are formed directly from y -- no
// running difference between neighbouring offsets -- so silence ties exactly (every score is the same 0 / sqrt(1e-8)) and a
// long session cannot drift.  Nothing in the order depends on S: a stream gives the same bits alone and in a group.
#include <algorithm>

#include "ops.h"

namespace rvcx {

namespace {

constexpr int kSolaWaves = 4;      // offsets per workgroup (one wave each)

__global__ void ring_shift_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ blocks,
                                  long n, long blk, long total) {
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long b = idx / n, r = idx - b * n;
    dst[idx] = r < n - blk ? src[b * n + r + blk] : blocks[b * blk + r - (n - blk)];
  }
}

// grid (ceil((Ls + 1) / kSolaWaves), S), 64 * kSolaWaves threads: wave w of block x scores offset d = x * kSolaWaves + w
__global__ void __launch_bounds__(64 * kSolaWaves) sola_score_kernel(const float* __restrict__ y, long y_bs,
                                                                      const float* __restrict__ b, float* __restrict__ scores,
                                                                      int Lx, int Ls) {
  const int lane = threadIdx.x & 63, d = blockIdx.x * kSolaWaves + (threadIdx.x >> 6);
  if (d > Ls) return;                               // whole waves leave together
  const float* ys = y + (long)blockIdx.y * y_bs + d;
  const float* bs = b + (long)blockIdx.y * Lx;
  float nom = 0.f, en = 0.f;
  for (int i = lane; i < Lx; i += 64) {             // d + i <= Ls + Lx - 1 < Lb + Lx + Ls
    const float v = ys[i];
    nom = fmaf(v, bs[i], nom);
    en = fmaf(v, v, en);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nom += __shfl_xor(nom, o, 64);
    en += __shfl_xor(en, o, 64);
  }
  if (lane == 0) scores[(long)blockIdx.y * (Ls + 1) + d] = nom / sqrtf(en + 1e-8f);
}

// one workgroup of 256 per stream: first-index argmax of the scores, cross-fade, carry.  b_out may alias b_in: element i of
// the carry is read and written by the same thread, in that order.
__global__ void __launch_bounds__(256) sola_apply_kernel(const float* __restrict__ y, long y_bs, const float* b_in,
                                                         const float* __restrict__ scores, float* __restrict__ out, long out_bs,
                                                         float* b_out, int* __restrict__ offset, int Lb, int Lx, int Ls) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int tid = threadIdx.x, st = blockIdx.x;
  const float* sc = scores + (long)st * (Ls + 1);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int d = tid; d <= Ls; d += 256) {            // ascending d per thread: strict > keeps the first index
    const float v = sc[d];
    if (v > best || bi == 0x7fffffff) {
      best = v;
      bi = d;
    }
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const float v = sv[tid + o];
      const int j = si[tid + o];
      if (j != 0x7fffffff && (si[tid] == 0x7fffffff || v > sv[tid] || (v == sv[tid] && j < si[tid]))) {
        sv[tid] = v;
        si[tid] = j;
      }
    }
    __syncthreads();
  }
  const int d = min(max(si[0], 0), Ls);             // (a NaN score can never win; the clamp keeps every read in bounds regardless)
  if (tid == 0) offset[st] = d;
  const float* ys = y + (long)st * y_bs + d;
  float* o = out + (long)st * out_bs;
  const float* bin = b_in + (long)st * Lx;
  float* bout = b_out + (long)st * Lx;
  const double step = Lx > 1 ? 1.5707963267948966 / (double)(Lx - 1) : 0.0;
  for (int i = tid; i < Lb; i += 256) {
    float v = ys[i];
    if (i < Lx) {
      const double w = sin(step * i);
      const float fin = (float)(w * w);
      v = v * fin + bin[i] * (1.f - fin);
    }
    o[i] = v;
  }
  __syncthreads();                                  // every read of the old carry (i < min(Lx, Lb)) precedes the writes below
  for (int i = tid; i < Lx; i += 256) bout[i] = ys[Lb + i];   // d + Lb + i <= Ls + Lb + Lx - 1
}

}  // namespace

void launch_ring_shift(const float* src, float* dst, const float* blocks, int S, long n, long blk, hipStream_t s) {
  const long tot = (long)S * n;
  hipLaunchKernelGGL(ring_shift_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 1 << 20)), dim3(256), 0, s, src, dst,
                     blocks, n, blk, tot);
}

void launch_sola(const float* y, long y_bs, const float* b_in, float* out, long out_bs, float* b_out, int* offset,
                 float* scores, int S, int Lb, int Lx, int Ls, hipStream_t s) {
  RVCX_CHECK(S >= 1 && Lb >= 1 && Lx >= 1 && Ls >= 0, "sola: bad geometry");
  hipLaunchKernelGGL(sola_score_kernel, dim3((Ls + kSolaWaves) / kSolaWaves, S), dim3(64 * kSolaWaves), 0, s, y, y_bs, b_in,
                     scores, Lx, Ls);
  hipLaunchKernelGGL(sola_apply_kernel, dim3(S), dim3(256), 0, s, y, y_bs, b_in, scores, out, out_bs, b_out, offset, Lb, Lx,
                     Ls);
}

}  // namespace rvcx
