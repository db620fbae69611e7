// The effects board inside a live session (include/rvcx.h "live post-production").  A block is 10 .. 200 ms:
// every stage is a short recurrence and the work is latency.  Each stage therefore runs in sample order from state the
// session carries -- the definition that makes a step's output independent of the cut -- and only its true dependent chain is
// walked by one lane, on data staged in LDS:
//
//  * biquads: two FMAs per sample (fx_bq_step); one workgroup per row, lane 0 walks a tile, the others load and store it.
//  * followers: sub + FMA per sample; the gate's square root between its two followers and both gains run wide.
//  * comb: the line's old values, their (1 - d) products, the input and the write-back run wide over up to D samples (a
//    line is read D samples before it is written); the damping one-pole between them is one FMA per sample on lane 0.
//    One wave per (comb, side, stream).
//  * all-pass: the comb sum wide, then blocks of the shortest delay, one sample per lane; both sides in one workgroup, which
//    then forms the stereo mix.
//  * chorus: blocks of floor(tau_min) - 1 samples, one sample per lane, on a ring in the state itself.
//
// State exists twice and a step reads set `cur` and writes the other one.  Delay lines are copied whole (they are short);
// a chorus ring is not: the set being written last saw the block before the previous one, so the step first copies the
// previous block over from the set it reads, then appends its own.  Both sets are complete up to their last block that way.
#include <algorithm>

#include "common.h"
#include "effects_device.h"

#pragma clang fp contract(off)

namespace rvcx {

constexpr int kFxlTile = 4096;       // samples of a row staged per round in the per-row kernels (16 kB)

FxLiveLayout fx_live_layout(int sr, long block) {
  FxLiveLayout L{};
  const FxReverb rv = fx_reverb_setup(sr, 0.0, 0.0, 0.0, 0.0, 0.0);
  long at = kFxlLines;
  for (int side = 0; side < 2; ++side)
    for (int i = 0; i < 8; ++i) L.comb[side][i] = (int)at, at += rv.comb[side][i];
  for (int side = 0; side < 2; ++side)
    for (int q = 0; q < 4; ++q) L.ap[side][q] = (int)at, at += rv.ap[side][q];
  L.cap = (long)sr + 2 + 2 * block;
  for (int c = 0; c < 2; ++c) L.chorus[c] = at, at += L.cap;
  L.per_stream = at;
  return L;
}

// ---- layout -----------------------------------------------------------------------------------------------------------------
__global__ void fxl_load_kernel(const float* __restrict__ src, long src_stride, int C, float* __restrict__ rows, long B) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  if (i >= B) return;
  for (int c = 0; c < C; ++c) rows[((long)s * C + c) * B + i] = src[(long)s * src_stride + i * C + c];
}

// a mono row leaves as L = R (convert_to_stereo)
__global__ void fxl_store_kernel(const float* __restrict__ rows, int C, float* __restrict__ out, long out_stride, long B) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  if (i >= B) return;
  const float l = rows[((long)s * C) * B + i], r = rows[((long)s * C + C - 1) * B + i];
  *reinterpret_cast<float2*>(out + (long)s * out_stride + 2 * i) = make_float2(l, r);
}

// ---- linear stages ------------------------------------------------------------------------------------------------------------
// One workgroup per row.  slot: the stage's (s1, s2) of channel 0 inside a stream's state.
__global__ void __launch_bounds__(256) fxl_biquad_kernel(FxBiquad q, const float* __restrict__ x, float* __restrict__ y, int C,
                                                         long B, long per_stream, int slot, const float* __restrict__ st_in,
                                                         float* __restrict__ st_out) {
  __shared__ __attribute__((aligned(16))) float tl[kFxlTile];
  const int r = blockIdx.x, t = threadIdx.x;
  const long so = (long)(r / C) * per_stream + slot + 2 * (r % C);
  float s1 = st_in[so], s2 = st_in[so + 1];
  const float* xr = x + (long)r * B;
  float* yr = y + (long)r * B;
  for (long j0 = 0; j0 < B; j0 += kFxlTile) {
    const int m = (int)min((long)kFxlTile, B - j0);
    for (int i = t; i < m; i += 256) tl[i] = xr[j0 + i];
    __syncthreads();
    if (t == 0) {
      int i = 0;
      for (; i + 4 <= m; i += 4) {
        float4 v = *reinterpret_cast<float4*>(tl + i);
        v.x = fx_bq_step(q, v.x, s1, s2);
        v.y = fx_bq_step(q, v.y, s1, s2);
        v.z = fx_bq_step(q, v.z, s1, s2);
        v.w = fx_bq_step(q, v.w, s1, s2);
        *reinterpret_cast<float4*>(tl + i) = v;
      }
      for (; i < m; ++i) tl[i] = fx_bq_step(q, tl[i], s1, s2);
    }
    __syncthreads();
    for (int i = t; i < m; i += 256) yr[j0 + i] = tl[i];
    __syncthreads();
  }
  if (t == 0) st_out[so] = s1, st_out[so + 1] = s2;
}

// ---- compressor and gate ----------------------------------------------------------------------------------------------------
// lane 0 walks a follower over a staged tile: e in, e out, env[i] = the state after sample i
__device__ inline float fxl_follow_tile(const float* in, float* env, int m, float e, int square, float c_att, float c_rel) {
  int i = 0;
  for (; i + 4 <= m; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(in + i);
    float4 w;
    w.x = e = fx_follow_step(v.x, e, square, c_att, c_rel);
    w.y = e = fx_follow_step(v.y, e, square, c_att, c_rel);
    w.z = e = fx_follow_step(v.z, e, square, c_att, c_rel);
    w.w = e = fx_follow_step(v.w, e, square, c_att, c_rel);
    *reinterpret_cast<float4*>(env + i) = w;
  }
  for (; i < m; ++i) env[i] = e = fx_follow_step(in[i], e, square, c_att, c_rel);
  return e;
}

// gate = 0: e follows |x| (c_att, c_rel).  gate = 1: r follows x^2 (c0, c50), e follows sqrt(r) (c_att, c_rel).
__global__ void __launch_bounds__(256) fxl_dynamics_kernel(int gate, float c0, float c50, float c_att, float c_rel, float thr,
                                                           float expo, const float* __restrict__ x, float* __restrict__ y,
                                                           int C, long B, long per_stream, const float* __restrict__ st_in,
                                                           float* __restrict__ st_out) {
  __shared__ __attribute__((aligned(16))) float xs[kFxlTile];
  __shared__ __attribute__((aligned(16))) float es[kFxlTile];
  const int row = blockIdx.x, t = threadIdx.x;
  const long so = (long)(row / C) * per_stream + kFxlFollow + (row % C);
  float e = st_in[so + (gate ? 4 : 0)], r = gate ? st_in[so + 2] : 0.f;
  const float* xr = x + (long)row * B;
  float* yr = y + (long)row * B;
  for (long j0 = 0; j0 < B; j0 += kFxlTile) {
    const int m = (int)min((long)kFxlTile, B - j0);
    for (int i = t; i < m; i += 256) xs[i] = xr[j0 + i];
    __syncthreads();
    if (gate) {
      if (t == 0) r = fxl_follow_tile(xs, es, m, r, 1, c0, c50);
      __syncthreads();
      for (int i = t; i < m; i += 256) es[i] = FX_SQRT(es[i]);
      __syncthreads();
      if (t == 0) e = fxl_follow_tile(es, es, m, e, 0, c_att, c_rel);
    } else if (t == 0) {
      e = fxl_follow_tile(xs, es, m, e, 0, c_att, c_rel);
    }
    __syncthreads();
    for (int i = t; i < m; i += 256) yr[j0 + i] = FX_MUL(xs[i], fx_gain(es[i], gate, thr, expo));
    __syncthreads();
  }
  if (t == 0) {
    st_out[so + (gate ? 4 : 0)] = e;
    if (gate) st_out[so + 2] = r;
  }
}

// ---- Freeverb -----------------------------------------------------------------------------------------------------------------
// One wave per (comb, side, stream).  x: the stream's rows (C of them; a mono row is both sides).  n0: the block's first
// global sample.  LDS: the line (D, padded to 4), then two tiles of `tile` floats.
__global__ void __launch_bounds__(64) fxl_comb_kernel(FxReverb rv, FxLiveLayout L, const float* __restrict__ x, int C,
                                                      float* __restrict__ combs, long B, long n0,
                                                      const float* __restrict__ st_in, float* __restrict__ st_out, int tile) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  const int ci = blockIdx.x, side = blockIdx.y, s = blockIdx.z, l = threadIdx.x;
  const int D = rv.comb[side][ci];
  float* line = sh;
  float* oo = sh + ((D + 3) & ~3);
  float* inn = oo + tile;
  const long sb = (long)s * L.per_stream;
  for (int i = l; i < D; i += 64) line[i] = st_in[sb + L.comb[side][ci] + i];
  float last = st_in[sb + kFxlLast + side * 8 + ci];
  const float* xl = x + ((long)s * C) * B;
  const float* xr = x + ((long)s * C + C - 1) * B;
  float* out = combs + (((long)s * 2 + side) * 8 + ci) * B;
  int pos = (int)(n0 % D);
  const int span = min(tile, D);                  // samples whose reads of the line precede every write
  __syncthreads();
  for (long j0 = 0; j0 < B; j0 += span) {
    const int m = (int)min((long)span, B - j0);
    for (int k = l; k < m; k += 64) {
      int p = pos + k;
      if (p >= D) p -= D;
      const float o = line[p];
      oo[k] = FX_MUL(o, rv.omd);
      out[j0 + k] = o;
      inn[k] = FX_MUL(0.015f, xl[j0 + k] + xr[j0 + k]);
    }
    __syncthreads();
    if (l == 0) {
      int k = 0;
      for (; k + 4 <= m; k += 4) {
        float4 v = *reinterpret_cast<float4*>(oo + k);
        v.x = last = FX_FMA(last, rv.d, v.x);
        v.y = last = FX_FMA(last, rv.d, v.y);
        v.z = last = FX_FMA(last, rv.d, v.z);
        v.w = last = FX_FMA(last, rv.d, v.w);
        *reinterpret_cast<float4*>(oo + k) = v;
      }
      for (; k < m; ++k) oo[k] = last = FX_FMA(last, rv.d, oo[k]);
    }
    __syncthreads();
    for (int k = l; k < m; k += 64) {
      int p = pos + k;
      if (p >= D) p -= D;
      line[p] = FX_FMA(oo[k], rv.fb, inn[k]);
    }
    __syncthreads();
    pos = (pos + m) % D;
  }
  for (int i = l; i < D; i += 64) st_out[sb + L.comb[side][ci] + i] = line[i];
  if (l == 0) st_out[sb + kFxlLast + side * 8 + ci] = last;
}

// One workgroup per stream, wave = side: the eight comb outputs summed in order, the four all-passes in series in blocks of T
// (the shortest all-pass delay of either side: inside a block every sample meets its own word of every line), then the mix.
// LDS: the lines of side 0, those of side 1, two tiles.
__global__ void __launch_bounds__(128) fxl_allpass_mix_kernel(FxReverb rv, FxLiveLayout L, const float* __restrict__ x, int C,
                                                              const float* __restrict__ combs, float* __restrict__ y, long B,
                                                              long n0, const float* __restrict__ st_in,
                                                              float* __restrict__ st_out, int tile, int T) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  const int s = blockIdx.x, side = threadIdx.x >> 6, l = threadIdx.x & 63;
  int D[4], base[4], pos[4], tot[2] = {0, 0};
  for (int q = 0; q < 4; ++q) tot[0] += rv.ap[0][q], tot[1] += rv.ap[1][q];
  for (int q = 0, at = 0; q < 4; ++q) D[q] = rv.ap[side][q], base[q] = at, at += D[q], pos[q] = (int)(n0 % D[q]);
  float* line = sh + (side ? tot[0] : 0);
  float* acc = sh + tot[0] + tot[1];               // [side][tile]
  const long sb = (long)s * L.per_stream + L.ap[side][0];
  for (int i = l; i < tot[side]; i += 64) line[i] = st_in[sb + i];
  const float* cb = combs + (((long)s * 2 + side) * 8) * B;
  const float* xl = x + ((long)s * C) * B;
  const float* xr = x + ((long)s * C + C - 1) * B;
  float* yl = y + ((long)s * 2) * B;
  float* yr = yl + B;
  __syncthreads();
  for (long j0 = 0; j0 < B; j0 += tile) {
    const int m = (int)min((long)tile, B - j0);
    float* a = acc + side * tile;
    for (int i = l; i < m; i += 64) {
      float in = cb[j0 + i];
      for (int c = 1; c < 8; ++c) in += cb[(long)c * B + j0 + i];
      a[i] = in;
    }
    __syncthreads();
    for (int k0 = 0; k0 < m; k0 += T) {
      const int k1 = min(k0 + T, m);
      for (int i = k0 + l; i < k1; i += 64) {
        float in = a[i];
        for (int q = 0; q < 4; ++q) {
          float* w = line + base[q] + (pos[q] + i) % D[q];
          const float v = *w;
          *w = FX_FMA(0.5f, v, in);
          in = FX_SUB(v, in);
        }
        a[i] = in;
      }
      __syncthreads();
    }
    for (int q = 0; q < 4; ++q) pos[q] = (pos[q] + m) % D[q];
    for (int i = threadIdx.x; i < m; i += 128) {
      const float ol = acc[i], orr = acc[tile + i];
      yl[j0 + i] = FX_FMA(ol, rv.w1, FX_FMA(orr, rv.w2, FX_MUL(rv.dry2, xl[j0 + i])));
      yr[j0 + i] = FX_FMA(orr, rv.w1, FX_FMA(ol, rv.w2, FX_MUL(rv.dry2, xr[j0 + i])));
    }
    __syncthreads();
  }
  for (int i = l; i < tot[side]; i += 64) st_out[sb + i] = line[i];
}

// ---- chorus ---------------------------------------------------------------------------------------------------------------------
// the delay line of a stream and channel: the last `cap` samples, sample n at n mod cap
struct FxlRing {
  const float* p;
  long cap;
  __device__ float operator[](long i) const { return p[i % cap]; }
};

// One workgroup per row.  The ring written is first brought up to the previous block (see the head of the file), then the
// block is appended: at once when feedback == 0 (the line is the input), else in blocks of T = floor(tau_min) - 1 samples,
// whose interpolation neighbours were all written by earlier blocks.
__global__ void __launch_bounds__(256) fxl_chorus_kernel(FxChorus ch, FxLiveLayout L, const float* __restrict__ x,
                                                         float* __restrict__ y, int C, long B, long n0, const float* st_in,
                                                         float* st_out) {
  const int r = blockIdx.x, t = threadIdx.x;
  const long so = (long)(r / C) * L.per_stream + L.chorus[r % C];
  const float* before = st_in + so;
  float* ring = st_out + so;
  const float* xr = x + (long)r * B;
  float* yr = y + (long)r * B;
  if (n0 > 0)
    for (long i = t; i < B; i += 256) ring[(n0 - B + i) % L.cap] = before[(n0 - B + i) % L.cap];
  const FxlRing d{ring, L.cap};
  if (ch.fb == 0.f) {
    for (long i = t; i < B; i += 256) ring[(n0 + i) % L.cap] = xr[i];
    __syncthreads();
    for (long i = t; i < B; i += 256) yr[i] = FX_FMA(ch.mix, fx_chorus_tap(ch, d, n0 + i), FX_MUL(ch.omm, xr[i]));
    return;
  }
  __syncthreads();
  for (long j0 = 0; j0 < B; j0 += ch.T) {
    const long j1 = min(j0 + ch.T, B);
    for (long i = j0 + t; i < j1; i += 256) {
      const float w = fx_chorus_tap(ch, d, n0 + i), xv = xr[i];
      ring[(n0 + i) % L.cap] = FX_FMA(ch.fb, w, xv);
      yr[i] = FX_FMA(ch.mix, w, FX_MUL(ch.omm, xv));
    }
    __syncthreads();
  }
}

// ---- one step -------------------------------------------------------------------------------------------------------------------
void fx_live_step(const FxLive& f, const float* src, long src_stride, int C, int cur, uint64_t step, float* out,
                  long out_stride, hipStream_t s, hipEvent_t* ev) {
  RVCX_CHECK(C == 1 || C == 2, "live effects: one or two channels");
  const FxLivePlan& P = f.plan;
  const FxLiveLayout& L = f.L;
  const int S = f.S;
  const long B = f.B, n0 = (long)step * B, per = L.per_stream;
  const float* si = f.state[cur];
  float* so = f.state[cur ^ 1];
  float* a = f.work;
  float* b = a + (size_t)2 * S * B;
  float* combs = b + (size_t)2 * S * B;
  auto mark = [&](int k) {
    if (ev) RVCX_HIP(hipEventRecord(ev[k], s));
  };
  const dim3 wide((unsigned)((B + 255) / 256), S);
  mark(0);
  hipLaunchKernelGGL(fxl_load_kernel, wide, dim3(256), 0, s, src, src_stride, C, a, B);
  int Cc = C;                                       // rows per stream: L == R is one row until the reverb
  auto biquad = [&](const FxBiquad& q, int j) {
    hipLaunchKernelGGL(fxl_biquad_kernel, dim3(S * Cc), dim3(256), 0, s, q, a, b, Cc, B, per, kFxlBiquad + 4 * j, si, so);
    std::swap(a, b);
  };
  if (P.on[0]) biquad(P.hp, 0);
  mark(1);
  if (P.on[1]) {
    hipLaunchKernelGGL(fxl_dynamics_kernel, dim3(S * Cc), dim3(256), 0, s, 0, 0.f, 0.f, P.comp_ca, P.comp_cr, P.comp_thr,
                       P.comp_expo, a, b, Cc, B, per, si, so);
    std::swap(a, b);
  }
  mark(2);
  if (P.on[2]) {
    hipLaunchKernelGGL(fxl_dynamics_kernel, dim3(S * Cc), dim3(256), 0, s, 1, P.gate_c0, P.gate_c50, P.gate_ca, P.gate_cr,
                       P.gate_thr, P.gate_expo, a, b, Cc, B, per, si, so);
    std::swap(a, b);
  }
  mark(3);
  if (P.on[3]) {
    int dmax = 0, tot = 0, T = P.rv.ap[0][0];
    for (int i = 0; i < 8; ++i) dmax = std::max(dmax, P.rv.comb[1][i]);
    for (int side = 0; side < 2; ++side)
      for (int q = 0; q < 4; ++q) tot += P.rv.ap[side][q], T = std::min(T, P.rv.ap[side][q]);
    // tiles as large as 64 kB of LDS allow, at most 2048 samples
    const int line = (dmax + 3) & ~3;
    const int ct = std::min(2048, ((16384 - line) / 2) & ~63), at = std::min(2048, ((16384 - tot) / 2) & ~63);
    RVCX_CHECK(ct >= 64 && at >= 64 && T >= 1, "live reverb: the delay lines exceed the LDS plan");
    hipLaunchKernelGGL(fxl_comb_kernel, dim3(8, 2, S), dim3(64), (size_t)(line + 2 * ct) * 4, s, P.rv, L, a, Cc, combs, B, n0, si,
                       so, ct);
    hipLaunchKernelGGL(fxl_allpass_mix_kernel, dim3(S), dim3(128), (size_t)(tot + 2 * at) * 4, s, P.rv, L, a, Cc, combs, b, B, n0,
                       si, so, at, T);
    std::swap(a, b);
    Cc = 2;
  }
  mark(4);
  if (P.on[4]) biquad(P.lo, 1);
  mark(5);
  if (P.on[5]) biquad(P.hi, 2);
  mark(6);
  if (P.on[6]) {
    RVCX_CHECK(P.ch.fb == 0.f || P.ch.T >= 1, "live chorus: block");
    hipLaunchKernelGGL(fxl_chorus_kernel, dim3(S * Cc), dim3(256), 0, s, P.ch, L, a, b, Cc, B, n0, si, so);
    std::swap(a, b);
  }
  hipLaunchKernelGGL(fxl_store_kernel, wide, dim3(256), 0, s, a, Cc, out, out_stride, B);
  mark(7);
}

}  // namespace rvcx
