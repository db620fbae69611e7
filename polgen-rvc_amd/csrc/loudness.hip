// Loudness, true peak, limiter and master (include/rvcx.h stages 9 - 12).
//
//  * Programme loudness: the K-weighting filter is a cascade of two biquads, i.e. a linear recurrence on four states.  It
//    runs as the biquad scan does (effects.hip): lane = chunk of kFxChunk samples from zero state, one carry walk per row
//    over the chunks' end states with the 4 x 4 map of a chunk of zeros, then every chunk again from its true state.  The
//    second run squares and sums instead of storing: a chunk writes one partial sum per hop it touches (at most three, hops
//    and chunks do not line up), and the gate kernel adds the partials of a hop in chunk order.  Everything is double.
//  * Gates: one workgroup per item.  Lane t sums blocks t, t + 256, ... in that order and the 256 lanes are folded by a
//    fixed tree, so a result depends on the item alone -- not on the batch or the grouping.
//  * True peak: 1024 samples and their 12-sample halos in LDS, a lane evaluates the three non-trivial phases of four
//    consecutive samples from 28 registers.  The oversampled signal is never stored.  max is exact and order independent,
//    so the per-item peak is a wave reduction and an atomic max on the non-negative floats' bits.
//  * Limiter: r = min(1, c / p), its minimum over W + 1 samples by doubling windows in LDS (exact), the release by
//    launch_fx_follower unchanged, the box mean as a sum of W + 1 doubles.  q = 1 - e is a multiple of 2^-24 in [0, 1], so
//    that sum is exact in double in ANY order (W + 1 <= 1921 < 2^11 terms): "index order" is kept anyway.
#include "effects.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "effects_device.h"

// every rounding below is written out: nothing may be fused behind the source's back, on either side
#pragma clang fp contract(off)

namespace rvcx {

// ---- coefficients and taps (host, double) ---------------------------------------------------------------------------------
FxKWeight fx_kweight(int sr) {
  FxKWeight k{};
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(M_PI * f0 / sr), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    k.sb0 = (Vh + Vb * K / Q + K * K) / a0, k.sb1 = 2.0 * (K * K - Vh) / a0, k.sb2 = (Vh - Vb * K / Q + K * K) / a0;
    k.sa1 = 2.0 * (K * K - 1.0) / a0, k.sa2 = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(M_PI * f0 / sr), a0 = 1.0 + K / Q + K * K;
    k.hb0 = 1.0, k.hb1 = -2.0, k.hb2 = 1.0;
    k.ha1 = 2.0 * (K * K - 1.0) / a0, k.ha2 = (1.0 - K / Q + K * K) / a0;
  }
  return k;
}

static double fx_bessel_i0(double x) {
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= (x / 2.0) / k;
    sum += term * term;
  }
  return sum;
}

const FxTpTaps& fx_tp_taps() {
  static const FxTpTaps taps = [] {
    FxTpTaps t{};
    const double i0b = fx_bessel_i0(9.0);
    for (int p = 1; p < 4; ++p)
      for (int j = 0; j < kTpTaps; ++j) {
        const double x = (double)(j - 12) + 0.25 * p, u = x / 12.0;
        const double sinc = std::sin(M_PI * x) / (M_PI * x);
        t.h[p - 1][j] = (float)(sinc * fx_bessel_i0(9.0 * std::sqrt(1.0 - u * u)) / i0b);
      }
    return t;
  }();
  return taps;
}

// ---- K-weighting + energy ---------------------------------------------------------------------------------------------------
struct FxMat4 {
  double m[4][4];
};
struct FxState4 {
  double s[4];
};

// the state a chunk leaves behind when it starts from zero
__global__ void fx_kw_local_kernel(FxKWeight kw, const float* __restrict__ x, const int* __restrict__ len, long ld, int nch,
                                   FxState4* __restrict__ z) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (k >= nch || (long)k * kFxChunk >= len[r]) return;
  const float4* p = reinterpret_cast<const float4*>(x + (long)r * ld + (long)k * kFxChunk);
  double st[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < kFxChunk / 4; ++i) {
    const float4 v = p[i];
    fx_kw_step(kw, (double)v.x, st);
    fx_kw_step(kw, (double)v.y, st);
    fx_kw_step(kw, (double)v.z, st);
    fx_kw_step(kw, (double)v.w, st);
  }
  FxState4 o;
  for (int i = 0; i < 4; ++i) o.s[i] = st[i];
  z[(long)r * nch + k] = o;
}

// One workgroup per row: s[k + 1] = M s[k] + z[k].  256 chunks at a time go through LDS, lane 0 walks them: the order is
// the chunk order whatever the row's length, the batch or the grouping.
__global__ void __launch_bounds__(256) fx_kw_carry_kernel(FxMat4 M, const FxState4* __restrict__ z, const int* __restrict__ len,
                                                          int nch_ld, FxState4* __restrict__ init) {
  __shared__ double sh[256][4];
  __shared__ double carry[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const int nch = (len[r] + kFxChunk - 1) / kFxChunk;
  if (t < 4) carry[t] = 0.0;
  for (int k0 = 0; k0 < nch; k0 += 256) {
    const int k = k0 + t;
    if (k < nch) {
      const FxState4 v = z[(long)r * nch_ld + k];
      for (int i = 0; i < 4; ++i) sh[t][i] = v.s[i];
    }
    __syncthreads();
    if (t == 0) {
      double c[4] = {carry[0], carry[1], carry[2], carry[3]};
      const int cnt = min(256, nch - k0);
      for (int j = 0; j < cnt; ++j) {
        double nx[4];
        for (int i = 0; i < 4; ++i) {
          nx[i] = fma(M.m[i][0], c[0], fma(M.m[i][1], c[1], fma(M.m[i][2], c[2], fma(M.m[i][3], c[3], sh[j][i]))));
          sh[j][i] = c[i];
        }
        for (int i = 0; i < 4; ++i) c[i] = nx[i];
      }
      for (int i = 0; i < 4; ++i) carry[i] = c[i];
    }
    __syncthreads();
    if (k < nch) {
      FxState4 v;
      for (int i = 0; i < 4; ++i) v.s[i] = sh[t][i];
      init[(long)r * nch_ld + k] = v;
    }
    __syncthreads();
  }
}

// The chunk again from its true state: squares summed per hop.  part[(r nch + k) 3 + j] belongs to hop (k kFxChunk) / h + j;
// samples behind the row's last whole hop are not counted.
__global__ void fx_kw_energy_kernel(FxKWeight kw, const float* __restrict__ x, const int* __restrict__ len, long ld, int nch,
                                    int h, const FxState4* __restrict__ init, double* __restrict__ part) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (k >= nch || (long)k * kFxChunk >= len[r]) return;
  const long first = (long)k * kFxChunk;
  const long end = min(first + kFxChunk, (long)(len[r] / h) * h);        // exclusive; may lie in front of the chunk
  const float4* p = reinterpret_cast<const float4*>(x + (long)r * ld + first);
  const FxState4 s0 = init[(long)r * nch + k];
  double st[4] = {s0.s[0], s0.s[1], s0.s[2], s0.s[3]};
  double acc = 0.0, out[3] = {0.0, 0.0, 0.0};
  int j = 0;
  long left = h - first % h;                                             // samples until the hop in progress is full
  const int cnt = (int)max(0L, end - first);
  for (int i = 0; i < cnt; i += 4) {
    const float4 v = p[i / 4];
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u < cnt) {
        const double y = fx_kw_step(kw, (double)e[u], st);
        acc = fma(y, y, acc);
        if (--left == 0) {
          out[j < 2 ? j : 2] = acc;          // h >= 800: a chunk touches at most three hops
          ++j, acc = 0.0, left = h;
        }
      }
    }
  }
  if (j < 3) out[j] = acc;
  double* o = part + ((long)r * nch + k) * 3;
  o[0] = out[0], o[1] = out[1], o[2] = out[2];
}

// fixed tree over the 256 lanes
__device__ inline void fx_fold256(double* sh_v, int* sh_n, double& v, int& n) {
  const int t = threadIdx.x;
  sh_v[t] = v, sh_n[t] = n;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) sh_v[t] += sh_v[t + off], sh_n[t] += sh_n[t + off];
    __syncthreads();
  }
  v = sh_v[0], n = sh_n[0];
  __syncthreads();
}

// One workgroup per item: hop sums from the partials, block energies, both gates.
__global__ void __launch_bounds__(256) fx_gate_kernel(const double* __restrict__ part, const int* __restrict__ len, int C, int nch,
                                                      int h, long nhop_ld, double* __restrict__ hops, double* __restrict__ zbuf,
                                                      double* __restrict__ lufs, float* __restrict__ mom, long mom_ld) {
  __shared__ double sh_v[256];
  __shared__ int sh_n[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const long n = len[b * C], nh = n / h, nb = nh - 3;
  if (nb < 1) {
    if (t == 0) lufs[b] = -INFINITY;
    return;
  }
  for (int c = 0; c < C; ++c) {
    const long r = (long)b * C + c;
    for (long k = t; k < nh; k += 256) {
      const long c0 = k * h / kFxChunk, c1 = ((k + 1) * h - 1) / kFxChunk;
      double sum = 0.0;
      for (long kc = c0; kc <= c1; ++kc) sum += part[(r * nch + kc) * 3 + (k - kc * kFxChunk / h)];
      hops[r * nhop_ld + k] = sum;
    }
  }
  __syncthreads();
  double* zb = zbuf + (long)b * nhop_ld;
  double acc = 0.0;
  int cnt = 0;
  for (long j = t; j < nb; j += 256) {
    const double z = fx_block_z(hops + (long)b * C * nhop_ld + j, nhop_ld, C, h);
    const double l = fx_lufs(z);
    zb[j] = z;
    if (mom) mom[(long)b * mom_ld + j] = (float)l;
    if (l > -70.0) acc += z, ++cnt;
  }
  fx_fold256(sh_v, sh_n, acc, cnt);
  if (cnt == 0) {
    if (t == 0) lufs[b] = -INFINITY;
    return;
  }
  const double gamma = fx_lufs(acc / cnt) - 10.0;
  acc = 0.0, cnt = 0;
  for (long j = t; j < nb; j += 256) {
    const double z = zb[j], l = fx_lufs(z);
    if (l > -70.0 && l > gamma) acc += z, ++cnt;
  }
  fx_fold256(sh_v, sh_n, acc, cnt);
  if (t == 0) lufs[b] = cnt ? fx_lufs(acc / cnt) : -INFINITY;
}

namespace {
struct LoudScratch {
  FxState4 *z, *init;
  double *part, *hops, *zbuf;
};
long fx_nhop_ld(long ld, int sr) { return ld / (sr / 10) + 1; }
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
LoudScratch fx_loud_carve(void* scratch, int B, int C, long ld, int sr) {
  const size_t R = (size_t)B * C, nch = (size_t)(ld / kFxChunk), nhop = (size_t)fx_nhop_ld(ld, sr);
  char* q = static_cast<char*>(scratch);
  LoudScratch L{};
  L.z = reinterpret_cast<FxState4*>(q), q += up256(R * nch * sizeof(FxState4));
  L.init = reinterpret_cast<FxState4*>(q), q += up256(R * nch * sizeof(FxState4));
  L.part = reinterpret_cast<double*>(q), q += up256(R * nch * 3 * sizeof(double));
  L.hops = reinterpret_cast<double*>(q), q += up256(R * nhop * sizeof(double));
  L.zbuf = reinterpret_cast<double*>(q);
  return L;
}
}  // namespace

size_t fx_loudness_scratch_bytes(int B, int C, long ld, int sr) {
  const size_t R = (size_t)B * C, nch = (size_t)(ld / kFxChunk), nhop = (size_t)fx_nhop_ld(ld, sr);
  return 2 * up256(R * nch * sizeof(FxState4)) + up256(R * nch * 3 * sizeof(double)) + up256(R * nhop * sizeof(double)) +
         up256((size_t)B * nhop * sizeof(double));
}

void launch_fx_loudness(const FxKWeight& k, const float* rows, const int* len, int B, int C, long ld, int sr, void* scratch,
                        double* lufs, float* mom, long mom_ld, hipStream_t s, hipEvent_t* ev) {
  const int nch = (int)(ld / kFxChunk), R = B * C, h = sr / 10;
  const LoudScratch L = fx_loud_carve(scratch, B, C, ld, sr);
  // M: what a chunk of zeros does to the four states, column by column
  FxMat4 M{};
  for (int col = 0; col < 4; ++col) {
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    st[col] = 1.0;
    for (int i = 0; i < kFxChunk; ++i) fx_kw_step(k, 0.0, st);
    for (int i = 0; i < 4; ++i) M.m[i][col] = st[i];
  }
  const dim3 grid((nch + 63) / 64, R);
  hipLaunchKernelGGL(fx_kw_local_kernel, grid, dim3(64), 0, s, k, rows, len, ld, nch, L.z);
  if (ev) RVCX_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(fx_kw_carry_kernel, dim3(R), dim3(256), 0, s, M, L.z, len, nch, L.init);
  if (ev) RVCX_HIP(hipEventRecord(ev[1], s));
  hipLaunchKernelGGL(fx_kw_energy_kernel, grid, dim3(64), 0, s, k, rows, len, ld, nch, h, L.init, L.part);
  if (ev) RVCX_HIP(hipEventRecord(ev[2], s));
  hipLaunchKernelGGL(fx_gate_kernel, dim3(B), dim3(256), 0, s, L.part, len, C, nch, h, fx_nhop_ld(ld, sr), L.hops, L.zbuf, lufs,
                     mom, mom_ld);
  if (ev) RVCX_HIP(hipEventRecord(ev[3], s));
}

// ---- true peak ----------------------------------------------------------------------------------------------------------------
constexpr int kTpTile = 1024;
__global__ void __launch_bounds__(256) fx_truepeak_kernel(FxTpTaps taps, const float* __restrict__ rows, const int* __restrict__ len,
                                                          int C, long ld, float* __restrict__ p, uint32_t* __restrict__ peak) {
  __shared__ __attribute__((aligned(16))) float sh[kTpTile + 32];
  const int b = blockIdx.y, t = threadIdx.x;
  const long n = len[b * C], base = (long)blockIdx.x * kTpTile;
  if (base >= n) return;
  float pm[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const float* xr = rows + ((long)b * C + c) * ld;
    // sh[i] = x[base - 12 + i], zero outside the signal
    for (int i = t; i < kTpTile + 28; i += 256) {
      const long g = base - 12 + i;
      sh[i] = (g >= 0 && g < n) ? xr[g] : 0.f;
    }
    __syncthreads();
    float w[28];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(sh + 4 * t + 4 * i);
      w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // sample base + 4 t + u sits at w[u + 12]; x[n + 12] at w[u + 24]
      float m = fabsf(w[u + 12]);
#pragma unroll
      for (int ph = 0; ph < 3; ++ph) m = fmaxf(m, fabsf(fx_tp_phase(w + u + 24, taps.h[ph])));
      pm[u] = fmaxf(pm[u], m);
    }
    __syncthreads();
  }
  float top = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long g = base + 4 * t + u;
    if (g < n) {
      top = fmaxf(top, pm[u]);
      if (p) p[(long)b * ld + g] = pm[u];
    }
  }
  for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off));
  // One atomic per workgroup, and only when it can raise the item's word: all workgroups of an item meet at one address, and
  // read-modify-writes on one cache line follow each other in L2 (2.6 ms of a 64 x 30 s batch when every wave sent one).
  // The plain look may see an older, smaller value -- then the atomic is sent needlessly, never wrongly.
  if ((t & 63) == 0) sh[t >> 6] = top;          // sh is free: the barrier behind the last channel has passed
  __syncthreads();
  if (t == 0) {
    top = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    const uint32_t bits = __float_as_uint(top);
    if (bits > __atomic_load_n(peak + b, __ATOMIC_RELAXED)) atomicMax(peak + b, bits);
  }
}

void launch_fx_truepeak(const float* rows, const int* len, int B, int C, long ld, float* p, uint32_t* peak, hipStream_t s) {
  RVCX_HIP(hipMemsetAsync(peak, 0, (size_t)B * sizeof(uint32_t), s));
  hipLaunchKernelGGL(fx_truepeak_kernel, dim3((unsigned)((ld + kTpTile - 1) / kTpTile), B), dim3(256), 0, s, fx_tp_taps(), rows,
                     len, C, ld, p, peak);
}

// ---- limiter ------------------------------------------------------------------------------------------------------------------
// u = 1 - min r[n .. n + W], rounded up (0 behind the item's end): r into LDS with W samples behind the tile, windows doubled until
// two of them cover W + 1
__global__ void __launch_bounds__(256) fx_slidemin_kernel(const float* __restrict__ p, const int* __restrict__ ilen, long ld,
                                                          float c, int W, float* __restrict__ u) {
  extern __shared__ float lds[];
  const int b = blockIdx.y, t = threadIdx.x, tot = kTpTile + W;
  const long n = ilen[b], base = (long)blockIdx.x * kTpTile;
  float* a = lds;
  float* o = lds + tot;
  for (int i = t; i < tot; i += 256) {
    const long g = base + i;
    a[i] = g < n ? fminf(1.f, c / p[(long)b * ld + g]) : 1.f;
  }
  __syncthreads();
  int span = 1;
  for (; 2 * span <= W + 1; span *= 2) {
    for (int i = t; i < tot; i += 256) o[i] = fminf(a[i], a[min(i + span, tot - 1)]);
    __syncthreads();
    float* q = a;
    a = o, o = q;
  }
  for (int i = t; i < kTpTile; i += 256) {
    const long g = base + i;
    if (g < ld) u[(long)b * ld + g] = g < n ? fx_one_minus_up(fminf(a[i], a[i + W + 1 - span])) : 0.f;
  }
}

// s[n] = mean of q[n - W .. n], q = 1 - e, an index below 0 taking q[0]; the smallest s of an item
__global__ void __launch_bounds__(256) fx_boxmean_kernel(const float* __restrict__ e, const int* __restrict__ ilen, long ld, int W,
                                                         float* __restrict__ sgain, uint32_t* __restrict__ smin) {
  extern __shared__ float lds[];
  const int b = blockIdx.y, t = threadIdx.x, tot = kTpTile + W;
  const long n = ilen[b], base = (long)blockIdx.x * kTpTile;
  if (base >= n) return;
  for (int i = t; i < tot; i += 256) {
    const long g = max(0L, base - W + i);                  // lds[i] = q[base - W + i]
    lds[i] = g < n ? FX_SUB(1.f, e[(long)b * ld + g]) : 1.f;
  }
  __syncthreads();
  float low = 1.f;
  const double div = (double)(W + 1);
  for (int i = t; i < kTpTile; i += 256) {
    if (base + i >= n) break;
    double sum = 0.0;
    for (int k = 0; k <= W; ++k) sum += (double)lds[i + k];
    const float sv = (float)(sum / div);
    sgain[(long)b * ld + base + i] = sv;
    low = fminf(low, sv);
  }
  for (int off = 32; off > 0; off >>= 1) low = fminf(low, __shfl_xor(low, off));
  if ((t & 63) == 0 && __float_as_uint(low) < __atomic_load_n(smin + b, __ATOMIC_RELAXED))      // as the true peak's max
    atomicMin(smin + b, __float_as_uint(low));
}

__global__ void fx_fill_u32_kernel(uint32_t* dst, uint32_t v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = v;
}

int launch_fx_limit_gain(const float* p, const int* ilen, const int* ilen_host, int B, long ld, float c, int W, float c_rel,
                         float* u, float* e, float* state, float* sgain, uint32_t* smin, hipStream_t s) {
  RVCX_CHECK(W >= 0 && W <= kFxMaxLookahead, "limiter lookahead exceeds the LDS plan");
  const dim3 grid((unsigned)(ld / kTpTile), B);           // ld is a multiple of kFxChunk = kTpTile
  const size_t tot = (size_t)(kTpTile + W) * sizeof(float);
  hipLaunchKernelGGL(fx_fill_u32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, smin, 0x3f800000u, B);
  hipLaunchKernelGGL(fx_slidemin_kernel, grid, dim3(256), 2 * tot, s, p, ilen, ld, c, W, u);
  const int passes = launch_fx_follower(u, e, ilen, ilen_host, B, ld, 0, 0, 0.f, c_rel, state, s);
  hipLaunchKernelGGL(fx_boxmean_kernel, grid, dim3(256), tot, s, e, ilen, ld, W, sgain, smin);
  return passes;
}

__global__ void fx_limit_apply_kernel(const float* rows, const float* __restrict__ sgain, const int* __restrict__ len,
                                      int C, long ld, float* y, float* __restrict__ stage, int16_t* __restrict__ pcm) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= len[b * C]) return;
  const float g = sgain ? sgain[(long)b * ld + i] : 1.f;
  for (int c = 0; c < C; ++c) {
    const long r = ((long)b * C + c) * ld + i, q = ((long)b * ld + i) * C + c;
    const float v = FX_MUL(rows[r], g);
    if (y) y[r] = v;
    if (stage) stage[q] = v;
    if (pcm) pcm[q] = fx_pcm16(v);
  }
}

void launch_fx_limit_apply(const float* rows, const float* sgain, const int* len, int B, int C, long ld, float* y, float* stage,
                           int16_t* pcm, hipStream_t s) {
  hipLaunchKernelGGL(fx_limit_apply_kernel, dim3((unsigned)((ld + 255) / 256), B), dim3(256), 0, s, rows, sgain, len, C, ld, y,
                     stage, pcm);
}

__global__ void fx_master_mix_kernel(float* __restrict__ v, const float* __restrict__ inst, const int* __restrict__ len_v,
                                     const int* __restrict__ len_i, const float* __restrict__ gv, const float* __restrict__ gi,
                                     int C, long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y, b = r / C;
  if (i >= len_v[r]) return;
  const long q = (long)r * ld + i;
  const float a = FX_MUL(gv[b], v[q]), m = i < len_i[r] ? FX_MUL(gi[b], inst[q]) : 0.f;
  v[q] = a + m;
}

void launch_fx_master_mix(float* v, const float* inst, const int* len_v, const int* len_i, const float* gv, const float* gi, int B,
                          int C, long ld, hipStream_t s) {
  hipLaunchKernelGGL(fx_master_mix_kernel, dim3((unsigned)((ld + 255) / 256), B * C), dim3(256), 0, s, v, inst, len_v, len_i, gv,
                     gi, C, ld);
}

__global__ void fx_scale_kernel(float* __restrict__ rows, const float* __restrict__ g, int C, long ld) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int r = blockIdx.y;
  if (i >= ld) return;
  const float k = g[r / C];
  float4* q = reinterpret_cast<float4*>(rows + (long)r * ld + i);
  float4 v = *q;
  v.x = FX_MUL(k, v.x), v.y = FX_MUL(k, v.y), v.z = FX_MUL(k, v.z), v.w = FX_MUL(k, v.w);
  *q = v;
}

void launch_fx_scale(float* rows, const float* g, int B, int C, long ld, hipStream_t s) {
  hipLaunchKernelGGL(fx_scale_kernel, dim3((unsigned)((ld / 4 + 255) / 256), B * C), dim3(256), 0, s, rows, g, C, ld);
}

// ---- host twins: sequentially, in the order rvcx.h defines ---------------------------------------------------------------------
double fx_loudness_host(const FxKWeight& k, const float* x, long n, int C, int sr, float* mom) {
  const long h = sr / 10, nh = n / h, nb = nh - 3;
  if (nb < 1) return -INFINITY;
  std::vector<double> hop((size_t)C * nh);
  for (int c = 0; c < C; ++c) {
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    for (long q = 0; q < nh; ++q) {
      double acc = 0.0;
      for (long i = q * h; i < (q + 1) * h; ++i) {
        const double y = fx_kw_step(k, (double)x[i * C + c], st);
        acc = fma(y, y, acc);
      }
      hop[(size_t)c * nh + q] = acc;
    }
  }
  std::vector<double> z((size_t)nb);
  double acc = 0.0;
  long cnt = 0;
  for (long j = 0; j < nb; ++j) {
    z[j] = fx_block_z(hop.data() + j, nh, C, h);
    const double l = fx_lufs(z[j]);
    if (mom) mom[j] = (float)l;
    if (l > -70.0) acc += z[j], ++cnt;
  }
  if (!cnt) return -INFINITY;
  const double gamma = fx_lufs(acc / cnt) - 10.0;
  acc = 0.0, cnt = 0;
  for (long j = 0; j < nb; ++j) {
    const double l = fx_lufs(z[j]);
    if (l > -70.0 && l > gamma) acc += z[j], ++cnt;
  }
  return cnt ? fx_lufs(acc / cnt) : -INFINITY;
}

float fx_truepeak_host(const float* x, long n, int C, float* p) {
  const FxTpTaps& taps = fx_tp_taps();
  float top = 0.f;
  for (long i = 0; i < n; ++i) {
    float m = 0.f;
    for (int c = 0; c < C; ++c) {
      float w[kTpTaps];                          // w[23 - j] = x[i + 12 - j]
      for (int j = 0; j < kTpTaps; ++j) {
        const long g = i + 12 - j;
        w[kTpTaps - 1 - j] = (g >= 0 && g < n) ? x[g * C + c] : 0.f;
      }
      m = fmaxf(m, fabsf(x[i * C + c]));
      for (int ph = 0; ph < 3; ++ph) m = fmaxf(m, fabsf(fx_tp_phase(w + kTpTaps - 1, taps.h[ph])));
    }
    if (p) p[i] = m;
    top = fmaxf(top, m);
  }
  return top;
}

void fx_limit_gain_host(const float* p, long n, float c, int W, float c_rel, float* sgain) {
  if (n <= 0) return;
  std::vector<float> u((size_t)n), e((size_t)n);
  for (long i = 0; i < n; ++i) {
    float g = 1.f;
    for (long k = i; k <= i + W && k < n; ++k) g = fminf(g, fminf(1.f, c / p[k]));
    u[i] = fx_one_minus_up(g);
  }
  fx_follower_host(u.data(), n, 0, 0, 0.f, c_rel, e.data());
  for (long i = 0; i < n; ++i) {
    double sum = 0.0;
    for (long k = i - W; k <= i; ++k) sum += (double)(1.f - e[k < 0 ? 0 : k]);
    sgain[i] = (float)(sum / (double)(W + 1));
  }
}

double fx_db20(float peak) { return peak > 0.f ? 20.0 * std::log10((double)peak) : -INFINITY; }
double fx_gain_to(double target, double L) { return std::isfinite(L) ? std::pow(10.0, (target - L) / 20.0) : 1.0; }

// stage 11 on one interleaved item, sequentially; returns max p (the true peak in front of the stage) and min s
void fx_limit_host(const float* x, long n, int C, int sr, double ceiling_db, double lookahead_ms, double release_ms, float* y,
                   float* gain, float* peak_out, float* smin_out) {
  std::vector<float> p((size_t)std::max<long>(n, 1)), sg((size_t)std::max<long>(n, 1), 1.f);
  const float peak = fx_truepeak_host(x, n, C, p.data()), c = (float)std::pow(10.0, ceiling_db / 20.0);
  float low = 1.f;
  if (peak <= c) {                             // skip: the input, bit for bit
    if (y != x) std::copy(x, x + n * C, y);
  } else {
    fx_limit_gain_host(p.data(), n, c, fx_lookahead(sr, lookahead_ms), fx_cte(release_ms, sr), sg.data());
    for (long i = 0; i < n; ++i) {
      low = std::min(low, sg[i]);
      for (int ch = 0; ch < C; ++ch) y[i * C + ch] = x[i * C + ch] * sg[i];
    }
  }
  if (gain) std::copy(sg.begin(), sg.begin() + n, gain);
  if (peak_out) *peak_out = peak;
  if (smin_out) *smin_out = low;
}

// stage 12 on one cover, sequentially
void fx_master_host(const float* vocal, long n_v, const float* inst, long n_i, int sr, double target_lufs, double vocal_offset_lu,
                    double ceiling_dbtp, int16_t* out, double* report7) {
  const long nv = (long)n_v, ni = (long)std::min(n_i, n_v);
  const FxKWeight kw = fx_kweight(sr);
  const double Lv = fx_loudness_host(kw, vocal, nv, 2, sr, nullptr), Li = fx_loudness_host(kw, inst, ni, 2, sr, nullptr);
  const float gv = (float)fx_gain_to(target_lufs + vocal_offset_lu, Lv), gi = (float)fx_gain_to(target_lufs, Li);
  std::vector<float> m((size_t)nv * 2 + 2), y((size_t)nv * 2 + 2);
  for (long i = 0; i < nv * 2; ++i) {
    const float a = gv * vocal[i], b = i < ni * 2 ? gi * inst[i] : 0.f;
    m[i] = a + b;
  }
  const double Lm = fx_loudness_host(kw, m.data(), nv, 2, sr, nullptr);
  const float gm = (float)fx_gain_to(target_lufs, Lm);
  for (long i = 0; i < nv * 2; ++i) m[i] = gm * m[i];
  float peak = 0.f, low = 1.f;
  fx_limit_host(m.data(), nv, 2, sr, ceiling_dbtp, 2.0, 100.0, y.data(), nullptr, &peak, &low);
  for (long i = 0; i < nv * 2; ++i) out[i] = fx_pcm16(y[i]);
  if (report7) {
    report7[0] = Lv, report7[1] = Li, report7[2] = Lm, report7[3] = fx_loudness_host(kw, y.data(), nv, 2, sr, nullptr);
    report7[4] = fx_db20(peak), report7[5] = fx_db20(fx_truepeak_host(y.data(), nv, 2, nullptr)), report7[6] = (double)low;
  }
}

}  // namespace rvcx
