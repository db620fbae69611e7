// Post-production kernels (include/rvcx.h "post-production"): every stage of the reference's effects board is a
// recurrence in time; each family is cut so that many lanes can walk it.
//
//  * Linear stages (high-pass, shelves): the state after a chunk is affine in the state before it, s' = M s + z with the
//    same M = A^L for every chunk.  Lane = chunk: zero-state run (z), one carry scan per row in double, the run again from
//    the true state.
//  * Envelope followers: a step is a monotone contraction of the state but not linear.  Lane = chunk, every chunk starts
//    from a guess; a chunk is run again while its initial state differs from its predecessor's final state.  When no chunk
//    changed the result is the sequential one bit for bit (induction from chunk 0, whose state 0 is no guess); pass k
//    settles at least chunk k.  Every rounding of a step is one IEEE operation, the same on host and device.
//  * Comb, all-pass, chorus with feedback: the recurrence reaches back D samples, so D consecutive samples are independent
//    and the blocks of D follow each other.  One wave per (item, side, comb) / (item, side) / row.  The comb's damping
//    one-pole runs through the block: it is a 64-lane scan of affine maps.
#include "effects.h"

#include <algorithm>
#include <cmath>

#include "common.h"
#include "effects_device.h"

// every rounding below is written out: nothing may be fused behind the source's back, on either side
#pragma clang fp contract(off)

namespace rvcx {

// ---- coefficients (host, double, rounded once) ----------------------------------------------------------------------------
FxBiquad fx_coeffs(int kind, int sr, double fc, double Q, double gain_db) {
  FxBiquad q{};
  if (kind == 0) {
    const double k = std::tan(M_PI * fc / sr), b0 = 1.0 / (k + 1.0);
    q.b0 = (float)b0, q.b1 = (float)-b0, q.a1 = (float)((k - 1.0) / (k + 1.0));
    return q;
  }
  const double A = std::pow(10.0, gain_db / 40.0), w = 2.0 * M_PI * fc / sr, cs = std::cos(w);
  const double beta = std::sin(w) * std::sqrt(A) / Q;
  double b0, b1, b2, a0, a1, a2;
  if (kind == 1) {
    b0 = A * ((A + 1) - (A - 1) * cs + beta), b1 = 2 * A * ((A - 1) - (A + 1) * cs), b2 = A * ((A + 1) - (A - 1) * cs - beta);
    a0 = (A + 1) + (A - 1) * cs + beta, a1 = -2 * ((A - 1) + (A + 1) * cs), a2 = (A + 1) + (A - 1) * cs - beta;
  } else {
    b0 = A * ((A + 1) + (A - 1) * cs + beta), b1 = -2 * A * ((A - 1) + (A + 1) * cs), b2 = A * ((A + 1) + (A - 1) * cs - beta);
    a0 = (A + 1) - (A - 1) * cs + beta, a1 = 2 * ((A - 1) - (A + 1) * cs), a2 = (A + 1) - (A - 1) * cs - beta;
  }
  q.b0 = (float)(b0 / a0), q.b1 = (float)(b1 / a0), q.b2 = (float)(b2 / a0), q.a1 = (float)(a1 / a0), q.a2 = (float)(a2 / a0);
  return q;
}

float fx_cte(double ms, int sr) { return ms < 1e-3 ? 0.f : (float)std::exp(-2.0 * M_PI * 1000.0 / (ms * sr)); }

FxReverb fx_reverb_setup(int sr, double room, double damping, double wet, double dry, double width) {
  static const int kComb[8] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, kAp[4] = {556, 441, 341, 225};
  FxReverb r{};
  for (int side = 0; side < 2; ++side) {
    for (int i = 0; i < 8; ++i) r.comb[side][i] = fx_delay(sr, kComb[i] + 23 * side);
    for (int i = 0; i < 4; ++i) r.ap[side][i] = fx_delay(sr, kAp[i] + 23 * side);
  }
  const double d = 0.4 * damping;
  r.fb = (float)(0.28 * room + 0.7), r.d = (float)d, r.omd = (float)(1.0 - d);
  r.w1 = (float)(1.5 * wet * (1.0 + width)), r.w2 = (float)(1.5 * wet * (1.0 - width)), r.dry2 = (float)(2.0 * dry);
  return r;
}

FxChorus fx_chorus_setup(int sr, double rate, double depth, double centre_ms, double feedback, double mix) {
  FxChorus c{};
  c.w = 2.0 * M_PI * rate / sr, c.srk = sr / 1000.0, c.centre = centre_ms, c.dep10 = 10.0 * depth;
  c.fb = (float)feedback, c.mix = (float)mix, c.omm = (float)(1.0 - mix);
  c.T = (int)std::floor(c.srk * std::max(1.0, centre_ms - std::fabs(c.dep10))) - 1;
  return c;
}

// ---- layout -----------------------------------------------------------------------------------------------------------------
__global__ void fx_deinterleave_kernel(const float* __restrict__ stage, float* __restrict__ rows, const int* __restrict__ len,
                                       int C, long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= ld) return;
  const bool in = i < len[b * C];
  for (int c = 0; c < C; ++c) rows[((long)b * C + c) * ld + i] = in ? stage[((long)b * ld + i) * C + c] : 0.f;
}

__global__ void fx_interleave_kernel(const float* __restrict__ rows, float* __restrict__ stage, const int* __restrict__ len,
                                     int C, long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= len[b * C]) return;
  for (int c = 0; c < C; ++c) stage[((long)b * ld + i) * C + c] = rows[((long)b * C + c) * ld + i];
}

void launch_fx_deinterleave(const float* stage, float* rows, const int* len, int B, int C, long ld, hipStream_t s) {
  hipLaunchKernelGGL(fx_deinterleave_kernel, dim3((unsigned)((ld + 255) / 256), B), dim3(256), 0, s, stage, rows, len, C, ld);
}
void launch_fx_interleave(const float* rows, float* stage, const int* len, int B, int C, long ld, hipStream_t s) {
  hipLaunchKernelGGL(fx_interleave_kernel, dim3((unsigned)((ld + 255) / 256), B), dim3(256), 0, s, rows, stage, len, C, ld);
}

// ---- linear stages ----------------------------------------------------------------------------------------------------------
// the state a chunk leaves behind when it starts from zero
__global__ void fx_bq_local_kernel(FxBiquad q, const float* __restrict__ x, const int* __restrict__ len, long ld, int nch,
                                   float2* __restrict__ z) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (k >= nch || (long)k * kFxChunk >= len[r]) return;
  const float4* p = reinterpret_cast<const float4*>(x + (long)r * ld + (long)k * kFxChunk);
  float s1 = 0.f, s2 = 0.f;
  for (int i = 0; i < kFxChunk / 4; ++i) {
    const float4 v = p[i];
    fx_bq_step(q, v.x, s1, s2);
    fx_bq_step(q, v.y, s1, s2);
    fx_bq_step(q, v.z, s1, s2);
    fx_bq_step(q, v.w, s1, s2);
  }
  z[(long)r * nch + k] = make_float2(s1, s2);
}

struct FxMat2 {
  double a, b, c, d;
};
__device__ inline void fx_apply(const FxMat2& m, double& s1, double& s2, double z1, double z2) {
  const double t1 = fma(m.a, s1, fma(m.b, s2, z1)), t2 = fma(m.c, s1, fma(m.d, s2, z2));
  s1 = t1, s2 = t2;
}

// One workgroup per row: s[k + 1] = M s[k] + z[k] over the row's chunks.  Lane t folds a run of chunks from zero, lane 0
// walks the 256 runs, every lane replays its run from the state it was handed and writes the chunks' initial states.
__global__ void __launch_bounds__(256) fx_bq_carry_kernel(FxMat2 M, const float2* __restrict__ z, const int* __restrict__ len,
                                                          int nch_ld, float2* __restrict__ init) {
  __shared__ double sh[256][6];
  const int r = blockIdx.x, t = threadIdx.x;
  const int nch = (len[r] + kFxChunk - 1) / kFxChunk;
  const int seg = (nch + 255) / 256;
  const int k0 = min(t * seg, nch), k1 = min(k0 + seg, nch);
  const float2* zr = z + (long)r * nch_ld;
  double s1 = 0.0, s2 = 0.0;
  FxMat2 P{1.0, 0.0, 0.0, 1.0};
  for (int k = k0; k < k1; ++k) {
    fx_apply(M, s1, s2, (double)zr[k].x, (double)zr[k].y);
    const FxMat2 Q{M.a * P.a + M.b * P.c, M.a * P.b + M.b * P.d, M.c * P.a + M.d * P.c, M.c * P.b + M.d * P.d};
    P = Q;
  }
  sh[t][0] = P.a, sh[t][1] = P.b, sh[t][2] = P.c, sh[t][3] = P.d, sh[t][4] = s1, sh[t][5] = s2;
  __syncthreads();
  if (t == 0) {
    double c1 = 0.0, c2 = 0.0;
    for (int j = 0; j < 256; ++j) {
      const FxMat2 Pj{sh[j][0], sh[j][1], sh[j][2], sh[j][3]};
      const double z1 = sh[j][4], z2 = sh[j][5];
      sh[j][4] = c1, sh[j][5] = c2;
      fx_apply(Pj, c1, c2, z1, z2);
    }
  }
  __syncthreads();
  s1 = sh[t][4], s2 = sh[t][5];
  for (int k = k0; k < k1; ++k) {
    init[(long)r * nch_ld + k] = make_float2((float)s1, (float)s2);
    fx_apply(M, s1, s2, (double)zr[k].x, (double)zr[k].y);
  }
}

__global__ void fx_bq_apply_kernel(FxBiquad q, const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ len,
                                   long ld, int nch, const float2* __restrict__ init) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (k >= nch || (long)k * kFxChunk >= len[r]) return;
  const long off = (long)r * ld + (long)k * kFxChunk;
  const float4* p = reinterpret_cast<const float4*>(x + off);
  float4* o = reinterpret_cast<float4*>(y + off);
  const float2 s0 = init[(long)r * nch + k];
  float s1 = s0.x, s2 = s0.y;
  for (int i = 0; i < kFxChunk / 4; ++i) {
    const float4 v = p[i];
    float4 w;
    w.x = fx_bq_step(q, v.x, s1, s2);
    w.y = fx_bq_step(q, v.y, s1, s2);
    w.z = fx_bq_step(q, v.z, s1, s2);
    w.w = fx_bq_step(q, v.w, s1, s2);
    o[i] = w;
  }
}

void launch_fx_biquad(const FxBiquad& q, const float* x, float* y, const int* len, int R, long ld, float* scratch,
                      hipStream_t s) {
  const int nch = (int)(ld / kFxChunk);
  float2* z = reinterpret_cast<float2*>(scratch);
  float2* init = z + (size_t)R * nch;
  // M = A^L, A = [[-a1, 1], [-a2, 0]]: what a chunk of zeros does to the state
  double m[4] = {1, 0, 0, 1}, a[4] = {-(double)q.a1, 1.0, -(double)q.a2, 0.0};
  for (int L = kFxChunk; L > 0; L >>= 1) {
    if (L & 1) {
      const double t[4] = {a[0] * m[0] + a[1] * m[2], a[0] * m[1] + a[1] * m[3], a[2] * m[0] + a[3] * m[2], a[2] * m[1] + a[3] * m[3]};
      std::copy(t, t + 4, m);
    }
    const double t[4] = {a[0] * a[0] + a[1] * a[2], a[0] * a[1] + a[1] * a[3], a[2] * a[0] + a[3] * a[2], a[2] * a[1] + a[3] * a[3]};
    std::copy(t, t + 4, a);
  }
  const dim3 grid((nch + 63) / 64, R);
  hipLaunchKernelGGL(fx_bq_local_kernel, grid, dim3(64), 0, s, q, x, len, ld, nch, z);
  hipLaunchKernelGGL(fx_bq_carry_kernel, dim3(R), dim3(256), 0, s, FxMat2{m[0], m[1], m[2], m[3]}, z, len, nch, init);
  hipLaunchKernelGGL(fx_bq_apply_kernel, grid, dim3(64), 0, s, q, x, y, len, ld, nch, init);
}

// ---- envelope followers -------------------------------------------------------------------------------------------------------
// One relaxation pass.  s_in: the state a chunk last started from; prev / next: the states the chunks left behind in the
// pass before / in this one.  A chunk whose predecessor's state is what it started from keeps its result.
__global__ void fx_follower_kernel(const float* __restrict__ x, float* __restrict__ env, const int* __restrict__ len, long ld,
                                   int nch, int square, int sqrt_out, float c_att, float c_rel, float* __restrict__ s_in,
                                   const float* __restrict__ prev, float* __restrict__ next, int first, int* __restrict__ changed) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (k >= nch || (long)k * kFxChunk >= len[r]) return;
  const long c = (long)r * nch + k;
  const float want = (first || k == 0) ? 0.f : prev[c - 1];
  if (!first && __float_as_uint(want) == __float_as_uint(s_in[c])) {
    next[c] = prev[c];
    return;
  }
  s_in[c] = want;
  const long off = (long)r * ld + (long)k * kFxChunk;
  const float4* p = reinterpret_cast<const float4*>(x + off);
  float4* o = reinterpret_cast<float4*>(env + off);
  float e = want;
  for (int i = 0; i < kFxChunk / 4; ++i) {
    const float4 v = p[i];
    float4 w;
    e = fx_follow_step(v.x, e, square, c_att, c_rel), w.x = sqrt_out ? FX_SQRT(e) : e;
    e = fx_follow_step(v.y, e, square, c_att, c_rel), w.y = sqrt_out ? FX_SQRT(e) : e;
    e = fx_follow_step(v.z, e, square, c_att, c_rel), w.z = sqrt_out ? FX_SQRT(e) : e;
    e = fx_follow_step(v.w, e, square, c_att, c_rel), w.w = sqrt_out ? FX_SQRT(e) : e;
    o[i] = w;
  }
  next[c] = e;
  *changed = 1;
}

int launch_fx_follower(const float* x, float* env, const int* len, const int* len_host, int R, long ld, int square,
                       int sqrt_out, float c_att, float c_rel, float* state, hipStream_t s) {
  const int nch = (int)(ld / kFxChunk);
  const size_t per = (size_t)R * nch;
  float* s_in = state;
  float* st[2] = {state + per, state + 2 * per};
  int* changed = reinterpret_cast<int*>(state + 3 * per);
  int most = 0;                                   // chunks of the longest row: the hard bound on the passes
  for (int r = 0; r < R; ++r) most = std::max(most, (len_host[r] + kFxChunk - 1) / kFxChunk);
  const dim3 grid((nch + 63) / 64, R);
  int passes = 0;
  for (int p = 1; p <= most; ++p) {
    RVCX_HIP(hipMemsetAsync(changed, 0, sizeof(int), s));
    hipLaunchKernelGGL(fx_follower_kernel, grid, dim3(64), 0, s, x, env, len, ld, nch, square, sqrt_out, c_att, c_rel, s_in,
                       st[p & 1], st[(p & 1) ^ 1], p == 1 ? 1 : 0, changed);
    if (p == most) {         // pass p settles chunk p - 1 at the latest: nothing is left to check
      passes = p;
      break;
    }
    int any = 0;
    RVCX_HIP(hipMemcpyAsync(&any, changed, sizeof(int), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));
    if (!any) break;
    passes = p;
  }
  return passes;
}

__global__ void fx_gain_kernel(const float* __restrict__ x, const float* __restrict__ env, float* __restrict__ y, long total,
                               int gate, float thr, float expo) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= total) return;
  const float4 v = *reinterpret_cast<const float4*>(x + i), e = *reinterpret_cast<const float4*>(env + i);
  float4 w;
  w.x = FX_MUL(v.x, fx_gain(e.x, gate, thr, expo));
  w.y = FX_MUL(v.y, fx_gain(e.y, gate, thr, expo));
  w.z = FX_MUL(v.z, fx_gain(e.z, gate, thr, expo));
  w.w = FX_MUL(v.w, fx_gain(e.w, gate, thr, expo));
  *reinterpret_cast<float4*>(y + i) = w;
}

void launch_fx_gain(const float* x, const float* env, float* y, int R, long ld, int gate, float thr, float expo, hipStream_t s) {
  const long total = (long)R * ld;      // ld is a multiple of 4 and the tails are zero
  hipLaunchKernelGGL(fx_gain_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, x, env, y, total, gate, thr, expo);
}

// ---- Freeverb -----------------------------------------------------------------------------------------------------------------
// One wave per (comb, item * 2 + side).  Lane l owns samples [l S, (l + 1) S) of every block of D; its slice of the delay
// line lives in LDS at [k][l] (no two lanes ever touch one word).  Per block: the damping one-pole from zero per lane, a
// scan over the lanes for the state each lane starts from, then the block itself.
__global__ void __launch_bounds__(64) fx_comb_kernel(FxReverb rv, const float* __restrict__ x, float* __restrict__ combs,
                                                     const int* __restrict__ len, long ld) {
  extern __shared__ float buf[];
  const int ci = blockIdx.x, is = blockIdx.y, b = is >> 1, side = is & 1, l = threadIdx.x;
  const int D = rv.comb[side][ci], S = (D + 63) / 64, n = len[2 * b];
  const float* xl = x + (long)(2 * b) * ld;
  const float* xr = xl + ld;
  float* out = combs + ((long)is * 8 + ci) * ld;
  const int cnt = max(0, min(S, D - l * S)), last_lane = (D - 1) / S;
  for (int k = 0; k < S; ++k) buf[k * 64 + l] = 0.f;
  float last = 0.f;
  for (int j0 = 0; j0 < n; j0 += D) {
    float m = 1.f, t = 0.f;
    for (int k = 0; k < cnt; ++k) {
      t = FX_FMA(t, rv.d, FX_MUL(buf[k * 64 + l], rv.omd));
      m = FX_MUL(m, rv.d);
    }
    // inclusive scan of the maps s -> m s + t in lane order
    for (int off = 1; off < 64; off <<= 1) {
      const float mp = __shfl_up(m, off), tp = __shfl_up(t, off);
      if (l >= off) {
        t = FX_FMA(m, tp, t);
        m = FX_MUL(m, mp);
      }
    }
    float me = __shfl_up(m, 1), te = __shfl_up(t, 1);
    if (l == 0) me = 1.f, te = 0.f;
    float s = FX_FMA(me, last, te);
    const int base = j0 + l * S;
    for (int k = 0; k < cnt; ++k) {
      const int i = base + k;
      const float o = buf[k * 64 + l];
      s = FX_FMA(s, rv.d, FX_MUL(o, rv.omd));
      float in = 0.f;
      if (i < n) {
        in = FX_MUL(0.015f, xl[i] + xr[i]);
        out[i] = o;
      }
      buf[k * 64 + l] = FX_FMA(s, rv.fb, in);
    }
    last = __shfl(s, last_lane);
  }
}

// One wave per (item, side): the eight comb outputs summed in order, then the four all-passes in series.  The shortest
// all-pass delay T bounds the block: inside it every sample reads what an earlier block wrote.
__global__ void __launch_bounds__(64) fx_allpass_kernel(FxReverb rv, const float* __restrict__ combs, float* __restrict__ ap,
                                                        const int* __restrict__ len, long ld) {
  extern __shared__ float buf[];
  const int is = blockIdx.x, b = is >> 1, side = is & 1, l = threadIdx.x, n = len[2 * b];
  int D[4], base[4], tot = 0, T = rv.ap[side][0];
  for (int q = 0; q < 4; ++q) {
    D[q] = rv.ap[side][q], base[q] = tot, tot += D[q];
    T = min(T, D[q]);
  }
  for (int i = l; i < tot; i += 64) buf[i] = 0.f;
  __syncthreads();
  const float* cb = combs + (long)is * 8 * ld;
  float* out = ap + (long)is * ld;
  for (int j0 = 0; j0 < n; j0 += T) {
    const int j1 = min(j0 + T, n);
    for (int i = j0 + l; i < j1; i += 64) {
      float in = cb[i];
      for (int c = 1; c < 8; ++c) in += cb[(long)c * ld + i];
      for (int q = 0; q < 4; ++q) {
        float* w = buf + base[q] + i % D[q];
        const float v = *w;
        *w = FX_FMA(0.5f, v, in);
        in = FX_SUB(v, in);
      }
      out[i] = in;
    }
    __syncthreads();
  }
}

__global__ void fx_reverb_mix_kernel(FxReverb rv, const float* __restrict__ x, const float* __restrict__ ap,
                                     float* __restrict__ y, const int* __restrict__ len, long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= len[2 * b]) return;
  const long l = (long)(2 * b) * ld + i, r = l + ld;
  const float ol = ap[l], orr = ap[r];
  y[l] = FX_FMA(ol, rv.w1, FX_FMA(orr, rv.w2, FX_MUL(rv.dry2, x[l])));
  y[r] = FX_FMA(orr, rv.w1, FX_FMA(ol, rv.w2, FX_MUL(rv.dry2, x[r])));
}

void launch_fx_reverb(const FxReverb& rv, const float* x, float* combs, float* ap, float* y, const int* len, int B, long ld,
                      hipStream_t s) {
  int dmax = 0, aptot = 0;
  for (int i = 0; i < 8; ++i) dmax = std::max(dmax, rv.comb[1][i]);
  for (int i = 0; i < 4; ++i) aptot += rv.ap[1][i];
  const size_t comb_lds = (size_t)((dmax + 63) / 64) * 64 * sizeof(float), ap_lds = (size_t)aptot * sizeof(float);
  RVCX_CHECK(comb_lds <= 48 * 1024 && ap_lds <= 48 * 1024, "reverb delay lines exceed the LDS plan");
  hipLaunchKernelGGL(fx_comb_kernel, dim3(8, 2 * B), dim3(64), comb_lds, s, rv, x, combs, len, ld);
  hipLaunchKernelGGL(fx_allpass_kernel, dim3(2 * B), dim3(64), ap_lds, s, rv, combs, ap, len, ld);
  hipLaunchKernelGGL(fx_reverb_mix_kernel, dim3((unsigned)((ld + 255) / 256), B), dim3(256), 0, s, rv, x, ap, y, len, ld);
}

// ---- chorus ---------------------------------------------------------------------------------------------------------------------
// feedback == 0: the delay line is the input, every sample is a gather
__global__ void fx_chorus_gather_kernel(FxChorus ch, const float* __restrict__ x, float* __restrict__ y,
                                        const int* __restrict__ len, long ld) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= len[r]) return;
  const float* xr = x + (long)r * ld;
  y[(long)r * ld + i] = FX_FMA(ch.mix, fx_chorus_tap(ch, xr, i), FX_MUL(ch.omm, xr[i]));
}

// One wave per row, blocks of T = floor(tau_min) - 1 samples: both interpolation neighbours of every sample of a block were
// written by earlier blocks.
__global__ void __launch_bounds__(64) fx_chorus_feedback_kernel(FxChorus ch, const float* __restrict__ x, float* __restrict__ d,
                                                                float* __restrict__ y, const int* __restrict__ len, long ld) {
  const int r = blockIdx.x, l = threadIdx.x, n = len[r];
  const float* xr = x + (long)r * ld;
  float* dr = d + (long)r * ld;
  float* yr = y + (long)r * ld;
  for (int j0 = 0; j0 < n; j0 += ch.T) {
    const int j1 = min(j0 + ch.T, n);
    for (int i = j0 + l; i < j1; i += 64) {
      const float w = fx_chorus_tap(ch, dr, i), xv = xr[i];
      dr[i] = FX_FMA(ch.fb, w, xv);
      yr[i] = FX_FMA(ch.mix, w, FX_MUL(ch.omm, xv));
    }
    __syncthreads();
  }
}

void launch_fx_chorus(const FxChorus& ch, const float* x, float* d, float* y, const int* len, int R, long ld, hipStream_t s) {
  if (ch.fb == 0.f) {
    hipLaunchKernelGGL(fx_chorus_gather_kernel, dim3((unsigned)((ld + 255) / 256), R), dim3(256), 0, s, ch, x, y, len, ld);
    return;
  }
  RVCX_CHECK(ch.T >= 1, "chorus block");
  hipLaunchKernelGGL(fx_chorus_feedback_kernel, dim3(R), dim3(64), 0, s, ch, x, d, y, len, ld);
}

// ---- mix ------------------------------------------------------------------------------------------------------------------------
__global__ void fx_mix_kernel(const int16_t* __restrict__ v, long nv, const int16_t* __restrict__ inst, long ni, double gv,
                              double gi, int16_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  out[i] = fx_mix_sample(v[i], i < ni ? inst[i] : 0, gv, gi);
}

void launch_fx_mix(const int16_t* v, long nv, const int16_t* inst, long ni, double gv, double gi, int16_t* out, hipStream_t s) {
  if (nv <= 0) return;
  hipLaunchKernelGGL(fx_mix_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, v, nv, inst, ni, gv, gi, out);
}

// ---- host twins: each stage sequentially, float32, in the order rvcx.h defines -----------------------------------------------
void fx_highpass_host(const FxBiquad& q, const float* x, long n, float* y) {
  float xp = 0.f, yp = 0.f;
  for (long i = 0; i < n; ++i) {
    const float xv = x[i];
    yp = fmaf(q.b0, xv, fmaf(q.b1, xp, -q.a1 * yp));
    xp = xv;
    y[i] = yp;
  }
}

void fx_biquad_host(const FxBiquad& q, const float* x, long n, float* y) {
  float s1 = 0.f, s2 = 0.f;
  for (long i = 0; i < n; ++i) y[i] = fx_bq_step(q, x[i], s1, s2);
}

void fx_follower_host(const float* x, long n, int square, int sqrt_out, float c_att, float c_rel, float* env) {
  float e = 0.f;
  for (long i = 0; i < n; ++i) {
    e = fx_follow_step(x[i], e, square, c_att, c_rel);
    env[i] = sqrt_out ? sqrtf(e) : e;
  }
}

void fx_gain_host(const float* x, const float* env, long n, int gate, float thr, float expo, float* y) {
  for (long i = 0; i < n; ++i) y[i] = x[i] * fx_gain(env[i], gate, thr, expo);
}

void fx_comb_host(const float* in, long n, int D, float fb, float d, float* out) {
  std::vector<float> buf((size_t)D, 0.f);
  const float omd = (float)(1.0 - (double)d);
  float last = 0.f;
  long p = 0;
  for (long i = 0; i < n; ++i) {
    const float o = buf[p];
    last = fmaf(last, d, o * omd);
    buf[p] = fmaf(last, fb, in[i]);
    out[i] = o;
    if (++p == D) p = 0;
  }
}

void fx_allpass_host(const float* in, long n, int D, float* out) {
  std::vector<float> buf((size_t)D, 0.f);
  long p = 0;
  for (long i = 0; i < n; ++i) {
    const float v = buf[p], x = in[i];
    buf[p] = fmaf(0.5f, v, x);
    out[i] = v - x;
    if (++p == D) p = 0;
  }
}

void fx_reverb_host(const FxReverb& rv, const float* x, long n, float* y) {
  const size_t N = (size_t)std::max<long>(n, 0);
  std::vector<float> in(N), c(N), o[2];
  for (size_t i = 0; i < N; ++i) in[i] = 0.015f * (x[2 * i] + x[2 * i + 1]);
  for (int side = 0; side < 2; ++side) {
    std::vector<float>& acc = o[side];
    acc.resize(N);
    fx_comb_host(in.data(), n, rv.comb[side][0], rv.fb, rv.d, acc.data());
    for (int k = 1; k < 8; ++k) {
      fx_comb_host(in.data(), n, rv.comb[side][k], rv.fb, rv.d, c.data());
      for (size_t i = 0; i < N; ++i) acc[i] += c[i];
    }
    for (int q = 0; q < 4; ++q) {
      fx_allpass_host(acc.data(), n, rv.ap[side][q], c.data());
      acc.swap(c);
    }
  }
  for (size_t i = 0; i < N; ++i) {
    const float ol = o[0][i], orr = o[1][i];
    y[2 * i] = fmaf(ol, rv.w1, fmaf(orr, rv.w2, rv.dry2 * x[2 * i]));
    y[2 * i + 1] = fmaf(orr, rv.w1, fmaf(ol, rv.w2, rv.dry2 * x[2 * i + 1]));
  }
}

void fx_chorus_host(const FxChorus& ch, const float* x, long n, float* y) {
  std::vector<float> d((size_t)std::max<long>(n, 1));
  for (long i = 0; i < n; ++i) {
    const float w = fx_chorus_tap(ch, d.data(), i);
    d[i] = fmaf(ch.fb, w, x[i]);
    y[i] = fmaf(ch.mix, w, ch.omm * x[i]);
  }
}

void fx_mix_host(const int16_t* v, long nv, const int16_t* inst, long ni, double gv, double gi, int16_t* out) {
  for (long i = 0; i < nv; ++i) out[i] = fx_mix_sample(v[i], i < ni ? inst[i] : 0, gv, gi);
}

}  // namespace rvcx
