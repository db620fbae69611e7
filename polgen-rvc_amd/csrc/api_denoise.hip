// C ABI of librvcx.so (include/rvcx.h): noise reduction (stage 15), its taps and its host twins.
#include "api_internal.h"
#include "denoise.h"
#include "effects.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

long pad256(long n) { return (std::max<long>(n, 1) + 255) / 256 * 256; }

struct DenoisePlan {
  int sr, Cc, nf, nt;
  FxStretchGeom g;
  FxDenoiseValues v;
};

// every refusal that depends on the parameters alone
DenoisePlan denoise_check(const char* who_c, const rvcx_fx_denoise_params* p) {
  const std::string who(who_c);
  if (!p) fail(who + ": null parameters");
  if (!fx_rate_ok(p->sample_rate)) fail(who + ": the sample rate must be a multiple of 100 Hz within 8000 .. 192000");
  if (p->channels != 1 && p->channels != 2) fail(who + ": channels must be 1 or 2");
  if (p->mode != 0 && p->mode != 1) fail(who + ": mode must be 0 (profile) or 1 (adaptive)");
  const float all[8] = {p->strength, p->n_std, p->knee_db, p->thresh_mult, p->slope, p->time_constant_s, p->freq_smooth_hz,
                        p->time_smooth_ms};
  for (float f : all)
    if (!std::isfinite(f)) fail(who + ": a value is not finite");
  auto range = [&](float f, double lo, double hi, const char* name) {
    if (!((double)f >= lo && (double)f <= hi))
      fail(who + ": " + name + " must lie in " + std::to_string(lo) + " .. " + std::to_string(hi));
  };
  range(p->strength, 0.0, 1.0, "strength");
  range(p->n_std, 0.0, 10.0, "n_std");
  range(p->knee_db, (double)0.1f, 20.0, "knee_db");
  range(p->thresh_mult, 0.0, 20.0, "thresh_mult");
  range(p->slope, (double)0.1f, 100.0, "slope");
  range(p->time_constant_s, (double)0.05f, 30.0, "time_constant_s");
  if (p->freq_smooth_hz < 0.f || p->time_smooth_ms < 0.f) fail(who + ": freq_smooth_hz and time_smooth_ms must not be negative");
  DenoisePlan P;
  P.sr = p->sample_rate, P.Cc = p->channels, P.g = fx_stretch_geom(p->sample_rate);
  const double nf = fx_denoise_nf(p->freq_smooth_hz, P.g.N, P.sr), nt = fx_denoise_nt(p->time_smooth_ms, P.sr, P.g.H);
  if (nf > kDenoiseMaxNf) fail(who + ": freq_smooth_hz spans more than 64 bins to a side at this rate");
  if (nt > kDenoiseMaxNt) fail(who + ": time_smooth_ms spans more than 16 frames to a side at this rate");
  P.nf = (int)nf, P.nt = (int)nt;
  P.v = FxDenoiseValues{p->mode, p->strength, p->n_std, p->knee_db, p->thresh_mult, p->slope, p->time_constant_s,
                        p->freq_smooth_hz, p->time_smooth_ms};
  return P;
}

void length_check(const std::string& who, int64_t n) {
  if (n < 1 || n > (int64_t)1 << 30) fail(who + ": every item needs 1 .. 2^30 frames");
}

void noise_check(const std::string& who, const DenoisePlan& P, const float* noise, int64_t n_noise) {
  if (!noise) return;
  if (P.v.mode == 1) fail(who + ": the adaptive mode takes no noise clip");
  if (n_noise < 1 || n_noise > (int64_t)1 << 30) fail(who + ": a noise clip needs 1 .. 2^30 frames");
}

struct DenoiseTaps {
  float* D = nullptr;
  float* S = nullptr;
  double* mu = nullptr;
  double* sd = nullptr;
  double* b = nullptr;
  float* m = nullptr;
  bool any() const { return D || S || mu || sd || b || m; }
};

void taps_check(const std::string& who, const DenoisePlan& P, const DenoiseTaps& t) {
  if (t.any() && P.Cc != 1) fail(who + ": the taps take one channel");
  if ((t.mu || t.sd) && P.v.mode != 0) fail(who + ": mu and sd exist in mode 0 only");
  if (t.b && P.v.mode != 1) fail(who + ": b exists in mode 1 only");
}

// stage 15 on B items; noise (optional table) and n_noise as at the ABI
void run_denoise(rvcx_ctx* ctx, Ctx* C, const DenoisePlan& P, int B, const float* const* x, const int64_t* n,
                 const float* const* noise, const int64_t* n_noise, float* const* y, const DenoiseTaps& taps) {
  const FxStretchGeom g = P.g;
  const int Cc = P.Cc;
  const size_t nb = (size_t)g.nb;
  auto clip_len = [&](int b) -> long { return noise && noise[b] ? (long)n_noise[b] : 0; };
  // x, y and the interleaved staging of an item; x and staging of its clip; the spectra of both
  auto item_bytes = [&](long n_item, long n_clip) {
    size_t per_row = (size_t)pad256(n_item) * 12 + fx_denoise_row_bytes(g, fx_stretch_T(n_item, g.H), P.v.mode, true, taps.b != nullptr);
    if (n_clip > 0) per_row += (size_t)pad256(n_clip) * 8 + fx_denoise_row_bytes(g, fx_stretch_T(n_clip, g.H), P.v.mode, false, false);
    return (size_t)Cc * (per_row + 16 * 256 + 64);
  };
  const size_t table_bytes = (size_t)g.N * 8 + ((size_t)1 << 20);
  const size_t budget = arena_budget(*C);
  long n_max = 0, c_max = 0;
  for (int b = 0; b < B; ++b) {
    n_max = std::max<long>(n_max, (long)n[b]), c_max = std::max(c_max, clip_len(b));
    const size_t own = item_bytes((long)n[b], clip_len(b)) + table_bytes;
    if (own > budget)
      fail("fx_denoise: item " + std::to_string(b) + " of " + std::to_string((long)n[b]) + " frames needs " + std::to_string(own) +
           " bytes, the arena budget is " + std::to_string(budget) + " (one item is not cut into segments)");
  }
  const char* cap = getenv("RVCX_MAX_BATCH");
  const size_t most = cap ? (size_t)std::max(1, atoi(cap)) : (size_t)B;
  const int G = (int)std::max<size_t>(
      1, std::min<size_t>(std::min<size_t>(most, (size_t)B), (budget - table_bytes) / item_bytes(n_max, c_max)));
  Arena& A = C->arena;
  A.reset();
  A.reserve(item_bytes(n_max, c_max) * std::min(G, B) + table_bytes);
  hipStream_t s = C->stream;
  C->timer.make();
  hipEvent_t* ev = C->timer.ev;
  float ms[9] = {0};
  std::vector<float> w;
  std::vector<float2> tw;
  fx_stretch_tables(g.N, w, tw);
  int groups = 0;
  for (int g0 = 0; g0 < B; g0 += G, ++groups) {
    const int Bg = std::min(G, B - g0), R = Bg * Cc;
    // the group's distinct clips: a clip that several items share is analysed once
    std::vector<std::pair<const float*, long>> clips;
    std::vector<int> clip_of((size_t)Bg, -1);
    long nmax = 0, cmax = 0;
    for (int b = 0; b < Bg; ++b) {
      nmax = std::max<long>(nmax, (long)n[g0 + b]);
      if (clip_len(g0 + b) < 1) continue;
      const std::pair<const float*, long> key(noise[g0 + b], clip_len(g0 + b));
      size_t u = 0;
      while (u < clips.size() && clips[u] != key) ++u;
      if (u == clips.size()) clips.push_back(key);
      clip_of[b] = (int)u;
      cmax = std::max(cmax, key.second);
    }
    const int U = (int)clips.size(), Rn = U * Cc;
    const long ld = pad256(nmax), ldn = pad256(cmax);
    A.reset();
    float* dw = A.alloc<float>((size_t)g.N);
    float2* dtw = A.alloc<float2>((size_t)g.N / 2);
    RVCX_HIP(hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
    RVCX_HIP(hipMemcpyAsync(dtw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice, s));
    FxDenoiseDev d{};
    d.g = g, d.v = P.v, d.nf = P.nf, d.nt = P.nt, d.w = dw, d.tw = dtw;
    d.c = fx_denoise_c(g.H, P.sr, P.v.time_constant_s);
    float* stage = A.alloc<float>((size_t)R * ld);
    float* rows = A.alloc<float>((size_t)R * ld);
    float* ys = A.alloc<float>((size_t)R * ld);
    int* dlen = A.alloc<int>((size_t)R + (size_t)std::max(Rn, 1) + (size_t)R);
    d.it.R = R, d.it.ld = ld, d.it.Tf = fx_stretch_T(nmax, g.H), d.it.len = dlen, d.it.x = rows;
    const size_t fb = (size_t)R * d.it.Tf * nb;
    d.it.D = A.alloc<float2>(fb);
    d.it.A2 = A.alloc<float>(fb);
    d.it.S = A.alloc<float>(fb);
    if (P.v.mode == 0) {
      d.mu = A.alloc<double>((size_t)R * nb);
      d.sd = A.alloc<double>((size_t)R * nb);
    } else {
      d.f = A.alloc<double>(fb);
      d.b = taps.b ? A.alloc<double>(fb) : nullptr;
    }
    float *stage_n = nullptr, *rows_n = nullptr;
    if (U > 0) {
      stage_n = A.alloc<float>((size_t)Rn * ldn);
      rows_n = A.alloc<float>((size_t)Rn * ldn);
      d.nz.R = Rn, d.nz.ld = ldn, d.nz.Tf = fx_stretch_T(cmax, g.H), d.nz.len = dlen + R, d.nz.x = rows_n;
      d.nz.A2 = A.alloc<float>((size_t)Rn * d.nz.Tf * nb);
      d.nz.S = A.alloc<float>((size_t)Rn * d.nz.Tf * nb);
    }
    d.prof = dlen + R + std::max(Rn, 1);
    std::vector<int> len((size_t)R + (size_t)std::max(Rn, 1) + (size_t)R, 0);
    for (int r = 0; r < R; ++r) {
      len[r] = (int)n[g0 + r / Cc];
      len[(size_t)R + std::max(Rn, 1) + r] = clip_of[r / Cc] < 0 ? -1 : clip_of[r / Cc] * Cc + r % Cc;
    }
    for (int r = 0; r < Rn; ++r) len[(size_t)R + r] = (int)clips[r / Cc].second;
    RVCX_HIP(hipEventRecord(ev[0], s));
    RVCX_HIP(hipMemcpyAsync(dlen, len.data(), len.size() * sizeof(int), hipMemcpyHostToDevice, s));
    for (int b = 0; b < Bg; ++b)
      RVCX_HIP(hipMemcpyAsync(stage + (size_t)b * ld * Cc, x[g0 + b], (size_t)n[g0 + b] * Cc * 4, hipMemcpyDefault, s));
    launch_fx_deinterleave(stage, rows, dlen, Bg, Cc, ld, s);
    if (U > 0) {
      for (int u = 0; u < U; ++u)
        RVCX_HIP(hipMemcpyAsync(stage_n + (size_t)u * ldn * Cc, clips[u].first, (size_t)clips[u].second * Cc * 4, hipMemcpyDefault, s));
      launch_fx_deinterleave(stage_n, rows_n, d.nz.len, U, Cc, ldn, s);
    }
    RVCX_HIP(hipEventRecord(ev[1], s));
    launch_denoise_analysis(d, s, ev + 2);
    const size_t cnt = (size_t)fx_stretch_T(len[0], g.H) * nb;               // taps: one row
    // (stream order: D leaves before the synthesis writes the frames over it, m after the mask took A2's place)
    if (taps.D) RVCX_HIP(hipMemcpyAsync(taps.D, d.it.D, cnt * 8, hipMemcpyDefault, s));
    if (taps.S) RVCX_HIP(hipMemcpyAsync(taps.S, d.it.S, cnt * 4, hipMemcpyDefault, s));
    launch_denoise_mask(d, s, ev + 4);
    if (taps.mu) RVCX_HIP(hipMemcpyAsync(taps.mu, d.mu, nb * 8, hipMemcpyDefault, s));
    if (taps.sd) RVCX_HIP(hipMemcpyAsync(taps.sd, d.sd, nb * 8, hipMemcpyDefault, s));
    if (taps.b) RVCX_HIP(hipMemcpyAsync(taps.b, d.b, cnt * 8, hipMemcpyDefault, s));
    if (taps.m) RVCX_HIP(hipMemcpyAsync(taps.m, d.it.A2, cnt * 4, hipMemcpyDefault, s));
    launch_denoise_synthesis(d, ys, ld, s, ev + 6);
    launch_fx_interleave(ys, stage, dlen, Bg, Cc, ld, s);
    for (int b = 0; b < Bg; ++b)
      RVCX_HIP(hipMemcpyAsync(y[g0 + b], stage + (size_t)b * ld * Cc, (size_t)n[g0 + b] * Cc * 4, hipMemcpyDefault, s));
    RVCX_HIP(hipEventRecord(ev[8], s));
    RVCX_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 8; ++k) {
      float t = 0.f;
      RVCX_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms[k] += t, ms[8] += t;
    }
  }
  A.reset();
  // {copies in + layout, analysis, smoothing, statistics or floor, mask, synthesis, overlap-add, copies back, total}
  std::copy(ms, ms + 9, C->timing);
  ctx->fx_groups = groups;
}

template <typename F>
int host_call(F&& body) {
  try {
    body();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

}  // namespace

extern "C" {

int rvcx_fx_denoise_tiles(int32_t* tile_t, int32_t* tile_k, int32_t* stat_chunk) {
  if (tile_t) *tile_t = kDenoiseTileT;
  if (tile_k) *tile_k = kDenoiseTileK;
  if (stat_chunk) *stat_chunk = kDenoiseStatChunk;
  return 0;
}

int rvcx_fx_denoise_frames(int64_t n, int sr, int64_t* T, int32_t* N, int32_t* nf, int32_t* nt) {
  return host_call([&] {
    if (!fx_rate_ok(sr)) fail("fx_denoise_frames: the sample rate must be a multiple of 100 Hz within 8000 .. 192000");
    length_check("fx_denoise_frames", n);
    const FxStretchGeom g = fx_stretch_geom(sr);
    if (T) *T = fx_stretch_T((long)n, g.H);
    if (N) *N = g.N;
    if (nf) *nf = (int32_t)fx_denoise_nf(500.0, g.N, sr);
    if (nt) *nt = (int32_t)fx_denoise_nt(50.0, sr, g.H);
  });
}

int rvcx_fx_denoise(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, const float* const* noise,
                    const int64_t* n_noise, const rvcx_fx_denoise_params* params, float* const* y) {
  API_BEGIN(ctx)
  const DenoisePlan P = denoise_check("fx_denoise", params);
  if (B < 1 || !x || !n || !y) fail("fx_denoise: null argument or B < 1");
  if (noise && !n_noise) fail("fx_denoise: noise clips without their lengths");
  for (int b = 0; b < B; ++b) {
    if (!x[b] || !y[b]) fail("fx_denoise: null pointer in a table");
    length_check("fx_denoise", n[b]);
    if (noise) noise_check("fx_denoise", P, noise[b], n_noise[b]);
  }
  if (P.v.strength == 0.f) {          // skip: nothing is launched, the output is the input bit for bit
    for (int b = 0; b < B; ++b)
      if (y[b] != x[b]) RVCX_HIP(hipMemcpy(y[b], x[b], (size_t)n[b] * P.Cc * 4, hipMemcpyDefault));
    std::fill(C->timing, C->timing + 9, 0.f);
    ctx->fx_groups = 0;
    return;
  }
  run_denoise(ctx, C, P, B, x, n, noise, n_noise, y, DenoiseTaps{});
  API_END
}

int rvcx_op_fx_denoise_taps(rvcx_ctx* ctx, const float* x, int64_t n, const float* noise, int64_t n_noise,
                            const rvcx_fx_denoise_params* params, float* y, float* D, float* S, double* mu, double* sd, double* b,
                            float* m) {
  API_BEGIN(ctx)
  const DenoisePlan P = denoise_check("op_fx_denoise_taps", params);
  if (!x || !y) fail("op_fx_denoise_taps: null pointer");
  length_check("op_fx_denoise_taps", n);
  noise_check("op_fx_denoise_taps", P, noise, n_noise);
  DenoiseTaps t;
  t.D = D, t.S = S, t.mu = mu, t.sd = sd, t.b = b, t.m = m;
  taps_check("op_fx_denoise_taps", P, t);
  if (P.v.strength == 0.f) fail("op_fx_denoise_taps: the stage is skipped at strength 0, it has no taps");
  run_denoise(ctx, C, P, 1, &x, &n, noise ? &noise : nullptr, &n_noise, &y, t);
  API_END
}

// ---- host only -----------------------------------------------------------------------------------------------------------------
int rvcx_fx_denoise_host(const float* x, int64_t n, const float* noise, int64_t n_noise, const rvcx_fx_denoise_params* params,
                         float* y, float* D, float* S, double* mu, double* sd, double* b, float* m) {
  return host_call([&] {
    const DenoisePlan P = denoise_check("fx_denoise_host", params);
    if (!x || !y) fail("fx_denoise_host: null pointer");
    length_check("fx_denoise_host", n);
    noise_check("fx_denoise_host", P, noise, n_noise);
    DenoiseTaps t;
    t.D = D, t.S = S, t.mu = mu, t.sd = sd, t.b = b, t.m = m;
    taps_check("fx_denoise_host", P, t);
    if (P.v.strength == 0.f) {
      if (t.any()) fail("fx_denoise_host: the stage is skipped at strength 0, it has no taps");
      if (y != x) std::memcpy(y, x, (size_t)n * P.Cc * 4);
      return;
    }
    std::vector<float> plane((size_t)n), clip((size_t)(noise ? n_noise : 0)), out((size_t)n);
    for (int c = 0; c < P.Cc; ++c) {
      for (int64_t i = 0; i < n; ++i) plane[i] = x[i * P.Cc + c];
      if (noise)
        for (int64_t i = 0; i < n_noise; ++i) clip[i] = noise[i * P.Cc + c];
      fx_denoise_host(plane.data(), (long)n, noise ? clip.data() : nullptr, (long)n_noise, P.sr, P.v, out.data(), D, S, mu, sd, b, m);
      for (int64_t i = 0; i < n; ++i) y[i * P.Cc + c] = out[i];
    }
  });
}

int rvcx_fx_denoise_smooth_host(const float* A2, int64_t T, int nb, int nf, int nt, float* S) {
  return host_call([&] {
    if (!A2 || !S) fail("fx_denoise_smooth_host: null pointer");
    if (T < 1 || T > (int64_t)1 << 24 || nb < 1 || nb > 4097) fail("fx_denoise_smooth_host: T in 1 .. 2^24 and nb in 1 .. 4097 are required");
    if (nf < 0 || nf > kDenoiseMaxNf || nt < 0 || nt > kDenoiseMaxNt)
      fail("fx_denoise_smooth_host: half-widths of 0 .. 64 bins and 0 .. 16 frames are required");
    fx_denoise_smooth_host(A2, (long)T, nb, nf, nt, S);
  });
}

}  // extern "C"
