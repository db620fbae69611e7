// C ABI of librvcx.so (include/rvcx.h): noise reduction (stage 15), its taps and its host twins.
#include "api_fx_common.h"
#include "denoise.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

struct DenoisePlan {
  int sr, Cc, nf, nt;
  FxStretchGeom g;
  FxDenoiseValues v;
};

// every refusal that depends on the parameters alone
DenoisePlan denoise_check(const char* who_c, const rvcx_fx_denoise_params* p) {
  const std::string who(who_c);
  if (!p) fail(who + ": null parameters");
  check_rate(who_c, p->sample_rate);
  check_channels(who_c, p->channels);
  if (p->mode != 0 && p->mode != 1) fail(who + ": mode must be 0 (profile) or 1 (adaptive)");
  check_finite(who_c, {p->strength, p->n_std, p->knee_db, p->thresh_mult, p->slope, p->time_constant_s, p->freq_smooth_hz,
                       p->time_smooth_ms});
  check_range(who_c, p->strength, 0.0, 1.0, "strength");
  check_range(who_c, p->n_std, 0.0, 10.0, "n_std");
  check_range(who_c, p->knee_db, (double)0.1f, 20.0, "knee_db");
  check_range(who_c, p->thresh_mult, 0.0, 20.0, "thresh_mult");
  check_range(who_c, p->slope, (double)0.1f, 100.0, "slope");
  check_range(who_c, p->time_constant_s, (double)0.05f, 30.0, "time_constant_s");
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
  long n_max = 0, c_max = 0;
  for (int b = 0; b < B; ++b) {
    n_max = std::max<long>(n_max, (long)n[b]), c_max = std::max(c_max, clip_len(b));
    check_item_fits("fx_denoise", *C, b, n[b], item_bytes((long)n[b], clip_len(b)) + table_bytes);
  }
  const size_t worst = item_bytes(n_max, c_max);
  const int G = fx_group_size(*C, B, worst, table_bytes);
  Arena& A = C->arena;
  A.reset();
  A.reserve(worst * G + table_bytes);
  hipStream_t s = C->stream;
  FxTimer T(*C);
  const StftTables tables(g.N);
  int groups = 0;
  for (int g0 = 0; g0 < B; g0 += G, ++groups) {
    const int Bg = std::min(G, B - g0), R = Bg * Cc;
    // the group's distinct clips: a clip that several items share is analysed once
    std::vector<std::pair<const float*, int64_t>> clips;
    std::vector<int> clip_of((size_t)Bg, -1);
    long nmax = 0, cmax = 0;
    for (int b = 0; b < Bg; ++b) {
      nmax = std::max<long>(nmax, (long)n[g0 + b]);
      if (clip_len(g0 + b) < 1) continue;
      const std::pair<const float*, int64_t> key(noise[g0 + b], clip_len(g0 + b));
      size_t u = 0;
      while (u < clips.size() && clips[u] != key) ++u;
      if (u == clips.size()) clips.push_back(key);
      clip_of[b] = (int)u;
      cmax = std::max<long>(cmax, key.second);
    }
    const int U = (int)clips.size(), Rn = U * Cc;
    const long ld = pad256(nmax), ldn = pad256(cmax);
    A.reset();
    FxDenoiseDev d{};
    tables.upload(*C, d.w, d.tw);
    d.g = g, d.v = P.v, d.nf = P.nf, d.nt = P.nt;
    d.c = fx_denoise_c(g.H, P.sr, P.v.time_constant_s);
    float* stage = A.alloc<float>((size_t)R * ld);
    float* rows = A.alloc<float>((size_t)R * ld);
    float* ys = A.alloc<float>((size_t)R * ld);
    d.it.R = R, d.it.ld = ld, d.it.Tf = fx_stretch_T(nmax, g.H), d.it.x = rows;
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
      d.nz.R = Rn, d.nz.ld = ldn, d.nz.Tf = fx_stretch_T(cmax, g.H), d.nz.x = rows_n;
      d.nz.A2 = A.alloc<float>((size_t)Rn * d.nz.Tf * nb);
      d.nz.S = A.alloc<float>((size_t)Rn * d.nz.Tf * nb);
    }
    // the items' rows, the clips' rows (one entry at the least), and per item row the clip row of its profile (-1: none)
    std::vector<int> len = row_lengths(n + g0, Bg, Cc);
    len.resize((size_t)R + (size_t)std::max(Rn, 1) + (size_t)R, 0);
    for (int r = 0; r < Rn; ++r) len[(size_t)R + r] = (int)clips[r / Cc].second;
    for (int r = 0; r < R; ++r) len[(size_t)R + std::max(Rn, 1) + r] = clip_of[r / Cc] < 0 ? -1 : clip_of[r / Cc] * Cc + r % Cc;
    T.mark(0);
    const int* dlen = to_dev(*C, len.data(), len.size());
    d.it.len = dlen, d.nz.len = U > 0 ? dlen + R : nullptr, d.prof = dlen + R + std::max(Rn, 1);
    stage_in([&](int b) { return std::make_pair(x[g0 + b], n[g0 + b]); }, Bg, Cc, ld, stage, rows, dlen, s);
    if (U > 0) stage_in([&](int u) { return clips[u]; }, U, Cc, ldn, stage_n, rows_n, d.nz.len, s);
    T.mark(1);
    launch_denoise_analysis(d, s, T.ev + 2);
    const size_t cnt = (size_t)fx_stretch_T(len[0], g.H) * nb;               // taps: one row
    // (stream order: D leaves before the synthesis writes the frames over it, m after the mask took A2's place)
    if (taps.D) RVCX_HIP(hipMemcpyAsync(taps.D, d.it.D, cnt * 8, hipMemcpyDefault, s));
    if (taps.S) RVCX_HIP(hipMemcpyAsync(taps.S, d.it.S, cnt * 4, hipMemcpyDefault, s));
    launch_denoise_mask(d, s, T.ev + 4);
    if (taps.mu) RVCX_HIP(hipMemcpyAsync(taps.mu, d.mu, nb * 8, hipMemcpyDefault, s));
    if (taps.sd) RVCX_HIP(hipMemcpyAsync(taps.sd, d.sd, nb * 8, hipMemcpyDefault, s));
    if (taps.b) RVCX_HIP(hipMemcpyAsync(taps.b, d.b, cnt * 8, hipMemcpyDefault, s));
    if (taps.m) RVCX_HIP(hipMemcpyAsync(taps.m, d.it.A2, cnt * 4, hipMemcpyDefault, s));
    launch_denoise_synthesis(d, ys, ld, s, T.ev + 6);
    stage_out(ys, dlen, Bg, Cc, ld, stage, s, [&](int b) { return std::make_pair(y[g0 + b], n[g0 + b]); });
    T.mark(8);
    RVCX_HIP(hipStreamSynchronize(s));
    // {copies in + layout, analysis, smoothing, statistics or floor, mask, synthesis, overlap-add, copies back, total}
    for (int k = 0; k < 8; ++k) T.ms[8] += T.add(k, k, k + 1);
  }
  A.reset();
  T.store(*C);
  ctx->fx_groups = groups;
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
    check_rate("fx_denoise_frames", sr);
    check_frames("fx_denoise_frames", n);
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
  for (int b = 0; b < B; ++b) {      // (not check_items: an item's clip is refused before the next item's pointers)
    if (!x[b] || !y[b]) fail("fx_denoise: null pointer in a table");
    check_frames("fx_denoise", n[b]);
    if (noise) noise_check("fx_denoise", P, noise[b], n_noise[b]);
  }
  if (P.v.strength == 0.f) return fx_skip(ctx, B, x, n, P.Cc, y);
  run_denoise(ctx, C, P, B, x, n, noise, n_noise, y, DenoiseTaps{});
  API_END
}

int rvcx_op_fx_denoise_taps(rvcx_ctx* ctx, const float* x, int64_t n, const float* noise, int64_t n_noise,
                            const rvcx_fx_denoise_params* params, float* y, float* D, float* S, double* mu, double* sd, double* b,
                            float* m) {
  API_BEGIN(ctx)
  const DenoisePlan P = denoise_check("op_fx_denoise_taps", params);
  if (!x || !y) fail("op_fx_denoise_taps: null pointer");
  check_frames("op_fx_denoise_taps", n);
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
    check_frames("fx_denoise_host", n);
    noise_check("fx_denoise_host", P, noise, n_noise);
    DenoiseTaps t;
    t.D = D, t.S = S, t.mu = mu, t.sd = sd, t.b = b, t.m = m;
    taps_check("fx_denoise_host", P, t);
    if (P.v.strength == 0.f) {
      if (t.any()) fail("fx_denoise_host: the stage is skipped at strength 0, it has no taps");
      if (y != x) std::memcpy(y, x, (size_t)n * P.Cc * 4);
      return;
    }
    std::vector<float> clip, out((size_t)n);
    host_planes(x, n, P.Cc, y, n, [&](int c, const float* plane) {
      if (noise) take_plane(noise, n_noise, P.Cc, c, clip);
      fx_denoise_host(plane, (long)n, noise ? clip.data() : nullptr, (long)n_noise, P.sr, P.v, out.data(), D, S, mu, sd, b, m);
      return out.data();
    });
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
