// C ABI of librvcx.so (include/rvcx.h): formant shift and envelope transfer (stage 17), the formant-preserving pitch shift
// (stage 18), their taps and their host twins.
#include "api_internal.h"
#include "effects.h"
#include "formant.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

long pad256(long n) { return (std::max<long>(n, 1) + 255) / 256 * 256; }

struct FormantPlan {
  int sr, Cc, nc;
  FxStretchGeom g;
  FxFormantValues v;
};

const rvcx_fx_formant_params kFormantDefaults = {0, 0, 1.f, 1.f, 1.5f, 8, 24.f, 1};

// every refusal that depends on the parameters alone
FormantPlan formant_check(const char* who_c, const rvcx_fx_formant_params* p) {
  const std::string who(who_c);
  if (!p) fail(who + ": null parameters");
  if (!fx_rate_ok(p->sample_rate)) fail(who + ": the sample rate must be a multiple of 100 Hz within 8000 .. 192000");
  if (p->channels != 1 && p->channels != 2) fail(who + ": channels must be 1 or 2");
  for (float f : {p->ratio, p->amount, p->quefrency_ms, p->max_gain_db})
    if (!std::isfinite(f)) fail(who + ": a value is not finite");
  auto range = [&](float f, double lo, double hi, const char* name) {
    if (!((double)f >= lo && (double)f <= hi))
      fail(who + ": " + name + " must lie in " + std::to_string(lo) + " .. " + std::to_string(hi));
  };
  range(p->ratio, 0.5, 2.0, "ratio");
  range(p->amount, 0.0, 1.0, "amount");
  range(p->max_gain_db, 0.0, 48.0, "max_gain_db");
  if (p->iterations < 0 || p->iterations > kFormantMaxIter) fail(who + ": iterations must lie in 0 .. 16");
  if (p->keep_energy != 0 && p->keep_energy != 1) fail(who + ": keep_energy must be 0 or 1");
  if (!(p->quefrency_ms > 0.f)) fail(who + ": quefrency_ms must be positive");
  FormantPlan P;
  P.sr = p->sample_rate, P.Cc = p->channels, P.g = fx_stretch_geom(p->sample_rate);
  const double nc = fx_formant_nc(p->quefrency_ms, P.sr);
  if (!(nc >= 1.0 && nc <= (double)(P.g.N / 8)))
    fail(who + ": quefrency_ms must span 1 .. " + std::to_string(P.g.N / 8) + " samples (N / 8) at this rate");
  P.nc = (int)nc;
  P.v = FxFormantValues{p->ratio, p->amount, p->quefrency_ms, p->max_gain_db, p->iterations, p->keep_energy};
  return P;
}

void length_check(const std::string& who, int64_t n) {
  if (n < 1 || n > (int64_t)1 << 30) fail(who + ": every item needs 1 .. 2^30 frames");
}

void items_check(const std::string& who, int B, const float* const* x, const int64_t* n, float* const* y) {
  if (B < 1 || !x || !n || !y) fail(who + ": null argument or B < 1");
  for (int b = 0; b < B; ++b) {
    if (!x[b] || !y[b]) fail(who + ": null pointer in a table");
    length_check(who, n[b]);
  }
}

// what one item takes of the arena: x, y and the interleaved staging, the same for its source, and the windowed frames
// (and, for the one row of a call with taps, 20 bytes per bin and 4 per frame)
size_t item_bytes(const FormantPlan& P, long n_item, bool with_src, bool taps = false) {
  const size_t T = (size_t)fx_stretch_T(n_item, P.g.H);
  const size_t per_row = (size_t)pad256(n_item) * (with_src ? 20 : 12) + fx_formant_row_bytes(P.g, (long)T) +
                         (taps ? T * ((size_t)P.g.nb * 20 + 4) : 0);
  return (size_t)P.Cc * (per_row + 16 * 256 + 64);
}
size_t table_bytes(const FormantPlan& P) { return (size_t)P.g.N * 8 + ((size_t)1 << 20); }

// an item without a source at ratio 1 is its own target: it is not run (the skip rule, item by item)
bool item_runs(const FormantPlan& P, const float* const* src, int b) { return P.v.ratio != 1.f || (src && src[b]); }

void fit_check(const std::string& who, Ctx* C, const FormantPlan& P, int B, const int64_t* n, const float* const* src,
               bool taps = false) {
  const size_t budget = arena_budget(*C);
  for (int b = 0; b < B; ++b) {
    if (!item_runs(P, src, b)) continue;
    const size_t own = item_bytes(P, (long)n[b], src && src[b], taps) + table_bytes(P);
    if (own > budget)
      fail(who + ": item " + std::to_string(b) + " of " + std::to_string((long)n[b]) + " frames needs " + std::to_string(own) +
           " bytes, the arena budget is " + std::to_string(budget) + " (one item is not cut into segments)");
  }
}

struct FormantTaps {
  float* D = nullptr;
  float* E = nullptr;
  float* Es = nullptr;
  float* g = nullptr;
  float* s = nullptr;
  bool any() const { return D || E || Es || g || s; }
};

// stage 17 on B items; src (optional table) as at the ABI.  ms receives {copies in + layout, frames, overlap-add, copies back}
void run_formant(rvcx_ctx* ctx, Ctx* C, const FormantPlan& P, int B, const float* const* x, const int64_t* n,
                 const float* const* src, float* const* y, const FormantTaps& taps, float* ms4) {
  const FxStretchGeom g = P.g;
  const int Cc = P.Cc;
  fit_check("fx_formant", C, P, B, n, src, taps.any());
  std::vector<int> run;                    // the items that are not skipped, in call order
  long n_max = 0;
  bool any_src = false;
  size_t own_max = 0;                      // the largest item on its own (fit_check has passed it)
  for (int b = 0; b < B; ++b) {
    if (!item_runs(P, src, b)) {
      if (y[b] != x[b]) RVCX_HIP(hipMemcpy(y[b], x[b], (size_t)n[b] * Cc * 4, hipMemcpyDefault));
      continue;
    }
    run.push_back(b);
    n_max = std::max<long>(n_max, (long)n[b]);
    any_src = any_src || (src && src[b]);
    own_max = std::max(own_max, item_bytes(P, (long)n[b], src && src[b], taps.any()));
  }
  std::fill(ms4, ms4 + 4, 0.f);
  ctx->fx_groups = 0;
  if (run.empty()) return;
  const int Br = (int)run.size();
  const size_t budget = arena_budget(*C), tb = table_bytes(P), worst = item_bytes(P, n_max, any_src, taps.any());
  const char* cap = getenv("RVCX_MAX_BATCH");
  const size_t most = cap ? (size_t)std::max(1, atoi(cap)) : (size_t)Br;
  const int G = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(most, (size_t)Br), (budget - tb) / worst));
  Arena& A = C->arena;
  A.reset();
  A.reserve((G > 1 ? worst * G : own_max) + tb);
  hipStream_t s = C->stream;
  C->timer.make();
  hipEvent_t* ev = C->timer.ev;
  std::vector<float> w;
  std::vector<float2> tw;
  fx_stretch_tables(g.N, w, tw);
  int groups = 0;
  for (int g0 = 0; g0 < Br; g0 += G, ++groups) {
    const int Bg = std::min(G, Br - g0), R = Bg * Cc;
    long nmax = 0;
    bool gsrc = false;
    for (int i = 0; i < Bg; ++i) {
      const int b = run[g0 + i];
      nmax = std::max<long>(nmax, (long)n[b]);
      gsrc = gsrc || (src && src[b]);
    }
    const long ld = pad256(nmax);
    A.reset();
    float* dw = A.alloc<float>((size_t)g.N);
    float2* dtw = A.alloc<float2>((size_t)g.N / 2);
    RVCX_HIP(hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
    RVCX_HIP(hipMemcpyAsync(dtw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice, s));
    FxFormantDev d{};
    d.g = g, d.v = P.v, d.nc = P.nc, d.limit = fx_formant_limit(P.v.max_gain_db), d.R = R, d.ld = ld, d.w = dw, d.tw = dtw;
    d.Tf = fx_stretch_T(nmax, g.H);
    float* stage = A.alloc<float>((size_t)R * ld);
    float* rows = A.alloc<float>((size_t)R * ld);
    float* ys = A.alloc<float>((size_t)R * ld);
    float *stage_s = nullptr, *rows_s = nullptr;
    if (gsrc) {
      stage_s = A.alloc<float>((size_t)R * ld);
      rows_s = A.alloc<float>((size_t)R * ld);
    }
    int* dlen = A.alloc<int>((size_t)R * 2);
    d.fr = A.alloc<float>((size_t)R * d.Tf * g.N);
    d.len = dlen, d.has_src = dlen + R, d.x = rows, d.src = rows_s;
    const size_t cnt = (size_t)fx_stretch_T((long)n[run[g0]], g.H) * g.nb;         // taps: one row
    if (taps.D) d.taps.D = A.alloc<float2>(cnt);
    if (taps.E) d.taps.E = A.alloc<float>(cnt);
    if (taps.Es) d.taps.Es = A.alloc<float>(cnt);
    if (taps.g) d.taps.g = A.alloc<float>(cnt);
    if (taps.s) d.taps.s = A.alloc<float>((size_t)d.Tf);
    std::vector<int> len((size_t)R * 2, 0);
    for (int r = 0; r < R; ++r) {
      const int b = run[g0 + r / Cc];
      len[r] = (int)n[b];
      len[R + r] = (src && src[b]) ? 1 : 0;
    }
    RVCX_HIP(hipEventRecord(ev[0], s));
    RVCX_HIP(hipMemcpyAsync(dlen, len.data(), len.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (gsrc) RVCX_HIP(hipMemsetAsync(stage_s, 0, (size_t)R * ld * 4, s));          // (rows without a source are never read)
    for (int i = 0; i < Bg; ++i) {
      const int b = run[g0 + i];
      RVCX_HIP(hipMemcpyAsync(stage + (size_t)i * ld * Cc, x[b], (size_t)n[b] * Cc * 4, hipMemcpyDefault, s));
      if (src && src[b]) RVCX_HIP(hipMemcpyAsync(stage_s + (size_t)i * ld * Cc, src[b], (size_t)n[b] * Cc * 4, hipMemcpyDefault, s));
    }
    launch_fx_deinterleave(stage, rows, dlen, Bg, Cc, ld, s);
    if (gsrc) launch_fx_deinterleave(stage_s, rows_s, dlen, Bg, Cc, ld, s);
    RVCX_HIP(hipEventRecord(ev[1], s));
    launch_formant(d, ys, ld, s, ev + 2);
    if (taps.D) RVCX_HIP(hipMemcpyAsync(taps.D, d.taps.D, cnt * 8, hipMemcpyDefault, s));
    if (taps.E) RVCX_HIP(hipMemcpyAsync(taps.E, d.taps.E, cnt * 4, hipMemcpyDefault, s));
    if (taps.Es) RVCX_HIP(hipMemcpyAsync(taps.Es, d.taps.Es, cnt * 4, hipMemcpyDefault, s));
    if (taps.g) RVCX_HIP(hipMemcpyAsync(taps.g, d.taps.g, cnt * 4, hipMemcpyDefault, s));
    if (taps.s) RVCX_HIP(hipMemcpyAsync(taps.s, d.taps.s, (size_t)fx_stretch_T((long)n[run[g0]], g.H) * 4, hipMemcpyDefault, s));
    launch_fx_interleave(ys, stage, dlen, Bg, Cc, ld, s);
    for (int i = 0; i < Bg; ++i) {
      const int b = run[g0 + i];
      RVCX_HIP(hipMemcpyAsync(y[b], stage + (size_t)i * ld * Cc, (size_t)n[b] * Cc * 4, hipMemcpyDefault, s));
    }
    RVCX_HIP(hipEventRecord(ev[4], s));
    RVCX_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) {
      float t = 0.f;
      RVCX_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
      ms4[k] += t;
    }
  }
  A.reset();
  ctx->fx_groups = groups;
}

// {copies in + layout, frames, overlap-add, copies back, 0, 0, 0, stage 14 (stage 18 only), total}
void set_timing(Ctx* C, const float* ms4, float pitch_ms) {
  float ms[9] = {ms4[0], ms4[1], ms4[2], ms4[3], 0.f, 0.f, 0.f, pitch_ms, ms4[0] + ms4[1] + ms4[2] + ms4[3] + pitch_ms};
  std::copy(ms, ms + 9, C->timing);
}

bool stage_skipped(const FormantPlan& P, int B, const float* const* src) {
  if (P.v.amount == 0.f) return true;
  for (int b = 0; b < B; ++b)
    if (item_runs(P, src, b)) return false;
  return true;
}

void copy_through(int B, const float* const* x, const int64_t* n, int Cc, float* const* y) {
  for (int b = 0; b < B; ++b)
    if (y[b] != x[b]) RVCX_HIP(hipMemcpy(y[b], x[b], (size_t)n[b] * Cc * 4, hipMemcpyDefault));
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

// stage 18's parameters: the caller's (or the defaults) on the call's shape, with ratio 1
rvcx_fx_formant_params preserve_params(const rvcx_fx_formant_params* p, int sr, int channels) {
  rvcx_fx_formant_params q = p ? *p : kFormantDefaults;
  q.sample_rate = sr, q.channels = channels, q.ratio = 1.f;
  return q;
}

void semitones_check(const std::string& who, double semitones) {
  if (!std::isfinite(semitones)) fail(who + ": a value is not finite");
  if (std::fabs(semitones) > 12.0) fail(who + ": semitones must lie in -12 .. 12");
}

}  // namespace

extern "C" {

int rvcx_fx_formant_frames(int64_t n, int sr, float quefrency_ms, int64_t* T, int32_t* N, int32_t* nc) {
  return host_call([&] {
    rvcx_fx_formant_params p = kFormantDefaults;
    p.sample_rate = sr, p.channels = 1, p.quefrency_ms = quefrency_ms;
    const FormantPlan P = formant_check("fx_formant_frames", &p);
    length_check("fx_formant_frames", n);
    if (T) *T = fx_stretch_T((long)n, P.g.H);
    if (N) *N = P.g.N;
    if (nc) *nc = P.nc;
  });
}

int rvcx_fx_formant(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, const float* const* src,
                    const rvcx_fx_formant_params* params, float* const* y) {
  API_BEGIN(ctx)
  const FormantPlan P = formant_check("fx_formant", params);
  items_check("fx_formant", B, x, n, y);
  float ms4[4] = {0};
  if (stage_skipped(P, B, src)) {      // skip: nothing is launched, the output is the input bit for bit
    copy_through(B, x, n, P.Cc, y);
    ctx->fx_groups = 0;
  } else {
    run_formant(ctx, C, P, B, x, n, src, y, FormantTaps{}, ms4);
  }
  set_timing(C, ms4, 0.f);
  API_END
}

int rvcx_fx_pitch_shift_formant(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, int channels, int sr,
                                double semitones, const rvcx_fx_formant_params* params, float* const* y) {
  API_BEGIN(ctx)
  semitones_check("fx_pitch_shift_formant", semitones);
  const rvcx_fx_formant_params q = preserve_params(params, sr, channels);
  const FormantPlan P = formant_check("fx_pitch_shift_formant", &q);
  items_check("fx_pitch_shift_formant", B, x, n, y);
  float ms4[4] = {0};
  if (rvcx_fx_pitch_ratio(sr, semitones) == sr) {      // skip: nothing is launched, the output is the input bit for bit
    copy_through(B, x, n, channels, y);
    ctx->fx_groups = 0;
    set_timing(C, ms4, 0.f);
    return;
  }
  const bool transfer = P.v.amount != 0.f;
  if (transfer) {
    // stage 14 writes every output before the transfer reads the first input: no output may touch any input, in part either
    for (int b = 0; b < B; ++b) {
      const uintptr_t y0 = (uintptr_t)y[b], y1 = y0 + (size_t)n[b] * channels * 4;
      for (int c = 0; c < B; ++c) {
        const uintptr_t x0 = (uintptr_t)x[c], x1 = x0 + (size_t)n[c] * channels * 4;
        if (y0 < x1 && x0 < y1)
          fail("fx_pitch_shift_formant: an output must not lie over an input (the inputs are the sources of the envelopes)");
      }
    }
    fit_check("fx_pitch_shift_formant", C, P, B, n, x);          // before stage 14 writes anything
  }
  if (rvcx_fx_pitch_shift(ctx, B, x, n, channels, sr, semitones, y) != 0) fail(g_last_error);
  const float pitch_ms = C->timing[8];
  const int pitch_groups = ctx->fx_groups;
  if (transfer) {
    std::vector<const float*> shifted(y, y + B);
    run_formant(ctx, C, P, B, shifted.data(), n, x, y, FormantTaps{}, ms4);
  }
  ctx->fx_groups += pitch_groups;
  set_timing(C, ms4, pitch_ms);
  API_END
}

int rvcx_op_fx_formant_taps(rvcx_ctx* ctx, const float* x, int64_t n, const float* src, const rvcx_fx_formant_params* params,
                            float* y, float* D, float* E, float* Es, float* g, float* s) {
  API_BEGIN(ctx)
  const FormantPlan P = formant_check("op_fx_formant_taps", params);
  if (P.Cc != 1) fail("op_fx_formant_taps: the taps take one channel");
  if (!x || !y) fail("op_fx_formant_taps: null pointer");
  length_check("op_fx_formant_taps", n);
  if (stage_skipped(P, 1, src ? &src : nullptr)) fail("op_fx_formant_taps: the stage is skipped at these values, it has no taps");
  FormantTaps t;
  t.D = D, t.E = E, t.Es = Es, t.g = g, t.s = s;
  float ms4[4] = {0};
  run_formant(ctx, C, P, 1, &x, &n, src ? &src : nullptr, &y, t, ms4);
  set_timing(C, ms4, 0.f);
  API_END
}

// ---- host only -----------------------------------------------------------------------------------------------------------------
int rvcx_fx_formant_host(const float* x, int64_t n, const float* src, const rvcx_fx_formant_params* params, float* y, float* D,
                         float* E, float* Es, float* g, float* s) {
  return host_call([&] {
    const FormantPlan P = formant_check("fx_formant_host", params);
    if (!x || !y) fail("fx_formant_host: null pointer");
    length_check("fx_formant_host", n);
    const bool taps = D || E || Es || g || s;
    if (taps && P.Cc != 1) fail("fx_formant_host: the taps take one channel");
    if (stage_skipped(P, 1, src ? &src : nullptr)) {
      if (taps) fail("fx_formant_host: the stage is skipped at these values, it has no taps");
      if (y != x) std::memcpy(y, x, (size_t)n * P.Cc * 4);
      return;
    }
    std::vector<float> plane((size_t)n), other((size_t)(src ? n : 0)), out((size_t)n);
    for (int c = 0; c < P.Cc; ++c) {
      for (int64_t i = 0; i < n; ++i) plane[i] = x[i * P.Cc + c];
      if (src)
        for (int64_t i = 0; i < n; ++i) other[i] = src[i * P.Cc + c];
      fx_formant_host(plane.data(), (long)n, src ? other.data() : nullptr, P.sr, P.v, out.data(), D, E, Es, g, s);
      for (int64_t i = 0; i < n; ++i) y[i * P.Cc + c] = out[i];
    }
  });
}

int rvcx_fx_pitch_shift_formant_host(const float* x, int64_t n, int channels, int sr, double semitones,
                                     const rvcx_fx_formant_params* params, float* y) {
  return host_call([&] {
    semitones_check("fx_pitch_shift_formant_host", semitones);
    const rvcx_fx_formant_params q = preserve_params(params, sr, channels);
    const FormantPlan P = formant_check("fx_pitch_shift_formant_host", &q);
    if (!x || !y) fail("fx_pitch_shift_formant_host: null pointer");
    length_check("fx_pitch_shift_formant_host", n);
    if (rvcx_fx_pitch_ratio(sr, semitones) == sr) {
      if (y != x) std::memcpy(y, x, (size_t)n * channels * 4);
      return;
    }
    std::vector<float> shifted((size_t)n * channels);
    if (rvcx_fx_pitch_shift_host(x, n, channels, sr, semitones, shifted.data(), nullptr, nullptr, nullptr, nullptr) != 0)
      fail(g_last_error);
    if (P.v.amount == 0.f) {
      std::memcpy(y, shifted.data(), shifted.size() * 4);
      return;
    }
    if (rvcx_fx_formant_host(shifted.data(), n, x, &q, y, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) fail(g_last_error);
  });
}

int rvcx_fx_formant_envelope_host(const float* L, int N, int nc, int iterations, float* E) {
  return host_call([&] {
    if (!L || !E) fail("fx_formant_envelope_host: null pointer");
    if (N < 512 || N > 8192 || (N & (N - 1)) != 0) fail("fx_formant_envelope_host: N must be a power of two within 512 .. 8192");
    if (nc < 1 || nc > N / 8) fail("fx_formant_envelope_host: 1 <= nc <= N / 8 is required");
    if (iterations < 0 || iterations > kFormantMaxIter) fail("fx_formant_envelope_host: iterations must lie in 0 .. 16");
    fx_formant_envelope_host(L, N, nc, iterations, E);
  });
}

}  // extern "C"
