// C ABI of librvcx.so (include/rvcx.h): formant shift and envelope transfer (stage 17), the formant-preserving pitch shift
// (stage 18), their taps and their host twins.
#include "api_fx_common.h"
#include "formant.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

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
  check_rate(who_c, p->sample_rate);
  check_channels(who_c, p->channels);
  check_finite(who_c, {p->ratio, p->amount, p->quefrency_ms, p->max_gain_db});
  check_range(who_c, p->ratio, 0.5, 2.0, "ratio");
  check_range(who_c, p->amount, 0.0, 1.0, "amount");
  check_range(who_c, p->max_gain_db, 0.0, 48.0, "max_gain_db");
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

void fit_check(const char* who, Ctx* C, const FormantPlan& P, int B, const int64_t* n, const float* const* src, bool taps = false) {
  for (int b = 0; b < B; ++b)
    if (item_runs(P, src, b)) check_item_fits(who, *C, b, n[b], item_bytes(P, (long)n[b], src && src[b], taps) + table_bytes(P));
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
  // the items that are not skipped, in call order: their tables side by side (rs: null where an item has no source)
  std::vector<const float*> rx, rs;
  std::vector<float*> ry;
  std::vector<int64_t> rn;
  bool any_src = false;
  size_t own_max = 0;                      // the largest item on its own (fit_check has passed it)
  for (int b = 0; b < B; ++b) {
    if (!item_runs(P, src, b)) {
      copy_through(1, x + b, n + b, Cc, y + b);
      continue;
    }
    rx.push_back(x[b]), rs.push_back(src ? src[b] : nullptr), ry.push_back(y[b]), rn.push_back(n[b]);
    any_src = any_src || rs.back();
    own_max = std::max(own_max, item_bytes(P, (long)n[b], rs.back(), taps.any()));
  }
  std::fill(ms4, ms4 + 4, 0.f);
  ctx->fx_groups = 0;
  if (rx.empty()) return;
  const int Br = (int)rx.size();
  const size_t tb = table_bytes(P), worst = item_bytes(P, (long)*std::max_element(rn.begin(), rn.end()), any_src, taps.any());
  const int G = fx_group_size(*C, Br, worst, tb);
  Arena& A = C->arena;
  A.reset();
  A.reserve((G > 1 ? worst * G : own_max) + tb);
  hipStream_t s = C->stream;
  FxTimer T(*C);
  const StftTables tables(g.N);
  int groups = 0;
  for (int g0 = 0; g0 < Br; g0 += G, ++groups) {
    const int Bg = std::min(G, Br - g0), R = Bg * Cc;
    const long nmax = (long)*std::max_element(rn.begin() + g0, rn.begin() + g0 + Bg);
    const bool gsrc = std::any_of(rs.begin() + g0, rs.begin() + g0 + Bg, [](const float* z) { return z != nullptr; });
    const long ld = pad256(nmax);
    A.reset();
    FxFormantDev d{};
    tables.upload(*C, d.w, d.tw);
    d.g = g, d.v = P.v, d.nc = P.nc, d.limit = fx_formant_limit(P.v.max_gain_db), d.R = R, d.ld = ld;
    d.Tf = fx_stretch_T(nmax, g.H);
    float* stage = A.alloc<float>((size_t)R * ld);
    float* rows = A.alloc<float>((size_t)R * ld);
    float* ys = A.alloc<float>((size_t)R * ld);
    float *stage_s = nullptr, *rows_s = nullptr;
    if (gsrc) {
      stage_s = A.alloc<float>((size_t)R * ld);
      rows_s = A.alloc<float>((size_t)R * ld);
    }
    d.fr = A.alloc<float>((size_t)R * d.Tf * g.N);
    d.x = rows, d.src = rows_s;
    const size_t cnt = (size_t)fx_stretch_T((long)rn[g0], g.H) * g.nb;             // taps: one row
    if (taps.D) d.taps.D = A.alloc<float2>(cnt);
    if (taps.E) d.taps.E = A.alloc<float>(cnt);
    if (taps.Es) d.taps.Es = A.alloc<float>(cnt);
    if (taps.g) d.taps.g = A.alloc<float>(cnt);
    if (taps.s) d.taps.s = A.alloc<float>((size_t)d.Tf);
    std::vector<int> len = row_lengths(rn.data() + g0, Bg, Cc);       // the rows' frames, then whether each row has a source
    for (int r = 0; r < R; ++r) len.push_back(rs[g0 + r / Cc] ? 1 : 0);
    T.mark(0);
    const int* dlen = to_dev(*C, len.data(), len.size());
    d.len = dlen, d.has_src = dlen + R;
    stage_in([&](int i) { return std::make_pair(rx[g0 + i], rn[g0 + i]); }, Bg, Cc, ld, stage, rows, dlen, s);
    if (gsrc) {
      RVCX_HIP(hipMemsetAsync(stage_s, 0, (size_t)R * ld * 4, s));                  // (rows without a source are never read)
      stage_in([&](int i) { return std::make_pair(rs[g0 + i], rn[g0 + i]); }, Bg, Cc, ld, stage_s, rows_s, dlen, s);
    }
    T.mark(1);
    launch_formant(d, ys, ld, s, T.ev + 2);
    if (taps.D) RVCX_HIP(hipMemcpyAsync(taps.D, d.taps.D, cnt * 8, hipMemcpyDefault, s));
    if (taps.E) RVCX_HIP(hipMemcpyAsync(taps.E, d.taps.E, cnt * 4, hipMemcpyDefault, s));
    if (taps.Es) RVCX_HIP(hipMemcpyAsync(taps.Es, d.taps.Es, cnt * 4, hipMemcpyDefault, s));
    if (taps.g) RVCX_HIP(hipMemcpyAsync(taps.g, d.taps.g, cnt * 4, hipMemcpyDefault, s));
    if (taps.s) RVCX_HIP(hipMemcpyAsync(taps.s, d.taps.s, (size_t)fx_stretch_T((long)rn[g0], g.H) * 4, hipMemcpyDefault, s));
    stage_out(ys, dlen, Bg, Cc, ld, stage, s, [&](int i) { return std::make_pair(ry[g0 + i], rn[g0 + i]); });
    T.mark(4);
    RVCX_HIP(hipStreamSynchronize(s));
    T.add_each(0, 0, 4);
  }
  A.reset();
  std::copy(T.ms, T.ms + 4, ms4);
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

// stage 18's parameters: the caller's (or the defaults) on the call's shape, with ratio 1
rvcx_fx_formant_params preserve_params(const rvcx_fx_formant_params* p, int sr, int channels) {
  rvcx_fx_formant_params q = p ? *p : kFormantDefaults;
  q.sample_rate = sr, q.channels = channels, q.ratio = 1.f;
  return q;
}

void semitones_check(const char* who, double semitones) {
  check_finite(who, {semitones});
  if (std::fabs(semitones) > 12.0) fail(std::string(who) + ": semitones must lie in -12 .. 12");
}

}  // namespace

extern "C" {

int rvcx_fx_formant_frames(int64_t n, int sr, float quefrency_ms, int64_t* T, int32_t* N, int32_t* nc) {
  return host_call([&] {
    rvcx_fx_formant_params p = kFormantDefaults;
    p.sample_rate = sr, p.channels = 1, p.quefrency_ms = quefrency_ms;
    const FormantPlan P = formant_check("fx_formant_frames", &p);
    check_frames("fx_formant_frames", n);
    if (T) *T = fx_stretch_T((long)n, P.g.H);
    if (N) *N = P.g.N;
    if (nc) *nc = P.nc;
  });
}

int rvcx_fx_formant(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, const float* const* src,
                    const rvcx_fx_formant_params* params, float* const* y) {
  API_BEGIN(ctx)
  const FormantPlan P = formant_check("fx_formant", params);
  check_items("fx_formant", B, x, n, y);
  if (stage_skipped(P, B, src)) return fx_skip(ctx, B, x, n, P.Cc, y);
  float ms4[4] = {0};
  run_formant(ctx, C, P, B, x, n, src, y, FormantTaps{}, ms4);
  set_timing(C, ms4, 0.f);
  API_END
}

int rvcx_fx_pitch_shift_formant(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, int channels, int sr,
                                double semitones, const rvcx_fx_formant_params* params, float* const* y) {
  API_BEGIN(ctx)
  semitones_check("fx_pitch_shift_formant", semitones);
  const rvcx_fx_formant_params q = preserve_params(params, sr, channels);
  const FormantPlan P = formant_check("fx_pitch_shift_formant", &q);
  check_items("fx_pitch_shift_formant", B, x, n, y);
  float ms4[4] = {0};
  if (rvcx_fx_pitch_ratio(sr, semitones) == sr) return fx_skip(ctx, B, x, n, channels, y);
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
  check_frames("op_fx_formant_taps", n);
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
    check_frames("fx_formant_host", n);
    const bool taps = D || E || Es || g || s;
    if (taps && P.Cc != 1) fail("fx_formant_host: the taps take one channel");
    if (stage_skipped(P, 1, src ? &src : nullptr)) {
      if (taps) fail("fx_formant_host: the stage is skipped at these values, it has no taps");
      if (y != x) std::memcpy(y, x, (size_t)n * P.Cc * 4);
      return;
    }
    std::vector<float> other, out((size_t)n);
    host_planes(x, n, P.Cc, y, n, [&](int c, const float* plane) {
      if (src) take_plane(src, n, P.Cc, c, other);
      fx_formant_host(plane, (long)n, src ? other.data() : nullptr, P.sr, P.v, out.data(), D, E, Es, g, s);
      return out.data();
    });
  });
}

int rvcx_fx_pitch_shift_formant_host(const float* x, int64_t n, int channels, int sr, double semitones,
                                     const rvcx_fx_formant_params* params, float* y) {
  return host_call([&] {
    semitones_check("fx_pitch_shift_formant_host", semitones);
    const rvcx_fx_formant_params q = preserve_params(params, sr, channels);
    const FormantPlan P = formant_check("fx_pitch_shift_formant_host", &q);
    if (!x || !y) fail("fx_pitch_shift_formant_host: null pointer");
    check_frames("fx_pitch_shift_formant_host", n);
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
