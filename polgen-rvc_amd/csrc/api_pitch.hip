// C ABI of librvcx.so (include/rvcx.h): time stretch and pitch shift (stages 13 and 14), their taps and their host twins.
#include "api_fx_common.h"

// A2 of rvcx_fx_stretch_own_host is written out rounding by rounding, as in pitch.hip
#pragma clang fp contract(off)

using namespace rvcx;
using namespace rvcx::api;

namespace {

int g_chunk_frames = 0, g_segment_frames = 0;      // rvcx_fx_stretch_override; 0: the default

int chunk_frames() { return g_chunk_frames > 0 ? g_chunk_frames : kStretchChunk; }
int segment_frames() { return g_segment_frames > 0 ? g_segment_frames : kStretchSegment; }

void stretch_check(const char* who, int sr, int channels, int64_t P, int64_t Q) {
  check_rate(who, sr);
  check_channels(who, channels);
  if (!fx_stretch_ratio_ok((long)P, (long)Q)) fail(std::string(who) + ": 1 <= Q <= 2^20 and Q / 2 <= P <= 2 Q are required");
}

long pitch_check(const char* who, int sr, int channels, double semitones) {
  check_finite(who, {semitones});
  if (std::fabs(semitones) > 12.0) fail(std::string(who) + ": semitones must lie in -12 .. 12");
  const long P = fx_pitch_P(sr > 0 ? sr : 1, semitones);
  stretch_check(who, sr, channels, P, sr);
  return P;
}

// the int lengths of the device rows hold the stretched item too
void out_len_check(const char* who, int B, const int64_t* n, long P, long Q) {
  for (int b = 0; b < B; ++b)
    if (fx_stretch_len((long)n[b], P, Q) > (long)INT32_MAX) fail(std::string(who) + ": the stretched item exceeds 2^31 - 1 frames");
}

// events of one call, one set per segment, so that no segment has to be waited for before the next is enqueued
struct EventPool {
  std::vector<hipEvent_t> ev;
  hipEvent_t* take(int k) {
    const size_t at = ev.size();
    ev.resize(at + k);
    for (int i = 0; i < k; ++i) RVCX_HIP(hipEventCreate(&ev[at + i]));
    return ev.data() + at;
  }
  ~EventPool() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct StretchTaps {
  float* D = nullptr;
  int32_t* own = nullptr;
  uint32_t* TH = nullptr;
  uint32_t* R = nullptr;
  bool any() const { return D || own || TH || R; }
};

// stage 13 on B items, and behind it the resampler of stage 14 when `pitch` (then Q = sr and the output has n[b] frames)
void run_stretch(rvcx_ctx* ctx, Ctx* C, int B, const float* const* x, const int64_t* n, int Cc, int sr, long P, long Q,
                 bool pitch, float* const* y, const StretchTaps& taps) {
  const FxStretchGeom g = fx_stretch_geom(sr);
  const int S = segment_frames(), Lc = std::min(chunk_frames(), S);
  const size_t table_bytes = (size_t)g.N * 8 + (pitch ? resample_table_doubles(0) * 8 : 0) + ((size_t)1 << 20);
  auto item_bytes = [&](long n_long) {
    const long ld = pad256(n_long), lds = pad256(fx_stretch_len(n_long, P, Q)), Tf = fx_stretch_T(n_long, g.H) + 2;
    return (size_t)Cc * ((size_t)std::max(ld, lds) * 4 + (size_t)ld * 8 + (size_t)lds * 4 +
                         fx_stretch_row_bytes(g, Tf, S, Lc, taps.D != nullptr) + 16 * 256 + 64);
  };
  const size_t worst = item_bytes((long)*std::max_element(n, n + B));
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
    const long nmax = (long)*std::max_element(n + g0, n + g0 + Bg);
    const long ld = pad256(nmax), lds = pad256(fx_stretch_len(nmax, P, Q)), ldm = std::max(ld, lds);
    const long Tmax = fx_stretch_T(nmax, g.H), Jmax = fx_stretch_J(Tmax, P, Q);
    const int nch = (S + Lc - 1) / Lc;
    const size_t nb = (size_t)g.nb;
    A.reset();
    FxStretchDev d{};
    tables.upload(*C, d.w, d.tw);
    ResampleFilter rf;
    if (pitch) rf = make_resample_filter(A, (int)P, sr, s, 0);
    d.g = g, d.P = P, d.Q = Q, d.R = R, d.ld = ld, d.Tf = Tmax + 2, d.S = S, d.Lc = Lc;
    float* stage = A.alloc<float>((size_t)Bg * Cc * ldm);
    float* rows = A.alloc<float>((size_t)R * ld);
    float* ys = A.alloc<float>((size_t)R * lds);
    float* yo = pitch ? A.alloc<float>((size_t)R * ld) : nullptr;
    const size_t fb = (size_t)R * d.Tf * nb;
    d.D = taps.D ? A.alloc<float2>(fb) : nullptr;
    d.A2 = A.alloc<float>(fb);
    d.TH = A.alloc<uint32_t>(fb);
    d.own = A.alloc<int>(fb);
    d.Rseg = A.alloc<uint32_t>((size_t)R * S * nb);
    d.Rcarry = A.alloc<uint32_t>((size_t)R * nb);
    d.par = A.alloc<int>((size_t)R * nch * nb);
    d.off = A.alloc<uint32_t>((size_t)R * nch * nb);
    d.Rstart = A.alloc<uint32_t>((size_t)R * (nch + 1) * nb);
    d.fr = A.alloc<float>((size_t)R * (S + 3) * g.N);
    d.tmp3 = A.alloc<float>((size_t)R * 3 * g.N);
    std::vector<int> len = row_lengths(n + g0, Bg, Cc);       // the R rows as they come, then the R rows as they leave
    for (int r = 0; r < R; ++r) len.push_back(pitch ? len[r] : (int)fx_stretch_len(len[r], P, Q));
    T.mark(0);
    const int* dlen = d.len = to_dev(*C, len.data(), len.size());
    stage_in([&](int b) { return std::make_pair(x[g0 + b], n[g0 + b]); }, Bg, Cc, ld, stage, rows, dlen, s);
    RVCX_HIP(hipMemsetAsync(d.Rcarry, 0, (size_t)R * nb * 4, s));           // R_0 = 0
    T.mark(1);
    launch_stretch_analysis(d, rows, s, T.ev + 2);
    if (taps.any()) {
      const size_t cnt = (size_t)(fx_stretch_T(len[0], g.H) + 2) * nb;       // taps: one row
      if (taps.D) RVCX_HIP(hipMemcpyAsync(taps.D, d.D, cnt * 8, hipMemcpyDefault, s));
      if (taps.own) RVCX_HIP(hipMemcpyAsync(taps.own, d.own, cnt * 4, hipMemcpyDefault, s));
      if (taps.TH) RVCX_HIP(hipMemcpyAsync(taps.TH, d.TH, cnt * 4, hipMemcpyDefault, s));
    }
    // the segments are enqueued one behind the other; each has its own four events, read once the group is done
    EventPool pool;
    const long nseg = (Jmax + S - 1) / S;
    pool.ev.reserve((size_t)nseg * 4);
    for (long s0 = 0; s0 < Jmax; s0 += S) {
      launch_stretch_segment(d, s0, ys, lds, s, pool.take(4));
      if (taps.R) {       // (stream order: the copy reads Rseg before the next segment's scan writes it)
        const long j1 = std::min<long>(s0 + S, Jmax);
        RVCX_HIP(hipMemcpyAsync(taps.R + (size_t)s0 * nb, d.Rseg, (size_t)(j1 - s0) * nb * 4, hipMemcpyDefault, s));
      }
    }
    T.mark(8);
    const float* res = ys;
    long ldo = lds;
    if (pitch) {
      RVCX_HIP(hipMemsetAsync(yo, 0, (size_t)R * ld * 4, s));               // zero-padded to n where the resampler ends early
      for (int r = 0; r < R; ++r) {                                           // one launch per channel plane
        const long ns = fx_stretch_len(len[r], P, Q);
        const long no = std::min<long>(resample_out_len(ns, (int)P, sr), len[r]);
        launch_resample_plane_f32(rf, ys + (size_t)r * lds, ns, yo + (size_t)r * ld, no, s);
      }
      res = yo, ldo = ld;
    }
    T.mark(9);
    stage_out(res, dlen + R, Bg, Cc, ldo, stage, s, [&](int b) { return std::make_pair(y[g0 + b], (int64_t)len[R + b * Cc]); });
    T.mark(10);
    RVCX_HIP(hipStreamSynchronize(s));
    // {copies in, transforms, owners, scan, inverse transforms, overlap-add, resampler, copies out, total}
    T.add_each(0, 0, 3);
    for (size_t k = 0; k + 3 < pool.ev.size(); k += 4)
      T.add(3, pool.ev[k], pool.ev[k + 1]), T.add(4, pool.ev[k + 1], pool.ev[k + 2]), T.add(5, pool.ev[k + 2], pool.ev[k + 3]);
    T.add(6, 8, 9), T.add(7, 9, 10), T.add(8, 0, 10);
  }
  A.reset();
  T.store(*C);
  ctx->fx_groups = groups;
}

void host_stretch(const char* who, const float* x, int64_t n, int channels, int sr, long P, long Q, bool pitch, float* y,
                  const StretchTaps& taps) {
  if (!x || !y) fail(std::string(who) + ": null pointer");
  check_frames(who, n, "1 .. 2^30 frames are required");
  if (taps.any() && channels != 1) fail(std::string(who) + ": the taps take one channel");
  out_len_check(who, 1, &n, P, Q);
  const long ns = fx_stretch_len((long)n, P, Q), no = pitch ? (long)n : ns;
  std::vector<float> st((size_t)std::max<long>(ns, 1)), out((size_t)(pitch ? no : 0));
  host_planes(x, n, channels, y, no, [&](int, const float* plane) -> const float* {
    fx_stretch_host(plane, (long)n, sr, P, Q, st.data(), taps.D, taps.own, taps.TH, taps.R);
    if (!pitch) return st.data();
    std::fill(out.begin(), out.end(), 0.f);
    resample_plane_host((int)P, sr, st.data(), ns, out.data(), std::min<long>(resample_out_len(ns, (int)P, sr), (long)n));
    return out.data();
  });
}

}  // namespace

extern "C" {

int rvcx_fx_stretch_chunk(void) { return chunk_frames(); }

int rvcx_fx_stretch_override(int chunk, int segment) {
  REQUIRE_DEBUG(nullptr, "rvcx_fx_stretch_override")
  if (chunk < 0 || segment < 0 || chunk > 4096 || segment > 4096) {
    g_last_error = "rvcx_fx_stretch_override: lengths of 0 .. 4096 frames";
    return -1;
  }
  g_chunk_frames = chunk, g_segment_frames = segment;
  return 0;
}

int64_t rvcx_fx_stretch_len(int64_t n, int64_t P, int64_t Q) {
  return (n >= 0 && n <= (int64_t)1 << 30 && fx_stretch_ratio_ok((long)P, (long)Q)) ? fx_stretch_len((long)n, (long)P, (long)Q) : -1;
}

int rvcx_fx_stretch_frames(int64_t n, int sr, int64_t P, int64_t Q, int64_t* T, int64_t* J, int32_t* N) {
  return host_call([&] {
    stretch_check("fx_stretch_frames", sr, 1, P, Q);
    check_frames("fx_stretch_frames", n, "1 .. 2^30 frames are required");
    const FxStretchGeom g = fx_stretch_geom(sr);
    const long t = fx_stretch_T((long)n, g.H);
    if (T) *T = t;
    if (J) *J = fx_stretch_J(t, (long)P, (long)Q);
    if (N) *N = g.N;
  });
}

int64_t rvcx_fx_pitch_ratio(int sr, double semitones) {
  return (fx_rate_ok(sr) && std::isfinite(semitones) && std::fabs(semitones) <= 12.0) ? fx_pitch_P(sr, semitones) : -1;
}

int rvcx_fx_stretch(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, int channels, int sr, int64_t P, int64_t Q,
                    float* const* y) {
  API_BEGIN(ctx)
  stretch_check("fx_stretch", sr, channels, P, Q);
  check_items("fx_stretch", B, x, n, y);
  out_len_check("fx_stretch", B, n, (long)P, (long)Q);
  run_stretch(ctx, C, B, x, n, channels, sr, (long)P, (long)Q, false, y, StretchTaps{});
  API_END
}

int rvcx_fx_pitch_shift(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, int channels, int sr, double semitones,
                        float* const* y) {
  API_BEGIN(ctx)
  const long P = pitch_check("fx_pitch_shift", sr, channels, semitones);
  check_items("fx_pitch_shift", B, x, n, y);
  if (P == sr) return fx_skip(ctx, B, x, n, channels, y);
  out_len_check("fx_pitch_shift", B, n, P, sr);
  run_stretch(ctx, C, B, x, n, channels, sr, P, sr, true, y, StretchTaps{});
  API_END
}

int rvcx_op_fx_stretch_taps(rvcx_ctx* ctx, const float* x, int64_t n, int sr, int64_t P, int64_t Q, float* y, float* D,
                            int32_t* own, uint32_t* TH, uint32_t* R) {
  API_BEGIN(ctx)
  stretch_check("op_fx_stretch_taps", sr, 1, P, Q);
  check_items("op_fx_stretch_taps", 1, &x, &n, &y);
  out_len_check("op_fx_stretch_taps", 1, &n, (long)P, (long)Q);
  StretchTaps t;
  t.D = D, t.own = own, t.TH = TH, t.R = R;
  run_stretch(ctx, C, 1, &x, &n, 1, sr, (long)P, (long)Q, false, &y, t);
  API_END
}

// ---- host only -----------------------------------------------------------------------------------------------------------------
int rvcx_fx_stretch_host(const float* x, int64_t n, int channels, int sr, int64_t P, int64_t Q, float* y, float* D, int32_t* own,
                         uint32_t* TH, uint32_t* R) {
  return host_call([&] {
    stretch_check("fx_stretch_host", sr, channels, P, Q);
    StretchTaps t;
    t.D = D, t.own = own, t.TH = TH, t.R = R;
    host_stretch("fx_stretch_host", x, n, channels, sr, (long)P, (long)Q, false, y, t);
  });
}

int rvcx_fx_pitch_shift_host(const float* x, int64_t n, int channels, int sr, double semitones, float* y, float* D, int32_t* own,
                             uint32_t* TH, uint32_t* R) {
  return host_call([&] {
    const long P = pitch_check("fx_pitch_shift_host", sr, channels, semitones);
    if (!x || !y) fail("fx_pitch_shift_host: null pointer");
    check_frames("fx_pitch_shift_host", n, "1 .. 2^30 frames are required");
    if (P == sr) {
      if (D || own || TH || R) fail("fx_pitch_shift_host: the stage is skipped at this shift, it has no taps");
      if (y != x) std::memcpy(y, x, (size_t)n * channels * 4);
      return;
    }
    StretchTaps t;
    t.D = D, t.own = own, t.TH = TH, t.R = R;
    host_stretch("fx_pitch_shift_host", x, n, channels, sr, P, sr, true, y, t);
  });
}

int rvcx_fx_stretch_own_host(const float* D, int nb, int32_t* own) {
  return host_call([&] {
    if (!D || !own || nb < 1 || nb > 4097) fail("fx_stretch_own_host: null pointer or nb outside 1 .. 4097");
    std::vector<float> A2((size_t)nb);
    for (int k = 0; k < nb; ++k) {
      const float rr = D[2 * k] * D[2 * k], ii = D[2 * k + 1] * D[2 * k + 1];
      A2[k] = rr + ii;
    }
    fx_stretch_own_host(A2.data(), nb, own);
  });
}

}  // extern "C"
