// C ABI of librvcx.so (include/rvcx.h): loudness metering, true peak, limiter and the loudness-matched master (stages 9 - 12),
// and their host twins.
#include "api_fx_common.h"
#include "effects_device.h"

// the host twins' roundings are written out, as in loudness.hip
#pragma clang fp contract(off)

using namespace rvcx;
using namespace rvcx::api;

namespace {

void loud_check(const char* who, int sr, int channels) {
  check_rate(who, sr);
  check_channels(who, channels);
}

void limit_check(const char* who, double ceiling_db, double lookahead_ms, double release_ms) {
  check_finite(who, {ceiling_db, lookahead_ms, release_ms});
  if (ceiling_db > 0.0) fail(std::string(who) + ": the ceiling must be <= 0 dB");
  if (lookahead_ms < 0.0 || lookahead_ms > 10.0) fail(std::string(who) + ": lookahead_ms must lie in 0 .. 10");
  if (release_ms < 0.0 || release_ms > 10000.0) fail(std::string(who) + ": release_ms must lie in 0 .. 10000");
}

void master_check(const char* who, int sr, double target, double offset, double ceiling) {
  loud_check(who, sr, 2);
  check_finite(who, {target, offset});
  if (target > 0.0) fail(std::string(who) + ": target_lufs must be <= 0");
  limit_check(who, ceiling, 2.0, 100.0);
}

float bits_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// the group size at this item size, and the arena reserved for it (1 MiB beside the items for the small tables)
int fx_group(Ctx* C, int B, size_t item_bytes) {
  const int G = fx_group_size(*C, B, item_bytes, 0);
  C->arena.reset();
  C->arena.reserve(item_bytes * G + ((size_t)1 << 20));
  return G;
}

}  // namespace

extern "C" {

int64_t rvcx_fx_momentary_len(int64_t n, int sr) { return fx_rate_ok(sr) && n > 0 ? fx_momentary_len((long)n, sr) : 0; }

int rvcx_fx_loudness(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, int channels, int sr, double* lufs,
                     double* tp_db, float* const* momentary) {
  API_BEGIN(ctx)
  loud_check("fx_loudness", sr, channels);
  check_items("fx_loudness", B, x, n);
  if (!lufs) fail("fx_loudness: null argument");
  for (int b = 0; b < B; ++b)
    if (momentary && fx_momentary_len((long)n[b], sr) > 0 && !momentary[b]) fail("fx_loudness: null pointer in a table");
  const int Cc = channels;
  const long ld_max = fx_ld(*std::max_element(n, n + B));
  const size_t item = (size_t)ld_max * Cc * 8 + fx_loudness_scratch_bytes(1, Cc, ld_max, sr) + (size_t)(ld_max / (sr / 10) + 1) * 4 + 8192;
  const int G = fx_group(C, B, item);
  Arena& A = C->arena;
  hipStream_t s = C->stream;
  FxTimer T(*C);
  std::vector<double> L((size_t)B);
  std::vector<uint32_t> pk((size_t)B, 0);
  std::vector<std::vector<float>> mom((size_t)B);
  const FxKWeight kw = fx_kweight(sr);
  int groups = 0;
  for (int g0 = 0; g0 < B; g0 += G, ++groups) {
    const int Bg = std::min(G, B - g0), R = Bg * Cc;
    const long ld = fx_ld(*std::max_element(n + g0, n + g0 + Bg));
    const size_t plane = (size_t)R * ld;
    const long mom_ld = fx_momentary_len(ld, sr) + 1;
    A.reset();
    float* stage = A.alloc<float>(plane);
    float* rows = A.alloc<float>(plane);
    void* scratch = A.alloc<char>(fx_loudness_scratch_bytes(Bg, Cc, ld, sr));
    double* dl = A.alloc<double>((size_t)Bg);
    uint32_t* dpk = A.alloc<uint32_t>((size_t)Bg);
    float* dmom = momentary ? A.alloc<float>((size_t)Bg * mom_ld) : nullptr;
    const std::vector<int> len = row_lengths(n + g0, Bg, Cc);
    T.mark(0);
    const int* dlen = to_dev(*C, len.data(), len.size());
    stage_in([&](int b) { return std::make_pair(x[g0 + b], n[g0 + b]); }, Bg, Cc, ld, stage, rows, dlen, s);
    T.mark(1);
    launch_fx_loudness(kw, rows, dlen, Bg, Cc, ld, sr, scratch, dl, dmom, mom_ld, s, T.ev + 2);
    if (tp_db) launch_fx_truepeak(rows, dlen, Bg, Cc, ld, nullptr, dpk, s);
    T.mark(6);
    RVCX_HIP(hipMemcpyAsync(L.data() + g0, dl, (size_t)Bg * sizeof(double), hipMemcpyDeviceToHost, s));
    if (tp_db) RVCX_HIP(hipMemcpyAsync(pk.data() + g0, dpk, (size_t)Bg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (momentary)
      for (int b = 0; b < Bg; ++b) {
        const long nb = fx_momentary_len((long)n[g0 + b], sr);
        mom[g0 + b].resize((size_t)nb);
        if (nb) RVCX_HIP(hipMemcpyAsync(mom[g0 + b].data(), dmom + (size_t)b * mom_ld, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
      }
    T.mark(7);
    RVCX_HIP(hipStreamSynchronize(s));
    // {copies + layout, local, carry, apply + energy, gates, true peak, copies back, -, total}
    T.add_each(0, 0, 7), T.add(8, 0, 7);
  }
  A.reset();
  // everything is in: the caller's memory is written only now
  for (int b = 0; b < B; ++b) {
    lufs[b] = L[b];
    if (tp_db) tp_db[b] = fx_db20(bits_float(pk[b]));
    if (momentary && !mom[b].empty()) RVCX_HIP(hipMemcpy(momentary[b], mom[b].data(), mom[b].size() * 4, hipMemcpyDefault));
  }
  T.store(*C);
  ctx->fx_groups = groups;
  API_END
}

int rvcx_op_fx_truepeak(rvcx_ctx* ctx, const float* x, int64_t n, int channels, float* p_out, double* tp_db) {
  API_BEGIN(ctx)
  loud_check("op_fx_truepeak", 48000, channels);
  check_items("op_fx_truepeak", 1, &x, &n);
  if (!tp_db) fail("op_fx_truepeak: null argument");
  const long ld = fx_ld(n);
  const int Cc = channels;
  Arena& A = C->arena;
  A.reset();
  A.reserve((size_t)ld * 4 * (2 * Cc + 1) + ((size_t)1 << 20));
  hipStream_t s = C->stream;
  float* stage = A.alloc<float>((size_t)ld * Cc);
  float* rows = A.alloc<float>((size_t)ld * Cc);
  float* p = A.alloc<float>((size_t)ld);
  uint32_t* dpk = A.alloc<uint32_t>(1);
  const int len[2] = {(int)n, (int)n};
  const int* dlen = to_dev(*C, len, 2);
  stage_in([&](int) { return std::make_pair(x, n); }, 1, Cc, ld, stage, rows, dlen, s);
  launch_fx_truepeak(rows, dlen, 1, Cc, ld, p, dpk, s);
  uint32_t pk = 0;
  RVCX_HIP(hipMemcpyAsync(&pk, dpk, sizeof(pk), hipMemcpyDeviceToHost, s));
  if (p_out) RVCX_HIP(hipMemcpyAsync(p_out, p, (size_t)n * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  *tp_db = fx_db20(bits_float(pk));
  A.reset();
  API_END
}

int rvcx_op_fx_limit(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float ceiling_db, float lookahead_ms,
                     float release_ms, float* y, float* gain) {
  API_BEGIN(ctx)
  loud_check("op_fx_limit", sr, channels);
  limit_check("op_fx_limit", ceiling_db, lookahead_ms, release_ms);
  check_items("op_fx_limit", 1, &x, &n);
  if (!y) fail("op_fx_limit: null argument");
  const long ld = fx_ld(n);
  const int Cc = channels;
  const size_t nch = (size_t)(ld / kFxChunk);
  Arena& A = C->arena;
  A.reset();
  A.reserve((size_t)ld * 4 * (2 * Cc + 4) + nch * 12 + ((size_t)1 << 20));
  hipStream_t s = C->stream;
  float* stage = A.alloc<float>((size_t)ld * Cc);
  float* rows = A.alloc<float>((size_t)ld * Cc);
  float* p = A.alloc<float>((size_t)ld);
  float* u = A.alloc<float>((size_t)ld);
  float* e = A.alloc<float>((size_t)ld);
  float* sg = A.alloc<float>((size_t)ld);
  float* state = A.alloc<float>(3 * nch + 64);
  uint32_t* dpk = A.alloc<uint32_t>(2);
  const int len[2] = {(int)n, (int)n};
  const int* dlen = to_dev(*C, len, 2);
  stage_in([&](int) { return std::make_pair(x, n); }, 1, Cc, ld, stage, rows, dlen, s);
  launch_fx_truepeak(rows, dlen, 1, Cc, ld, p, dpk, s);
  uint32_t pk = 0;
  RVCX_HIP(hipMemcpyAsync(&pk, dpk, sizeof(pk), hipMemcpyDeviceToHost, s));
  RVCX_HIP(hipStreamSynchronize(s));       // the skip decision needs the peak
  const float c = (float)std::pow(10.0, (double)ceiling_db / 20.0);
  if (bits_float(pk) <= c) {               // skip: nothing is launched, the output is the input bit for bit
    if (y != x) RVCX_HIP(hipMemcpyAsync(y, x, (size_t)n * Cc * 4, hipMemcpyDefault, s));
    if (gain) {
      const std::vector<float> one((size_t)n, 1.f);
      RVCX_HIP(hipMemcpyAsync(gain, one.data(), (size_t)n * 4, hipMemcpyDefault, s));
      RVCX_HIP(hipStreamSynchronize(s));
    }
  } else {
    ctx->fx_passes[0] = launch_fx_limit_gain(p, dlen, len, 1, ld, c, fx_lookahead(sr, lookahead_ms), fx_cte(release_ms, sr), u, e,
                                             state, sg, dpk + 1, s);
    launch_fx_limit_apply(rows, sg, dlen, 1, Cc, ld, nullptr, stage, nullptr, s);
    RVCX_HIP(hipMemcpyAsync(y, stage, (size_t)n * Cc * 4, hipMemcpyDefault, s));
    if (gain) RVCX_HIP(hipMemcpyAsync(gain, sg, (size_t)n * 4, hipMemcpyDefault, s));
  }
  RVCX_HIP(hipStreamSynchronize(s));
  A.reset();
  API_END
}

int rvcx_fx_master(rvcx_ctx* ctx, int B, const float* const* vocal, const int64_t* n_v, const float* const* inst,
                   const int64_t* n_i, int sr, double target_lufs, double vocal_offset_lu, double ceiling_dbtp,
                   int16_t* const* out, double* report7) {
  API_BEGIN(ctx)
  master_check("fx_master", sr, target_lufs, vocal_offset_lu, ceiling_dbtp);
  check_items("fx_master", B, vocal, n_v);
  if (!inst || !n_i || !out) fail("fx_master: null argument");
  for (int b = 0; b < B; ++b) {
    if (n_i[b] < 0 || n_i[b] > (int64_t)1 << 30) fail("fx_master: an instrumental needs 0 .. 2^30 frames");
    if ((n_i[b] && !inst[b]) || !out[b]) fail("fx_master: null pointer in a table");
  }
  const long ld_max = fx_ld(*std::max_element(n_v, n_v + B));
  const size_t item = (size_t)ld_max * 56 + fx_loudness_scratch_bytes(1, 2, ld_max, sr) + (size_t)(ld_max / kFxChunk) * 12 + 8192;
  const int G = fx_group(C, B, item);
  Arena& A = C->arena;
  hipStream_t s = C->stream;
  FxTimer T(*C);
  const FxKWeight kw = fx_kweight(sr);
  const float c = (float)std::pow(10.0, ceiling_dbtp / 20.0), c_rel = fx_cte(100.0, sr);
  const int W = fx_lookahead(sr, 2.0);
  std::vector<double> rep((size_t)B * 7);
  std::vector<std::vector<int16_t>> pcm_host((size_t)B);
  int groups = 0;
  for (int g0 = 0; g0 < B; g0 += G, ++groups) {
    const int Bg = std::min(G, B - g0), R = Bg * 2;
    const long ld = fx_ld(*std::max_element(n_v + g0, n_v + g0 + Bg));
    const size_t plane = (size_t)R * ld, nch = (size_t)(ld / kFxChunk);
    A.reset();
    float* stage = A.alloc<float>(plane);
    float* V = A.alloc<float>(plane);
    float* I = A.alloc<float>(plane);
    float* p = A.alloc<float>((size_t)Bg * ld);
    float* u = A.alloc<float>((size_t)Bg * ld);
    float* e = A.alloc<float>((size_t)Bg * ld);
    float* sg = A.alloc<float>((size_t)Bg * ld);
    int16_t* pcm = A.alloc<int16_t>(plane);
    float* state = A.alloc<float>(3 * (size_t)Bg * nch + 64);
    void* scratch = A.alloc<char>(fx_loudness_scratch_bytes(Bg, 2, ld, sr));
    double* dl = A.alloc<double>((size_t)Bg * 2);
    uint32_t* dpk = A.alloc<uint32_t>((size_t)Bg * 2);
    float* dg = A.alloc<float>((size_t)Bg * 2);
    std::vector<int> len((size_t)R * 2 + Bg);       // the vocals' rows, the instrumentals' rows (cut to their vocal), the items
    for (int b = 0; b < Bg; ++b) {
      const int nv = (int)n_v[g0 + b], ni = (int)std::min(n_i[g0 + b], n_v[g0 + b]);
      len[2 * b] = len[2 * b + 1] = nv, len[R + 2 * b] = len[R + 2 * b + 1] = ni, len[2 * R + b] = nv;
    }
    std::vector<double> L((size_t)Bg * 2), Lm((size_t)Bg), Lr((size_t)Bg);
    std::vector<float> gains((size_t)Bg * 2), gm((size_t)Bg);
    std::vector<uint32_t> pk((size_t)Bg * 2), low((size_t)Bg, 0x3f800000u);
    T.mark(0);
    const int* dlen_v = to_dev(*C, len.data(), len.size());
    const int *dlen_i = dlen_v + R, *dilen = dlen_v + 2 * R;
    // both stems pass through the one staging buffer (stream order); an empty instrumental copies nothing and has no frames to read
    stage_in([&](int b) { return std::make_pair(vocal[g0 + b], n_v[g0 + b]); }, Bg, 2, ld, stage, V, dlen_v, s);
    stage_in([&](int b) { return std::make_pair(inst[g0 + b], (int64_t)len[R + 2 * b]); }, Bg, 2, ld, stage, I, dlen_i, s);
    T.mark(1);
    // the stems
    launch_fx_loudness(kw, V, dlen_v, Bg, 2, ld, sr, scratch, dl, nullptr, 0, s, nullptr);
    launch_fx_loudness(kw, I, dlen_i, Bg, 2, ld, sr, scratch, dl + Bg, nullptr, 0, s, nullptr);
    T.mark(2);
    RVCX_HIP(hipMemcpyAsync(L.data(), dl, L.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));      // the gains are formed on the host in double, as the host twin forms them
    for (int b = 0; b < Bg; ++b) {
      gains[b] = (float)fx_gain_to(target_lufs + vocal_offset_lu, L[b]);
      gains[Bg + b] = (float)fx_gain_to(target_lufs, L[Bg + b]);
    }
    RVCX_HIP(hipMemcpyAsync(dg, gains.data(), gains.size() * sizeof(float), hipMemcpyHostToDevice, s));
    launch_fx_master_mix(V, I, dlen_v, dlen_i, dg, dg + Bg, Bg, 2, ld, s);
    T.mark(3);
    launch_fx_loudness(kw, V, dlen_v, Bg, 2, ld, sr, scratch, dl, nullptr, 0, s, nullptr);
    T.mark(4);
    RVCX_HIP(hipMemcpyAsync(Lm.data(), dl, Lm.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < Bg; ++b) gm[b] = (float)fx_gain_to(target_lufs, Lm[b]);
    RVCX_HIP(hipMemcpyAsync(dg, gm.data(), gm.size() * sizeof(float), hipMemcpyHostToDevice, s));
    launch_fx_scale(V, dg, Bg, 2, ld, s);
    launch_fx_truepeak(V, dlen_v, Bg, 2, ld, p, dpk, s);
    T.mark(5);
    RVCX_HIP(hipMemcpyAsync(pk.data(), dpk, (size_t)Bg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));      // the skip decision needs the peaks
    bool over = false;
    for (int b = 0; b < Bg; ++b) over = over || bits_float(pk[b]) > c;
    if (over) {       // an item under the ceiling has r = 1 everywhere, hence s = 1 exactly: its samples pass bit for bit
      ctx->fx_passes[0] = launch_fx_limit_gain(p, dilen, len.data() + 2 * R, Bg, ld, c, W, c_rel, u, e, state, sg, dpk + Bg, s);
      RVCX_HIP(hipMemcpyAsync(low.data(), dpk + Bg, (size_t)Bg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    T.mark(6);
    launch_fx_limit_apply(V, over ? sg : nullptr, dlen_v, Bg, 2, ld, V, nullptr, pcm, s);
    T.mark(7);
    launch_fx_loudness(kw, V, dlen_v, Bg, 2, ld, sr, scratch, dl, nullptr, 0, s, nullptr);
    launch_fx_truepeak(V, dlen_v, Bg, 2, ld, nullptr, dpk, s);
    T.mark(8);
    RVCX_HIP(hipMemcpyAsync(Lr.data(), dl, Lr.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipMemcpyAsync(pk.data() + Bg, dpk, (size_t)Bg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    for (int b = 0; b < Bg; ++b) {
      pcm_host[g0 + b].resize((size_t)len[2 * b] * 2);
      RVCX_HIP(hipMemcpyAsync(pcm_host[g0 + b].data(), pcm + (size_t)b * ld * 2, (size_t)len[2 * b] * 4, hipMemcpyDeviceToHost, s));
    }
    T.mark(9);
    RVCX_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < Bg; ++b) {
      double* r = rep.data() + (size_t)(g0 + b) * 7;
      r[0] = L[b], r[1] = L[Bg + b], r[2] = Lm[b], r[3] = Lr[b], r[4] = fx_db20(bits_float(pk[b])), r[5] = fx_db20(bits_float(pk[Bg + b]));
      r[6] = (double)bits_float(low[b]);
    }
    // {stems, mix, mix loudness, scale + true peak, limiter gain, gain + int16, result meters, copies at either end, total}
    T.add_each(0, 1, 7), T.add(7, 0, 1), T.add(7, 8, 9), T.add(8, 0, 9);
  }
  A.reset();
  for (int b = 0; b < B; ++b) RVCX_HIP(hipMemcpy(out[b], pcm_host[b].data(), pcm_host[b].size() * 2, hipMemcpyDefault));
  if (report7) std::copy(rep.begin(), rep.end(), report7);
  T.store(*C);
  ctx->fx_groups = groups;
  API_END
}

// ---- host only ---------------------------------------------------------------------------------------------------------------
int rvcx_fx_kweight_coeffs(int sr, double* coef10) {
  return host_call([&] {
    if (!coef10) fail("fx_kweight_coeffs: null pointer");
    check_rate("fx_kweight_coeffs", sr);
    const FxKWeight k = fx_kweight(sr);
    const double v[10] = {k.sb0, k.sb1, k.sb2, k.sa1, k.sa2, k.hb0, k.hb1, k.hb2, k.ha1, k.ha2};
    std::copy(v, v + 10, coef10);
  });
}

int rvcx_fx_truepeak_taps(float* taps72) {
  return host_call([&] {
    if (!taps72) fail("fx_truepeak_taps: null pointer");
    const FxTpTaps& t = fx_tp_taps();
    std::copy(&t.h[0][0], &t.h[0][0] + 3 * kTpTaps, taps72);
  });
}

int rvcx_fx_loudness_host(const float* x, int64_t n, int channels, int sr, double* lufs, float* momentary) {
  return host_call([&] {
    loud_check("fx_loudness_host", sr, channels);
    if (!x || !lufs) fail("fx_loudness_host: null pointer");
    if (n < 0) fail("fx_loudness_host: n < 0");
    *lufs = fx_loudness_host(fx_kweight(sr), x, (long)n, channels, sr, momentary);
  });
}

int rvcx_fx_truepeak_host(const float* x, int64_t n, int channels, float* p, double* tp_db) {
  return host_call([&] {
    loud_check("fx_truepeak_host", 48000, channels);
    if (!x || !tp_db) fail("fx_truepeak_host: null pointer");
    if (n < 0) fail("fx_truepeak_host: n < 0");
    *tp_db = fx_db20(fx_truepeak_host(x, (long)n, channels, p));
  });
}

int rvcx_fx_limit_host(const float* x, int64_t n, int channels, int sr, float ceiling_db, float lookahead_ms, float release_ms,
                       float* y, float* gain) {
  return host_call([&] {
    loud_check("fx_limit_host", sr, channels);
    limit_check("fx_limit_host", ceiling_db, lookahead_ms, release_ms);
    if (!x || !y) fail("fx_limit_host: null pointer");
    if (n < 0) fail("fx_limit_host: n < 0");
    fx_limit_host(x, (long)n, channels, sr, ceiling_db, lookahead_ms, release_ms, y, gain, nullptr, nullptr);
  });
}

int rvcx_fx_master_host(const float* vocal, int64_t n_v, const float* inst, int64_t n_i, int sr, double target_lufs,
                        double vocal_offset_lu, double ceiling_dbtp, int16_t* out, double* report7) {
  return host_call([&] {
    master_check("fx_master_host", sr, target_lufs, vocal_offset_lu, ceiling_dbtp);
    if (n_v < 0 || n_i < 0) fail("fx_master_host: negative frame count");
    if ((n_v && (!vocal || !out)) || (n_i && !inst)) fail("fx_master_host: null pointer");
    fx_master_host(vocal, (long)n_v, inst, (long)n_i, sr, target_lufs, vocal_offset_lu, ceiling_dbtp, out, report7);
  });
}

}  // extern "C"
