// C ABI of librvcx.so (include/rvcx.h): the per-stage entry points the Python mirror calls.
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

extern "C" {

static int synth_infer_impl(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                            const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                            const float* src_noise, uint64_t seed, float* out, float* stats, float* zflow, int dec_skip,
                            int skip_head = 0);

int rvcx_synth_infer(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                     const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                     const float* src_noise, uint64_t seed, float* out) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return synth_infer_impl(ctx, model_id, B, T, lens, phone, pitch, pitchf, sid, z_noise, src_noise, seed, out, nullptr,
                          nullptr, 0);
}

int rvcx_synth_infer_window(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                            const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                            const float* src_noise, uint64_t seed, int dec_skip, float* out) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return synth_infer_impl(ctx, model_id, B, T, lens, phone, pitch, pitchf, sid, z_noise, src_noise, seed, out, nullptr,
                          nullptr, dec_skip < 0 ? 0 : dec_skip);
}

int rvcx_synth_dec_rf(rvcx_ctx* ctx, int model_id) {
  int rf = -1;
  const int rc = api_call(ctx, false, [&](Ctx* C) { rf = get_synth(*C, model_id).dec_rf_frames; });
  return rc ? -1 : rf;
}

int rvcx_synth_infer_taps(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                          const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                          const float* src_noise, uint64_t seed, float* out, float* stats, float* zflow) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return synth_infer_impl(ctx, model_id, B, T, lens, phone, pitch, pitchf, sid, z_noise, src_noise, seed, out, stats,
                          zflow, 0);
}

int rvcx_synth_infer_head(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                          const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                          const float* src_noise, uint64_t seed, int skip_head, float* out, float* zflow) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return synth_infer_impl(ctx, model_id, B, T, lens, phone, pitch, pitchf, sid, z_noise, src_noise, seed, out, nullptr,
                          zflow, 0, skip_head);
}

static int synth_infer_impl(rvcx_ctx* ctx, int model_id, int B, int T, const int32_t* lens, const float* phone,
                            const int32_t* pitch, const float* pitchf, const int32_t* sid, const float* z_noise,
                            const float* src_noise, uint64_t seed, float* out, float* stats, float* zflow, int dec_skip,
                            int skip_head) {
  API_BEGIN(ctx)
  SynthModel& M = get_synth(*C, model_id);
  const int D = M.cfg.input_dim, inter = M.cfg.inter_channels;
  if (skip_head < 0 || skip_head >= T) fail("synth_infer: skip_head outside [0, T)");
  if (skip_head > 0 && lens)
    for (int b = 0; b < B; ++b)
      if (lens[b] != T) fail("synth_infer: skip_head needs equal lengths (every item T frames)");
  const int Tk = T - skip_head;                     // frames the source, the flow and the decoder see
  const size_t Tupp = (size_t)Tk * M.upp;
  C->ensure_splitk(B);
  C->arena.reserve(synth_arena_bytes(M, B, T) + (size_t)B * T * D * 8 + (size_t)B * Tupp * 8 +
                   (size_t)B * 3 * inter * T * 4 + 4096);
  C->arena.reset();
  float* ph = to_dev(*C, phone, (size_t)B * T * D);
  float* ph_ct = C->arena.alloc<float>((size_t)B * T * D);
  launch_transpose(ph, ph_ct, B, T, D, C->stream);
  SynthIO io;
  io.B = B;
  io.T = T;
  io.lens_host = lens;
  io.phone_ct = ph_ct;
  io.pitch = to_dev<int>(*C, pitch, (size_t)B * T);
  io.pitchf = to_dev(*C, pitchf, (size_t)B * T);
  io.sid_host = sid;
  float* zn = C->arena.alloc<float>((size_t)B * inter * T);
  float* sn = C->arena.alloc<float>((size_t)B * Tupp);
  fill_noise(zn, z_noise, (size_t)B * inter * T, seed, 0, C->stream);
  fill_noise(sn, src_noise, (size_t)B * Tupp, seed, (uint64_t)1 << 40, C->stream);
  io.z_noise = zn;
  io.src_noise = sn;
  float* dout = C->arena.alloc<float>((size_t)B * Tupp);
  io.out = dout;
  if (stats) io.stats_out = C->arena.alloc<float>((size_t)B * 2 * inter * T);
  if (zflow) io.z_out = C->arena.alloc<float>((size_t)B * inter * T);
  io.dec_skip = dec_skip;
  io.skip_head = skip_head;
  synth_forward(*C, M, io, nullptr);
  if (stats) RVCX_HIP(hipMemcpyAsync(stats, io.stats_out, (size_t)B * 2 * inter * T * 4, hipMemcpyDefault, C->stream));
  if (zflow) RVCX_HIP(hipMemcpyAsync(zflow, io.z_out, (size_t)B * inter * Tk * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipMemcpyAsync(out, dout, (size_t)B * Tupp * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->arena.reset();
  API_END
}

int64_t rvcx_crepe_frames(int64_t n, int hop) { return hop > 0 ? 1 + n / hop : -1; }

int rvcx_crepe_predict(rvcx_ctx* ctx, const float* x, int64_t n, int hop, float fmin, float fmax, const float* dither,
                       uint64_t seed, float* pitch, float* probs, int32_t* bins) {
  API_BEGIN(ctx)
  if (!C->crepe) fail("crepe not loaded");
  if (!x || !pitch || n <= 0 || hop <= 0) fail("crepe_predict: bad argument");
  const long F = crepe_frames(n, hop);
  C->arena.reserve(crepe_arena_bytes(*C->crepe, n, hop) + (size_t)n * 8 + (size_t)F * (360 + 16) * 4 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dx = to_dev(*C, x, (size_t)n);
  std::vector<float> h((size_t)n);
  RVCX_HIP(hipMemcpyAsync(h.data(), dx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  RVCX_HIP(hipStreamSynchronize(s));
  const float scale = (float)crepe_quantile999(h);
  if (!(scale > 0.f)) fail("crepe: the signal is silent (its 99.9 % quantile is 0)");
  float* dd = C->arena.alloc<float>((size_t)F);
  if (dither) RVCX_HIP(hipMemcpyAsync(dd, dither, (size_t)F * 4, hipMemcpyDefault, s));
  else launch_crepe_dither(dd, F, seed + 0x63726570ull, 0, s);
  float* dp = C->arena.alloc<float>((size_t)F);
  float* dpr = probs ? C->arena.alloc<float>((size_t)F * 360) : nullptr;
  int* db = bins ? C->arena.alloc<int>((size_t)F) : nullptr;
  crepe_forward(*C, *C->crepe, dx, n, scale, hop, fmin, fmax, dd, dp, dpr, db, s);
  RVCX_HIP(hipMemcpyAsync(pitch, dp, (size_t)F * 4, hipMemcpyDefault, s));
  if (probs) RVCX_HIP(hipMemcpyAsync(probs, dpr, (size_t)F * 360 * 4, hipMemcpyDefault, s));
  if (bins) RVCX_HIP(hipMemcpyAsync(bins, db, (size_t)F * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->check_dev_err();
  C->arena.reset();
  API_END
}

int rvcx_fcpe_f0(rvcx_ctx* ctx, int B, const float* audio, int64_t n, float threshold, float* f0, float* salience,
                 float* mel) {
  API_BEGIN(ctx)
  if (!C->fcpe) fail("fcpe not loaded");
  C->ensure_splitk(B);
  const int F = (int)(1 + n / 160), nb = C->fcpe->cfg.out_dims;
  C->arena.reserve(fcpe_arena_bytes(*C->fcpe, B, n) + (size_t)B * (n + (size_t)F * (nb + 130)) * 4);
  C->arena.reset();
  float* da = to_dev(*C, audio, (size_t)B * n);
  float* df0 = C->arena.alloc<float>((size_t)B * F);
  float* ds = salience ? C->arena.alloc<float>((size_t)B * F * nb) : nullptr;
  float* dm = mel ? C->arena.alloc<float>((size_t)B * 128 * F) : nullptr;
  fcpe_forward(*C, *C->fcpe, B, da, n, threshold, df0, ds, dm, C->stream);
  RVCX_HIP(hipMemcpyAsync(f0, df0, (size_t)B * F * 4, hipMemcpyDefault, C->stream));
  if (salience) RVCX_HIP(hipMemcpyAsync(salience, ds, (size_t)B * F * nb * 4, hipMemcpyDefault, C->stream));
  if (mel) RVCX_HIP(hipMemcpyAsync(mel, dm, (size_t)B * 128 * F * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->check_dev_err();
  C->arena.reset();
  API_END
}

int rvcx_rmvpe_f0(rvcx_ctx* ctx, int B, const float* audio, int64_t n, float thred, float f0_min, float f0_max,
                  float* f0, float* hidden) {
  API_BEGIN(ctx)
  if (!C->rmvpe) fail("rmvpe not loaded");
  C->ensure_splitk(B);
  const int F = (int)(1 + n / 160);
  C->arena.reserve(rmvpe_arena_bytes(*C->rmvpe, B, n) + (size_t)B * (n + (size_t)F * 362) * 4);
  C->arena.reset();
  float* da = to_dev(*C, audio, (size_t)B * n);
  float* df0 = C->arena.alloc<float>((size_t)B * F);
  float* dh = hidden ? C->arena.alloc<float>((size_t)B * F * 360) : nullptr;
  rmvpe_forward(*C, *C->rmvpe, B, da, n, thred, f0_min, f0_max, df0, dh, C->stream);
  RVCX_HIP(hipMemcpyAsync(f0, df0, (size_t)B * F * 4, hipMemcpyDefault, C->stream));
  if (hidden) RVCX_HIP(hipMemcpyAsync(hidden, dh, (size_t)B * F * 360 * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->check_dev_err();
  C->arena.reset();
  API_END
}

int rvcx_rmvpe_mel(rvcx_ctx* ctx, int B, const float* audio, int64_t n, float* mel) {
  API_BEGIN(ctx)
  if (!C->rmvpe) fail("rmvpe not loaded");
  C->ensure_splitk(B);
  const int F = (int)(1 + n / 160);
  C->arena.reserve(rmvpe_arena_bytes(*C->rmvpe, B, n) + (size_t)B * (n + (size_t)F * 130) * 4);
  C->arena.reset();
  float* da = to_dev(*C, audio, (size_t)B * n);
  float* df0 = C->arena.alloc<float>((size_t)B * F);
  float* dm = C->arena.alloc<float>((size_t)B * 128 * F);
  rmvpe_forward(*C, *C->rmvpe, B, da, n, 0.03f, 50.f, 1100.f, df0, nullptr, C->stream, dm);
  RVCX_HIP(hipMemcpyAsync(mel, dm, (size_t)B * 128 * F * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->check_dev_err();
  C->arena.reset();
  API_END
}

int rvcx_hubert_frames(rvcx_ctx* ctx, int64_t n) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ctx->c.hubert) return -1;
  return hubert_frames(*ctx->c.hubert, n);
}

int rvcx_hubert_features(rvcx_ctx* ctx, int B, const float* wav, int64_t n, int output_layer, float* feats) {
  API_BEGIN(ctx)
  if (!C->hubert) fail("hubert not loaded");
  const int T = hubert_frames(*C->hubert, n), E = C->hubert->cfg.embed_dim;
  if (T <= 0) fail("hubert: input too short");
  C->ensure_splitk(B);
  C->arena.reserve(hubert_arena_bytes(*C->hubert, B, n) + (size_t)B * (n + (size_t)2 * T * E) * 4);
  C->arena.reset();
  float* dw = to_dev(*C, wav, (size_t)B * n);
  float* fct = C->arena.alloc<float>((size_t)B * E * T);
  float* ftc = C->arena.alloc<float>((size_t)B * E * T);
  hipStream_t st = C->stream;
  hubert_forward(*C, *C->hubert, B, dw, n, output_layer, fct, st);
  launch_transpose(fct, ftc, B, E, T, st);   // (B,E,T) -> (B,T,E)
  RVCX_HIP(hipMemcpyAsync(feats, ftc, (size_t)B * E * T * 4, hipMemcpyDefault, st));
  RVCX_HIP(hipStreamSynchronize(st));
  C->arena.reset();
  API_END
}

int rvcx_index_blend(rvcx_ctx* ctx, float* feats, int T, float index_rate, int64_t* ids, float* dist) {
  API_BEGIN(ctx)
  if (!C->index) fail("index not loaded");
  const int D = C->index->dim;
  C->arena.reserve(index_arena_bytes(*C->index, T) + (size_t)T * (2 * D + 24) * 4 + (64 << 20));
  C->arena.reset();
  float* f = to_dev(*C, feats, (size_t)T * D);
  float* fct = C->arena.alloc<float>((size_t)T * D);
  launch_transpose(f, fct, 1, T, D, C->stream);
  int64_t* dids = C->arena.alloc<int64_t>((size_t)T * 8);
  float* ddist = C->arena.alloc<float>((size_t)T * 8);
  index_blend(*C, *C->index, fct, T, index_rate, dids, ddist, C->stream);
  launch_transpose(fct, f, 1, D, T, C->stream);
  RVCX_HIP(hipMemcpyAsync(feats, f, (size_t)T * D * 4, hipMemcpyDefault, C->stream));
  if (ids) RVCX_HIP(hipMemcpyAsync(ids, dids, (size_t)T * 8 * 8, hipMemcpyDefault, C->stream));
  if (dist) RVCX_HIP(hipMemcpyAsync(dist, ddist, (size_t)T * 8 * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->arena.reset();
  API_END
}

// the tail of every rvcx_get_f0*: both tracks to the caller, then the call's device errors
static void f0_to_host(Ctx& c, int32_t* coarse, const int* dc, float* f0, const float* df, long frames) {
  RVCX_HIP(hipMemcpyAsync(coarse, dc, (size_t)frames * 4, hipMemcpyDefault, c.stream));
  RVCX_HIP(hipMemcpyAsync(f0, df, (size_t)frames * 4, hipMemcpyDefault, c.stream));
  RVCX_HIP(hipStreamSynchronize(c.stream));
  c.check_dev_err();
  c.arena.reset();
}

int rvcx_get_f0(rvcx_ctx* ctx, const float* wav16k, int64_t n, const rvcx_params* p, int32_t* coarse, float* f0,
                int64_t* p_len) {
  API_BEGIN(ctx)
  const long t_pad = 16000L * p->x_pad, n_pad = n + 2 * t_pad;
  C->arena.reserve(f0_arena_bytes(*C, *p, 1, n_pad) + (size_t)n_pad * 48 + (64 << 20));
  C->arena.reset();
  float* dw = to_dev(*C, wav16k, (size_t)n);
  double* ext = C->arena.alloc<double>(highpass_ext_doubles(n));
  float* a32 = C->arena.alloc<float>((size_t)n);
  launch_highpass(dw, nullptr, ext, nullptr, a32, n, C->stream);
  float* apad = C->arena.alloc<float>((size_t)n_pad);
  launch_reflect_pad(a32, apad, 1, (int)n, (int)t_pad, n_pad, C->stream);
  const long pl = n_pad / 160;
  int* dc = C->arena.alloc<int>((size_t)pl + 8);
  float* df = C->arena.alloc<float>((size_t)pl + 8);
  get_f0_device(*C, apad, 1, n_pad, *p, dc, df, 0, C->stream);
  f0_to_host(*C, coarse, dc, f0, df, pl);
  *p_len = pl;
  API_END
}

// VC.get_f0 on one padded + filtered signal, behind every rvcx_get_f0*_x.  method: the back-end, -1 = params.f0_method.
// Frames: rmvpe is un-truncated (1 + n / 160); fcpe resizes to p_len and mangio-crepe computes p_len
static int get_f0_x(rvcx_ctx* ctx, const float* x, int64_t n, int64_t p_len, const rvcx_params* p, int method,
                    const float* inp_f0, int inp_f0_rows, const F0Extra* extra, int32_t* coarse, float* f0, int64_t* frames) {
  API_BEGIN(ctx)
  if (!p || !x || !coarse || !f0) fail("get_f0: null argument");
  if (n <= 0) fail("get_f0: empty signal");
  rvcx_params q = *p;
  if (method >= 0) q.f0_method = method;
  check_f0_backend(*C, q);
  if (q.f0_method == RVCX_F0_CREPE && !extra) fail("get_f0: mangio-crepe takes its dither through rvcx_get_f0_crepe_x");
  const long F = q.f0_method == RVCX_F0_RMVPE ? 1 + n / 160 : (long)p_len;
  if (F <= 0) fail("get_f0: p_len must be positive");
  const std::vector<double> track = f0_file_track(inp_f0, inp_f0 ? inp_f0_rows : 0);
  C->arena.reserve(f0_arena_bytes(*C, q, 1, n) + (size_t)n * 8 + (size_t)(F + n / 160 + 8) * 48 + track.size() * 8 +
                   (64 << 20));
  C->arena.reset();
  float* dx = to_dev(*C, x, (size_t)n);
  int* dc = C->arena.alloc<int>((size_t)F);
  float* df = C->arena.alloc<float>((size_t)F);
  F0Opts o;
  o.frames = F;
  o.track = &track;
  o.extra = extra;
  get_f0_device(*C, dx, 1, n, q, dc, df, F, C->stream, o);
  f0_to_host(*C, coarse, dc, f0, df, F);
  if (frames) *frames = F;
  API_END
}

int rvcx_get_f0_x(rvcx_ctx* ctx, const float* x, int64_t n, const rvcx_params* p, int32_t* coarse, float* f0) {
  return get_f0_x(ctx, x, n, 0, p, RVCX_F0_RMVPE, nullptr, 0, nullptr, coarse, f0, nullptr);
}

int rvcx_get_f0_x_ex(rvcx_ctx* ctx, const float* x, int64_t n, int64_t p_len, const rvcx_params* p, const float* inp_f0,
                     int inp_f0_rows, int32_t* coarse, float* f0, int64_t* frames) {
  return get_f0_x(ctx, x, n, p_len, p, -1, inp_f0, inp_f0_rows, nullptr, coarse, f0, frames);
}

int rvcx_get_f0_fcpe_x(rvcx_ctx* ctx, const float* x, int64_t n, int64_t p_len, const rvcx_params* p, int32_t* coarse,
                       float* f0) {
  return get_f0_x(ctx, x, n, p_len, p, RVCX_F0_FCPE, nullptr, 0, nullptr, coarse, f0, nullptr);
}

int rvcx_get_f0_crepe_x(rvcx_ctx* ctx, const float* x, int64_t n, int64_t p_len, const rvcx_params* p, const float* inp_f0,
                        int inp_f0_rows, const float* dither, int64_t dither_n, int32_t* coarse, float* f0) {
  F0Extra ex;
  ex.dither = dither;
  ex.dither_n = dither ? dither_n : 0;
  return get_f0_x(ctx, x, n, p_len, p, RVCX_F0_CREPE, inp_f0, inp_f0_rows, &ex, coarse, f0, nullptr);
}

int rvcx_f0_file_track(const float* inp_f0, int rows, double* track, int cap) {
  try {
    const std::vector<double> t = f0_file_track(inp_f0, rows);
    for (size_t i = 0; i < t.size() && (int)i < cap; ++i) track[i] = t[i];
    return (int)t.size();
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

int64_t rvcx_resample_len(int64_t n, int sr_in, int sr_out) {
  return (sr_in > 0 && sr_out > 0 && n >= 0) ? (int64_t)resample_out_len((long)n, sr_in, sr_out) : -1;
}

int rvcx_resample_f64_kind(rvcx_ctx* ctx, const double* x, int64_t frames, int channels, int sr_in, int sr_out, int kind,
                           double* y) {
  // load_audio's resampler is what a "convert this folder" loop calls BETWEEN two submits (the next file is decoded while
  // two tickets are in flight), so it does not complete the tickets: with tickets in flight it works in a buffer of its own
  // (nothing a ticket uses is touched or moved) on the front stream, whose work for the tickets in flight ended long ago,
  // so that it runs beside their synthesizer instead of behind it.  Same kernels, same bits as on an idle context.
  return api_call(ctx, true, [&](Ctx* C) {
    if (!x || !y || frames <= 0 || channels < 1 || sr_in <= 0 || sr_out <= 0) fail("resample: bad argument");
    const bool beside = !ctx->inflight.empty();
    Arena& A = beside ? ctx->load_arena : C->arena;
    hipStream_t s = (beside && !C->serial) ? C->stream2 : C->stream;
    const long n_out = resample_out_len((long)frames, sr_in, sr_out);
    A.reset();
    A.reserve(((size_t)frames * channels + (size_t)n_out) * 8 + ((size_t)8 << 20));
    double* dx = A.alloc<double>((size_t)frames * channels);
    RVCX_HIP(hipMemcpyAsync(dx, x, (size_t)frames * channels * sizeof(double), hipMemcpyDefault, s));
    double* dy = A.alloc<double>((size_t)std::max<long>(n_out, 1));
    const ResampleFilter f = make_resample_filter(A, sr_in, sr_out, s, kind);
    launch_resample_f64(f, dx, (long)frames, channels, dy, n_out, s);
    RVCX_HIP(hipMemcpyAsync(y, dy, (size_t)n_out * 8, hipMemcpyDefault, s));
    RVCX_HIP(hipStreamSynchronize(s));
    A.reset();
  }, /*drain=*/false);
}

int rvcx_resample_f64(rvcx_ctx* ctx, const double* x, int64_t frames, int channels, int sr_in, int sr_out, double* y) {
  return rvcx_resample_f64_kind(ctx, x, frames, channels, sr_in, sr_out, -1, y);
}

int rvcx_vc_frames(rvcx_ctx* ctx, int64_t n) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ctx->c.hubert) return -1;
  const int Th = hubert_frames(*ctx->c.hubert, n);
  if (Th <= 0) return -1;
  return (int)std::min<long>(n / 160, 2L * Th);
}

int rvcx_vc(rvcx_ctx* ctx, int model_id, const float* audio0, int64_t n, const int32_t* pitch, const float* pitchf,
            int n_pitch, int sid, float index_rate, float protect, const float* z_noise, const float* src_noise,
            uint64_t seed, float* out, int64_t* out_n) {
  API_BEGIN(ctx)
  SynthModel& M = get_synth(*C, model_id);
  if (!C->hubert) fail("hubert not loaded");
  if (!pitch || !pitchf) fail("vc: non-f0 models cannot run in the reference either (generators.py:57-77)");
  const int E = M.cfg.input_dim, inter = M.cfg.inter_channels;      // v2: the HuBERT's embed_dim; v1: its final_proj width
  RVCX_CHECK(E == C->hubert->cfg.embed_dim || (C->hubert->has_final_proj && E == C->hubert->final_proj.cout),
             "the voice model's input_dim is neither the HuBERT's embed_dim (v2) nor its final_proj width (v1)");
  const int Th = hubert_frames(*C->hubert, n);
  RVCX_CHECK(Th > 0, "vc: chunk too short");
  const int T = (int)std::min<long>(n / 160, 2L * Th);       // p_len clamp, pipeline.py:257-262
  RVCX_CHECK(n_pitch >= T, "vc: pitch / pitchf shorter than the chunk's frame count");
  const size_t nz = (size_t)inter * T, nsrc = (size_t)T * M.upp;
  size_t need = hubert_arena_bytes(*C->hubert, 1, n) + synth_arena_bytes(M, 1, T) + (size_t)n * 4 +
                ((size_t)T * ((size_t)3 * E + inter + 3 * M.upp + 16)) * 4;
  if (C->index && index_rate != 0.f) need += index_arena_bytes(*C->index, Th);
  C->arena.reserve(need);
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dw = to_dev(*C, audio0, (size_t)n);
  int* dp = to_dev<int>(*C, pitch, (size_t)T);
  float* dpf = to_dev(*C, pitchf, (size_t)T);
  float* phone = C->arena.alloc<float>((size_t)E * T);
  vc_front(*C, E, 1, dw, n, Th, T, dpf, index_rate, protect, phone, s);
  float* zn = C->arena.alloc<float>(nz);
  float* sn = C->arena.alloc<float>(nsrc);
  fill_noise(zn, z_noise, nz, seed, 0, s);
  fill_noise(sn, src_noise, nsrc, seed, (uint64_t)1 << 35, s);
  float* wavout = C->arena.alloc<float>(nsrc);
  SynthIO io;
  io.B = 1;
  io.T = T;
  io.phone_ct = phone;
  io.pitch = dp;
  io.pitchf = dpf;
  io.sid_host = &sid;
  io.z_noise = zn;
  io.src_noise = sn;
  io.out = wavout;
  synth_forward(*C, M, io, nullptr);
  RVCX_HIP(hipMemcpyAsync(out, wavout, nsrc * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  if (out_n) *out_n = (int64_t)nsrc;
  C->arena.reset();
  API_END
}

int rvcx_highpass_exact(const double* x, double* y, int64_t n) {
  try {
    if (!x || !y) fail("highpass_exact: null pointer");
    highpass_exact_host(x, n, y);
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

}  // extern "C"
