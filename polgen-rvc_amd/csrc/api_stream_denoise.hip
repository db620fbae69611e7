// C ABI of librvcx.so (include/rvcx.h "live noise reduction", stage 16): the causal spectral gate at either edge of a
// live-stream session's step (rvcx_stream_open_dn, _set_denoise, _last_dn_ms; the step itself is api_stream.hip's), the same
// gate without a session (rvcx_op_stream_denoise), its host twin and the delay rule.
#include "api_fx_common.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

struct LivePlan {
  DnLiveHostPlan h;
  FxStretchGeom g;
};

// every refusal that depends on the parameters alone; sr: the rate the side runs at (params->sample_rate may be 0 or sr)
LivePlan live_check(const char* who_c, const rvcx_live_denoise_params* p, int sr) {
  const std::string who(who_c);
  if (!p) fail(who + ": null parameters");
  if (p->sample_rate != 0 && p->sample_rate != sr) fail(who + ": sample_rate must be 0 or the rate of the signal, " + std::to_string(sr));
  check_rate(who_c, sr, true);
  if (p->channels != 0 && p->channels != 1) fail(who + ": channels must be 0 or 1 (live noise reduction is mono)");
  if (p->mode != 0 && p->mode != 1) fail(who + ": mode must be 0 (profile) or 1 (adaptive)");
  check_finite(who_c, {p->strength, p->n_std, p->knee_db, p->thresh_mult, p->slope, p->time_constant_s, p->fall_time_s,
                       p->freq_smooth_hz, p->time_smooth_ms});
  check_range(who_c, p->strength, 0.0, 1.0, "strength");
  check_range(who_c, p->n_std, 0.0, 10.0, "n_std");
  check_range(who_c, p->knee_db, (double)0.1f, 20.0, "knee_db");
  check_range(who_c, p->thresh_mult, 0.0, 20.0, "thresh_mult");
  check_range(who_c, p->slope, (double)0.1f, 100.0, "slope");
  check_range(who_c, p->time_constant_s, (double)0.05f, 30.0, "time_constant_s");
  check_range(who_c, p->fall_time_s, (double)0.01f, (double)p->time_constant_s, "fall_time_s (0.01 .. time_constant_s)");
  if (p->freq_smooth_hz < 0.f || p->time_smooth_ms < 0.f) fail(who + ": freq_smooth_hz and time_smooth_ms must not be negative");
  LivePlan P;
  P.g = dn_live_geom(sr);
  const double nf = dn_live_nf(p->freq_smooth_hz, P.g.N, sr), nt = dn_live_nt(p->time_smooth_ms, sr, P.g.H);
  if (nf > kDnLiveMaxNf) fail(who + ": freq_smooth_hz spans more than 64 bins to a side at this rate");
  if (nt > kDnLiveMaxNt) fail(who + ": time_smooth_ms spans more than 32 frames at this rate");
  P.h.sr = sr, P.h.nf = (int)nf, P.h.nt = (int)nt;
  P.h.v = DnLiveValues{p->mode,  p->strength, p->n_std, p->knee_db, p->thresh_mult, p->slope,
                       dn_live_c(P.g.H, sr, p->time_constant_s), dn_live_c(P.g.H, sr, p->fall_time_s)};
  return P;
}

void clip_check(const std::string& who, const LivePlan& P, const float* noise, int64_t n_noise) {
  if (P.h.v.mode == 1) {
    if (noise) fail(who + ": the adaptive mode takes no noise clip");
    return;
  }
  if (!noise) fail(who + ": mode 0 needs a noise clip");
  if (n_noise < P.g.N / 2 || n_noise > (int64_t)1 << 22)
    fail(who + ": a noise clip needs N / 2 = " + std::to_string(P.g.N / 2) + " .. 2^22 samples (one whole frame at least)");
}

// arena bytes of the profile's scratch
size_t profile_bytes(const LivePlan& P, long n_noise) {
  const size_t Tp = (size_t)dn_live_frames(n_noise, P.g.N, P.g.H);
  return ((size_t)2 * n_noise + (size_t)P.g.N + Tp * P.g.nb + 2 * ((size_t)2 * P.g.N + (size_t)(P.h.nt + 2) * P.g.nb + 8)) * 4 + 4096;
}

// mu and sd (device, nb doubles each) of a clip (host or device pointer): the step's own kernel on the clip as one block,
// analysis alone, then stage 15's statistics.  Scratch comes from the arena (above the caller's mark).
void profile_device(Ctx& c, const LivePlan& P, const float* w, const float2* tw, const float* noise, long n_noise, double* mu,
                    double* sd) {
  Arena& A = c.arena;
  const size_t mk = A.mark();
  DnLive d;
  d.S = 1, d.sr = P.h.sr, d.nf = P.h.nf, d.nt = P.h.nt, d.B = n_noise, d.g = P.g, d.v = P.h.v;
  d.v.mode = 2;
  d.w = w, d.tw = tw;
  dn_live_layout(d);
  const long Tp = dn_live_frames(n_noise, P.g.N, P.g.H);
  float* clip = A.alloc<float>((size_t)n_noise);
  RVCX_HIP(hipMemcpyAsync(clip, noise, (size_t)n_noise * 4, hipMemcpyDefault, c.stream));
  for (float*& q : d.state) {
    q = A.alloc<float>((size_t)d.per_stream);
    RVCX_HIP(hipMemsetAsync(q, 0, (size_t)d.per_stream * 4, c.stream));
  }
  d.acc = A.alloc<float>((size_t)P.g.N + n_noise);
  DnLiveTaps t;
  t.S = A.alloc<float>((size_t)Tp * P.g.nb), t.T = Tp;
  dn_live_step(d, clip, n_noise, 0, 0, nullptr, 0, c.stream, &t);
  launch_dn_live_stats(t.S, Tp, P.g.nb, mu, sd, c.stream);
  A.reset(mk);       // (stream order: whatever takes this memory next runs behind these launches)
}

}  // namespace

extern "C" {

int rvcx_stream_denoise_delay(int sr) { return dn_live_rate_ok(sr) ? dn_live_geom(sr).N : -1; }

int rvcx_stream_denoise_frames(int64_t n, int sr, float freq_smooth_hz, float time_smooth_ms, int64_t* T, int32_t* N, int32_t* nf,
                               int32_t* nt) {
  return host_call([&] {
    check_rate("stream_denoise_frames", sr, true);
    if (n < 0 || n > (int64_t)1 << 40) fail("stream_denoise_frames: n out of range");
    if (!(freq_smooth_hz >= 0.f) || !(time_smooth_ms >= 0.f) || !std::isfinite(freq_smooth_hz) || !std::isfinite(time_smooth_ms))
      fail("stream_denoise_frames: the widths must be finite and not negative");
    const FxStretchGeom g = dn_live_geom(sr);
    if (T) *T = dn_live_frames((long)n, g.N, g.H);
    if (N) *N = g.N;
    if (nf) *nf = (int32_t)std::min(1e6, dn_live_nf(freq_smooth_hz, g.N, sr));
    if (nt) *nt = (int32_t)std::min(1e6, dn_live_nt(time_smooth_ms, sr, g.H));
  });
}

int rvcx_stream_open_dn(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_stream_io* io, const rvcx_fx_params* fx,
                        const rvcx_stream_dn* dn, const rvcx_params* p, const int32_t* sid, const float* pitch, int* stream_id) {
  if (!dn || (!dn->in.params && !dn->out.params)) return rvcx_stream_open_fx(ctx, model_id, cfg, io, fx, p, sid, pitch, stream_id);
  CtxLock ctx_guard_ = lock_ctx(ctx);
  const rvcx_stream_dn_side* sides[2] = {&dn->in, &dn->out};
  // every refusal of both sides first: nothing is opened for parameters they would not run
  LivePlan P[2];
  int rc = api_call(ctx, false, [&](Ctx* C) {
    if (!cfg) fail("stream_open_dn: null argument");
    const SynthModel& M = get_synth(*C, model_id);
    const int rate[2] = {16000, io && io->out_rate != 0 ? io->out_rate : M.cfg.sr};
    for (int k = 0; k < 2; ++k) {
      if (!sides[k]->params) continue;
      const char* who = k == 0 ? "stream_open_dn (input side)" : "stream_open_dn (output side)";
      P[k] = live_check(who, sides[k]->params, rate[k]);
      clip_check(who, P[k], sides[k]->noise_hd, sides[k]->n_noise);
    }
  });
  if (rc != 0) return rc;
  int id = 0;
  rc = rvcx_stream_open_fx(ctx, model_id, cfg, io, fx, p, sid, pitch, &id);
  if (rc != 0) return rc;
  rc = api_call(ctx, false, [&](Ctx* C) {
    StreamSession& se = get_session(ctx, id);
    hipStream_t s = C->stream;
    for (int k = 0; k < 2; ++k) {
      if (!sides[k]->params) continue;
      StreamSession::DnSide& sd = se.dn[k];
      auto d = std::make_unique<DnLive>();
      d->S = se.S, d->sr = P[k].h.sr, d->nf = P[k].h.nf, d->nt = P[k].h.nt, d->g = P[k].g, d->v = P[k].h.v;
      d->B = k == 0 ? (long)se.cfg.block_frames * 160 : (se.out.on ? se.out.g.B_out : se.Lb);
      RVCX_CHECK(d->B * 100 == (long)se.cfg.block_frames * d->sr, "stream_open_dn: the block is not block_frames x 10 ms at the side's rate");
      dn_live_layout(*d);
      sd.d = std::move(d);                    // from here on the session's destructor frees what was allocated
      DnLive& L = *sd.d;
      const int N = L.g.N, nb = L.g.nb;
      const size_t sb = (size_t)se.S * L.per_stream * 4;
      for (float*& q : L.state) {
        RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&q), sb));
        RVCX_HIP(hipMemsetAsync(q, 0, sb, s));
      }
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&L.acc), (size_t)se.S * (N + L.B) * 4));
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&sd.stage), (size_t)se.S * L.B * 4));
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&sd.tables), (size_t)2 * N * 4));
      const StftTables tables(N);             // (into the session's own memory, not the arena)
      RVCX_HIP(hipMemcpyAsync(sd.tables, tables.w.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
      RVCX_HIP(hipMemcpyAsync(sd.tables + N, tables.tw.data(), (size_t)N / 2 * 8, hipMemcpyHostToDevice, s));
      RVCX_HIP(hipStreamSynchronize(s));      // (the tables are this scope's)
      L.w = sd.tables, L.tw = reinterpret_cast<const float2*>(sd.tables + N);
      if (L.v.mode == 0) {
        RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&sd.prof), (size_t)2 * nb * sizeof(double)));
        C->arena.reserve(profile_bytes(P[k], (long)sides[k]->n_noise) + (1 << 20));
        C->arena.reset();
        profile_device(*C, P[k], L.w, L.tw, sides[k]->noise_hd, (long)sides[k]->n_noise, sd.prof, sd.prof + nb);
        RVCX_HIP(hipStreamSynchronize(s));
        C->arena.reset();
        L.mu = sd.prof, L.sd = sd.prof + nb;
      }
      for (hipEvent_t& e : sd.ev) RVCX_HIP(hipEventCreate(&e));
      sd.p = *sides[k]->params;
    }
    RVCX_HIP(hipStreamSynchronize(s));
  });
  if (rc != 0) {
    const std::string why = ctx->c.last_error;
    (void)rvcx_stream_close(ctx, id);
    g_last_error = ctx->c.last_error = why;
    return -1;
  }
  if (stream_id) *stream_id = id;
  return 0;
}

int rvcx_stream_set_denoise(rvcx_ctx* ctx, int stream_id, int side, const rvcx_live_denoise_params* params) {
  API_BEGIN(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  if (side != 0 && side != 1) fail("stream_set_denoise: side must be 0 (input) or 1 (output)");
  StreamSession::DnSide& sd = se.dn[side];
  if (!sd.d) fail("stream_set_denoise: the session was opened without noise reduction on this side (its delay is fixed at open)");
  const LivePlan P = live_check("stream_set_denoise", params, sd.d->sr);
  if (P.h.nt != sd.d->nt)
    fail("stream_set_denoise: time_smooth_ms would change the frames of history from " + std::to_string(sd.d->nt) + " to " +
         std::to_string(P.h.nt) + " (the state's layout is fixed at open)");
  if (P.h.v.mode == 0 && !sd.prof) fail("stream_set_denoise: mode 0 needs the noise clip the side was opened without");
  // every check has passed: nothing below can fail, all state is kept
  sd.d->nf = P.h.nf, sd.d->v = P.h.v;
  sd.d->mu = sd.prof, sd.d->sd = sd.prof ? sd.prof + sd.d->g.nb : nullptr;
  sd.p = *params;
  API_END
}

int rvcx_stream_last_dn_ms(rvcx_ctx* ctx, int stream_id, float* ms2) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ms2) return -1;
  auto it = ctx->sessions.find(stream_id);
  if (it == ctx->sessions.end()) return -1;
  for (int k = 0; k < 2; ++k) ms2[k] = it->second->dn[k].d ? it->second->dn_ms[k] : 0.f;
  return 0;
}

int rvcx_fx_denoise_live_host(const float* x, int64_t n, int sr, const float* noise, int64_t n_noise,
                              const rvcx_live_denoise_params* params, float* y, float* D, float* S, double* f, float* m) {
  return host_call([&] {
    const LivePlan P = live_check("fx_denoise_live_host", params, sr);
    if (!x || !y) fail("fx_denoise_live_host: null pointer");
    check_frames("fx_denoise_live_host", n, "1 .. 2^30 samples are required");
    clip_check("fx_denoise_live_host", P, noise, n_noise);
    if (f && P.h.v.mode != 1) fail("fx_denoise_live_host: f exists in mode 1 only");
    std::vector<double> mu, sd;
    if (P.h.v.mode == 0) {
      mu.resize((size_t)P.g.nb), sd.resize((size_t)P.g.nb);
      dn_live_profile_host(noise, (long)n_noise, P.h, mu.data(), sd.data());
    }
    dn_live_host(x, (long)n, P.h, mu.data(), sd.data(), y, D, S, f, m);
  });
}

int rvcx_op_stream_denoise(rvcx_ctx* ctx, const float* x, int S, int64_t frames, int sr, int block_frames,
                           const rvcx_live_denoise_params* params, const float* noise, int64_t n_noise, float* y, float* S_tap,
                           double* f_tap, float* m_tap) {
  API_BEGIN(ctx)
  const LivePlan P = live_check("op_stream_denoise", params, sr);
  if (!x || !y) fail("op_stream_denoise: null argument");
  if (S < 1 || S > 4096 || frames < 1 || block_frames < 1) fail("op_stream_denoise: S in 1 .. 4096, frames and block_frames >= 1");
  clip_check("op_stream_denoise", P, noise, n_noise);
  if (f_tap && P.h.v.mode != 1) fail("op_stream_denoise: f exists in mode 1 only");
  DnLive d;
  d.S = S, d.sr = sr, d.nf = P.h.nf, d.nt = P.h.nt, d.g = P.g, d.v = P.h.v;
  d.B = (long)block_frames * sr / 100;
  if (frames % d.B != 0)
    fail("op_stream_denoise: frames must be a multiple of the block, block_frames * sr / 100 = " + std::to_string(d.B));
  dn_live_layout(d);
  const long K = (long)(frames / d.B), T = dn_live_frames((long)frames, P.g.N, P.g.H);
  const size_t nx = (size_t)S * frames, ns = (size_t)S * d.per_stream, nbins = (size_t)S * std::max(T, 1L) * P.g.nb;
  if (nx > ((size_t)1 << 31)) fail("op_stream_denoise: more than 2^31 samples");
  const bool taps = S_tap || f_tap || m_tap;
  C->arena.reserve((2 * nx + 2 * ns + (size_t)S * (P.g.N + d.B) + (size_t)2 * P.g.N + (size_t)4 * P.g.nb) * 4 +
                   (taps ? nbins * 16 : 0) + (noise ? profile_bytes(P, (long)n_noise) : 0) + (1 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  Arena& A = C->arena;
  const StftTables tables(P.g.N);
  tables.upload(*C, d.w, d.tw);
  if (P.h.v.mode == 0) {
    double* mu = A.alloc<double>((size_t)P.g.nb);
    double* sd = A.alloc<double>((size_t)P.g.nb);
    profile_device(*C, P, d.w, d.tw, noise, (long)n_noise, mu, sd);
    d.mu = mu, d.sd = sd;
  }
  float* dx = to_dev(*C, x, nx);
  float* dy = A.alloc<float>(nx);
  for (float*& q : d.state) {
    q = A.alloc<float>(ns);
    RVCX_HIP(hipMemsetAsync(q, 0, ns * 4, s));
  }
  d.acc = A.alloc<float>((size_t)S * (P.g.N + d.B));
  DnLiveTaps t;
  if (taps && T > 0) {
    t.T = T;
    if (S_tap) t.S = A.alloc<float>(nbins);
    if (f_tap) t.f = A.alloc<double>(nbins);
    if (m_tap) t.m = A.alloc<float>(nbins);
  }
  for (long k = 0; k < K; ++k)       // exactly a session's steps: set k & 1 is read, the other one written
    dn_live_step(d, dx + (size_t)k * d.B, (long)frames, (int)(k & 1), (uint64_t)k, dy + (size_t)k * d.B, (long)frames, s, &t);
  RVCX_HIP(hipMemcpyAsync(y, dy, nx * 4, hipMemcpyDefault, s));
  if (t.S) RVCX_HIP(hipMemcpyAsync(S_tap, t.S, nbins * 4, hipMemcpyDefault, s));
  if (t.f) RVCX_HIP(hipMemcpyAsync(f_tap, t.f, nbins * 8, hipMemcpyDefault, s));
  if (t.m) RVCX_HIP(hipMemcpyAsync(m_tap, t.m, nbins * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  A.reset();
  API_END
}

}  // extern "C"
