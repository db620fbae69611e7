// C ABI of librvcx.so (include/rvcx.h "live formant shift", stage 19): the causal formant shift at either edge of a live-stream
// session's step (rvcx_stream_open_fm, _set_formant, _last_fm_ms; the step itself is api_stream.hip's), the same stage without a
// session (rvcx_op_stream_formant), its host twin and the delay rule.
#include "api_fx_common.h"
#include "formant_live.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

struct LivePlan {
  int sr, nc;
  FxStretchGeom g;
  FxFormantValues v;
};

// every refusal that depends on the parameters alone; sr: the rate the side runs at (params->sample_rate may be 0 or sr)
LivePlan live_check(const char* who_c, const rvcx_live_formant_params* p, int sr) {
  const std::string who(who_c);
  if (!p) fail(who + ": null parameters");
  if (p->sample_rate != 0 && p->sample_rate != sr) fail(who + ": sample_rate must be 0 or the rate of the signal, " + std::to_string(sr));
  check_rate(who_c, sr, true);
  if (p->channels != 0 && p->channels != 1) fail(who + ": channels must be 0 or 1 (the live formant shift is mono)");
  check_finite(who_c, {p->ratio, p->amount, p->quefrency_ms, p->max_gain_db});
  check_range(who_c, p->ratio, 0.5, 2.0, "ratio");
  check_range(who_c, p->amount, 0.0, 1.0, "amount");
  check_range(who_c, p->max_gain_db, 0.0, 48.0, "max_gain_db");
  if (p->iterations < 0 || p->iterations > kFormantMaxIter) fail(who + ": iterations must lie in 0 .. 16");
  if (p->keep_energy != 0 && p->keep_energy != 1) fail(who + ": keep_energy must be 0 or 1");
  if (!(p->quefrency_ms > 0.f)) fail(who + ": quefrency_ms must be positive");
  LivePlan P;
  P.sr = sr, P.g = dn_live_geom(sr);
  const double nc = fx_formant_nc(p->quefrency_ms, sr);
  if (!(nc >= 1.0 && nc <= (double)(P.g.N / 8)))
    fail(who + ": quefrency_ms must span 1 .. " + std::to_string(P.g.N / 8) + " samples (N / 8) at this rate");
  P.nc = (int)nc;
  P.v = FxFormantValues{p->ratio, p->amount, p->quefrency_ms, p->max_gain_db, p->iterations, p->keep_energy};
  return P;
}

}  // namespace

extern "C" {

int rvcx_stream_formant_delay(int sr) { return dn_live_rate_ok(sr) ? dn_live_geom(sr).N : -1; }

int rvcx_stream_formant_frames(int64_t n, int sr, float quefrency_ms, int64_t* T, int32_t* N, int32_t* nc) {
  return host_call([&] {
    rvcx_live_formant_params p = {0, 0, 1.f, 1.f, quefrency_ms, 8, 24.f, 1};
    const LivePlan P = live_check("stream_formant_frames", &p, sr);
    if (n < 0 || n > (int64_t)1 << 40) fail("stream_formant_frames: n out of range");
    if (T) *T = dn_live_frames((long)n, P.g.N, P.g.H);
    if (N) *N = P.g.N;
    if (nc) *nc = P.nc;
  });
}

int rvcx_stream_open_fm(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_stream_io* io, const rvcx_fx_params* fx,
                        const rvcx_stream_dn* dn, const rvcx_stream_fm* fm, const rvcx_params* p, const int32_t* sid,
                        const float* pitch, int* stream_id) {
  if (!fm || (!fm->in.params && !fm->out.params)) return rvcx_stream_open_dn(ctx, model_id, cfg, io, fx, dn, p, sid, pitch, stream_id);
  CtxLock ctx_guard_ = lock_ctx(ctx);
  const rvcx_stream_fm_side* sides[2] = {&fm->in, &fm->out};
  // every refusal of both sides first: nothing is opened for parameters they would not run (rvcx_stream_open_dn then makes its
  // own in front of anything it opens)
  LivePlan P[2];
  int rc = api_call(ctx, false, [&](Ctx* C) {
    if (!cfg) fail("stream_open_fm: null argument");
    const SynthModel& M = get_synth(*C, model_id);
    const int rate[2] = {16000, io && io->out_rate != 0 ? io->out_rate : M.cfg.sr};
    for (int k = 0; k < 2; ++k)
      if (sides[k]->params)
        P[k] = live_check(k == 0 ? "stream_open_fm (input side)" : "stream_open_fm (output side)", sides[k]->params, rate[k]);
  });
  if (rc != 0) return rc;
  int id = 0;
  rc = rvcx_stream_open_dn(ctx, model_id, cfg, io, fx, dn, p, sid, pitch, &id);
  if (rc != 0) return rc;
  rc = api_call(ctx, false, [&](Ctx* C) {
    StreamSession& se = get_session(ctx, id);
    hipStream_t s = C->stream;
    for (int k = 0; k < 2; ++k) {
      if (!sides[k]->params) continue;
      StreamSession::FmSide& sd = se.fm[k];
      auto d = std::make_unique<FmLive>();
      d->S = se.S, d->sr = P[k].sr, d->nc = P[k].nc, d->g = P[k].g, d->v = P[k].v;
      d->B = k == 0 ? (long)se.cfg.block_frames * 160 : (se.out.on ? se.out.g.B_out : se.Lb);
      RVCX_CHECK(d->B * 100 == (long)se.cfg.block_frames * d->sr, "stream_open_fm: the block is not block_frames x 10 ms at the side's rate");
      sd.d = std::move(d);                    // from here on the session's destructor frees what was allocated
      FmLive& L = *sd.d;
      const int N = L.g.N;
      const size_t sb = (size_t)se.S * fm_live_per_stream(L) * 4;
      for (float*& q : L.state) {
        RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&q), sb));
        RVCX_HIP(hipMemsetAsync(q, 0, sb, s));
      }
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&L.fr), (size_t)se.S * fm_live_slots(L) * N * 4));
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&sd.stage), (size_t)se.S * L.B * 4));
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&sd.tables), (size_t)2 * N * 4));
      const StftTables tables(N);             // (into the session's own memory, not the arena)
      RVCX_HIP(hipMemcpyAsync(sd.tables, tables.w.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
      RVCX_HIP(hipMemcpyAsync(sd.tables + N, tables.tw.data(), (size_t)N / 2 * 8, hipMemcpyHostToDevice, s));
      RVCX_HIP(hipStreamSynchronize(s));      // (the tables are this scope's)
      L.w = sd.tables, L.tw = reinterpret_cast<const float2*>(sd.tables + N);
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

int rvcx_stream_set_formant(rvcx_ctx* ctx, int stream_id, int side, const rvcx_live_formant_params* params) {
  API_BEGIN(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  if (side != 0 && side != 1) fail("stream_set_formant: side must be 0 (input) or 1 (output)");
  StreamSession::FmSide& sd = se.fm[side];
  if (!sd.d) fail("stream_set_formant: the session was opened without a formant shift on this side (its delay is fixed at open)");
  const LivePlan P = live_check("stream_set_formant", params, sd.d->sr);
  // every check has passed: nothing below can fail, all state is kept
  sd.d->nc = P.nc, sd.d->v = P.v;
  sd.p = *params;
  API_END
}

int rvcx_stream_last_fm_ms(rvcx_ctx* ctx, int stream_id, float* ms2) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ms2) return -1;
  auto it = ctx->sessions.find(stream_id);
  if (it == ctx->sessions.end()) return -1;
  for (int k = 0; k < 2; ++k) ms2[k] = it->second->fm[k].d ? it->second->fm_ms[k] : 0.f;
  return 0;
}

int rvcx_fx_formant_live_host(const float* x, int64_t n, int sr, const rvcx_live_formant_params* params, float* y, float* D,
                              float* E, float* g, float* s) {
  return host_call([&] {
    const LivePlan P = live_check("fx_formant_live_host", params, sr);
    if (!x || !y) fail("fx_formant_live_host: null pointer");
    check_frames("fx_formant_live_host", n, "1 .. 2^30 samples are required");
    fm_live_host(x, (long)n, sr, P.v, y, D, E, g, s);
  });
}

int rvcx_op_stream_formant(rvcx_ctx* ctx, const float* x, int S, int64_t frames, int sr, int block_frames,
                           const rvcx_live_formant_params* params, float* y, float* E_tap, float* g_tap, float* s_tap) {
  const int64_t from0 = 0;
  return rvcx_op_stream_formant_history(ctx, x, S, frames, sr, block_frames, 1, params, &from0, y, E_tap, g_tap, s_tap);
}

int rvcx_op_stream_formant_history(rvcx_ctx* ctx, const float* x, int S, int64_t frames, int sr, int block_frames, int n_params,
                                   const rvcx_live_formant_params* params, const int64_t* from_block, float* y, float* E_tap,
                                   float* g_tap, float* s_tap) {
  API_BEGIN(ctx)
  if (n_params < 1 || !params || !from_block) fail("op_stream_formant: null parameters");
  std::vector<LivePlan> plans;
  for (int i = 0; i < n_params; ++i) {
    plans.push_back(live_check("op_stream_formant", params + i, sr));
    if (i == 0 ? from_block[0] != 0 : from_block[i] <= from_block[i - 1])
      fail("op_stream_formant: the parameter history starts at block 0 and ascends");
  }
  const LivePlan& P = plans[0];
  if (!x || !y) fail("op_stream_formant: null argument");
  if (S < 1 || S > 4096 || frames < 1 || block_frames < 1) fail("op_stream_formant: S in 1 .. 4096, frames and block_frames >= 1");
  FmLive d;
  d.S = S, d.sr = sr, d.nc = P.nc, d.g = P.g, d.v = P.v;
  d.B = (long)block_frames * sr / 100;
  if (frames % d.B != 0)
    fail("op_stream_formant: frames must be a multiple of the block, block_frames * sr / 100 = " + std::to_string(d.B));
  const long K = (long)(frames / d.B), T = dn_live_frames((long)frames, P.g.N, P.g.H);
  const size_t nx = (size_t)S * frames, ns = (size_t)S * fm_live_per_stream(d), nfr = (size_t)S * fm_live_slots(d) * P.g.N,
               nfrm = (size_t)S * std::max(T, 1L), nbins = nfrm * P.g.nb;
  if (nx > ((size_t)1 << 31)) fail("op_stream_formant: more than 2^31 samples");
  C->arena.reserve((2 * nx + 2 * ns + nfr + (size_t)2 * P.g.N) * 4 + (E_tap ? nbins * 4 : 0) + (g_tap ? nbins * 4 : 0) +
                   (s_tap ? nfrm * 4 : 0) + (1 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  Arena& A = C->arena;
  const StftTables tables(P.g.N);
  tables.upload(*C, d.w, d.tw);
  float* dx = to_dev(*C, x, nx);
  float* dy = A.alloc<float>(nx);
  for (float*& q : d.state) {
    q = A.alloc<float>(ns);
    RVCX_HIP(hipMemsetAsync(q, 0, ns * 4, s));
  }
  d.fr = A.alloc<float>(nfr);
  FmLiveTaps t;
  if ((E_tap || g_tap || s_tap) && T > 0) {
    t.T = T;
    if (E_tap) t.E = A.alloc<float>(nbins);
    if (g_tap) t.g = A.alloc<float>(nbins);
    if (s_tap) t.s = A.alloc<float>(nfrm);
  }
  int at = 0;
  for (long k = 0; k < K; ++k) {     // exactly a session's steps: set k & 1 is read, the other one written
    while (at + 1 < n_params && from_block[at + 1] <= k) ++at;
    d.nc = plans[at].nc, d.v = plans[at].v;
    fm_live_step(d, dx + (size_t)k * d.B, (long)frames, (int)(k & 1), (uint64_t)k, dy + (size_t)k * d.B, (long)frames, s, &t);
  }
  RVCX_HIP(hipMemcpyAsync(y, dy, nx * 4, hipMemcpyDefault, s));
  if (t.E) RVCX_HIP(hipMemcpyAsync(E_tap, t.E, nbins * 4, hipMemcpyDefault, s));
  if (t.g) RVCX_HIP(hipMemcpyAsync(g_tap, t.g, nbins * 4, hipMemcpyDefault, s));
  if (t.s) RVCX_HIP(hipMemcpyAsync(s_tap, t.s, nfrm * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  A.reset();
  API_END
}

}  // extern "C"
