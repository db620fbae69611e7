// C ABI of librvcx.so (include/rvcx.h "live post-production"): the effects board inside a live-stream session, the same board
// without a session (rvcx_op_stream_fx) and the reverb's host twin.
#include "api_internal.h"
#include "effects.h"

using namespace rvcx;
using namespace rvcx::api;

namespace {

// what a step launches, from a validated plan (the expressions of fx_run, api_fx.hip); mask bit i keeps stage i + 1
FxLivePlan live_plan(const FxPlan& P, unsigned mask) {
  FxLivePlan L;
  const bool on[7] = {P.hp, P.comp, P.gate, P.reverb, P.lo, P.hi, P.chorus};
  for (int k = 0; k < 7; ++k) L.on[k] = on[k] && ((mask >> k) & 1u);
  L.hp = fx_coeffs(0, P.sr, P.hp_fc, 0.0, 0.0);
  L.lo = fx_coeffs(1, P.sr, P.lo_fc, P.lo_q, P.lo_db);
  L.hi = fx_coeffs(2, P.sr, P.hi_fc, P.hi_q, P.hi_db);
  L.comp_ca = fx_cte(P.comp_att, P.sr), L.comp_cr = fx_cte(P.comp_rel, P.sr);
  L.comp_thr = (float)std::pow(10.0, P.comp_thr_db / 20.0), L.comp_expo = (float)(1.0 / P.comp_ratio - 1.0);
  L.gate_c0 = fx_cte(0.0, P.sr), L.gate_c50 = fx_cte(50.0, P.sr);
  L.gate_ca = fx_cte(P.gate_att, P.sr), L.gate_cr = fx_cte(P.gate_rel, P.sr);
  L.gate_thr = (float)std::pow(10.0, P.gate_thr_db / 20.0), L.gate_expo = (float)(P.gate_ratio - 1.0);
  L.rv = fx_reverb_setup(P.sr, P.room, P.damp, P.wet, P.dry, P.width);
  L.rv.omd = (float)(1.0 - (double)L.rv.d);      // the comb twin's 1 - d (fx_comb_host is handed the float d)
  L.ch = fx_chorus_setup(P.sr, P.rate, P.depth, P.centre, P.fb, P.mix);
  return L;
}

// rvcx_fx_params as a session takes them: rate and channels are the session's, the fields may say so or be 0
FxPlan session_plan(const char* who, const rvcx_fx_params& p, int sr, bool low_rate) {
  if (p.sample_rate != 0 && p.sample_rate != sr)
    fail(std::string(who) + ": sample_rate must be 0 or the rate the blocks leave at, " + std::to_string(sr));
  if (p.channels != 0 && p.channels != 2) fail(std::string(who) + ": channels must be 0 or 2 (the board returns stereo)");
  return fx_board_plan(who, p, sr, 2, low_rate);
}

// the floats of a stream's state that belong to stage k + 1 alone, {offset, count} pairs (the reverb is never an identity)
std::vector<std::pair<long, long>> stage_state(const FxLiveLayout& L, int k) {
  switch (k) {
    case 0: return {{kFxlBiquad, 4}};
    case 1: return {{kFxlFollow, 2}};
    case 2: return {{kFxlFollow + 2, 4}};
    case 4: return {{kFxlBiquad + 4, 4}};
    case 5: return {{kFxlBiquad + 8, 4}};
    default: return {{L.chorus[0], 2 * L.cap}};
  }
}

}  // namespace

extern "C" {

int rvcx_stream_open_fx(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_stream_io* io,
                        const rvcx_fx_params* fx, const rvcx_params* p, const int32_t* sid, const float* pitch, int* stream_id) {
  if (!fx) return rvcx_stream_open_io(ctx, model_id, cfg, io, p, sid, pitch, stream_id);
  CtxLock ctx_guard_ = lock_ctx(ctx);
  // every refusal of the board first: nothing is opened for parameters it would not run
  int sr = 0;
  FxPlan P;
  int rc = api_call(ctx, false, [&](Ctx* C) {
    if (!cfg) fail("stream_open_fx: null argument");
    const SynthModel& M = get_synth(*C, model_id);
    sr = io && io->out_rate != 0 ? io->out_rate : M.cfg.sr;
    P = session_plan("stream_open_fx", *fx, sr, M.cfg.sr < 8000);
  });
  if (rc != 0) return rc;
  int id = 0;
  rc = rvcx_stream_open_io(ctx, model_id, cfg, io, p, sid, pitch, &id);
  if (rc != 0) return rc;
  rc = api_call(ctx, false, [&](Ctx* C) {
    StreamSession& se = get_session(ctx, id);
    auto f = std::make_unique<FxLive>();
    f->S = se.S, f->sr = sr;
    f->B = se.out.on ? se.out.g.B_out : se.Lb;
    RVCX_CHECK(f->B * 100 == (long)se.cfg.block_frames * sr, "stream_open_fx: the block is not block_frames x 10 ms at the delivery rate");
    f->L = fx_live_layout(sr, f->B);
    f->plan = live_plan(P, ~0u);
    se.fx = std::move(f);                     // from here on the session's destructor frees what was allocated
    const size_t sb = (size_t)se.S * se.fx->L.per_stream * 4;
    for (float*& q : se.fx->state) {
      RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&q), sb));
      RVCX_HIP(hipMemsetAsync(q, 0, sb, C->stream));
    }
    RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se.fx->work), fx_live_work_floats(se.S, se.fx->B) * 4));
    RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se.fx_out), (size_t)se.S * se.fx->B * 2 * 4));
    RVCX_HIP(hipStreamSynchronize(C->stream));
    se.fxp = *fx;
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

int rvcx_stream_out_channels(rvcx_ctx* ctx, int stream_id) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  auto it = ctx->sessions.find(stream_id);
  return it == ctx->sessions.end() ? -1 : (it->second->fx ? 2 : 1);
}

int rvcx_stream_set_fx(rvcx_ctx* ctx, int stream_id, const rvcx_fx_params* fx) {
  API_BEGIN(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  if (!fx) fail("stream_set_fx: null parameters");
  if (!se.fx) fail("stream_set_fx: the session was opened without effects (its channel count is fixed at open)");
  FxLive& f = *se.fx;
  const FxLivePlan next = live_plan(session_plan("stream_set_fx", *fx, f.sr, f.sr < 8000), ~0u);
  // every check has passed.  A stage the new values make an identity forgets its state, in both sets: it starts clean when
  // it comes back; everything else is kept, so a tail rings on
  bool any = false;
  for (int k = 0; k < 7; ++k) {
    if (!f.plan.on[k] || next.on[k]) continue;
    for (const auto& span : stage_state(f.L, k))
      for (float* q : f.state)
        RVCX_HIP(hipMemset2DAsync(q + span.first, (size_t)f.L.per_stream * 4, 0, (size_t)span.second * 4, (size_t)f.S, C->stream));
    any = true;
  }
  if (any) RVCX_HIP(hipStreamSynchronize(C->stream));
  f.plan = next;
  se.fxp = *fx;
  API_END
}

int rvcx_stream_last_fx_ms(rvcx_ctx* ctx, int stream_id, float* ms8) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ms8) return -1;
  auto it = ctx->sessions.find(stream_id);
  if (it == ctx->sessions.end() || !it->second->fx) return -1;
  std::copy(it->second->fx_ms, it->second->fx_ms + 8, ms8);
  return 0;
}

int rvcx_op_stream_fx(rvcx_ctx* ctx, const float* x, int S, int64_t frames, int channels, int sr, int block_frames,
                      const rvcx_fx_params* fx, uint32_t stage_mask, float* y) {
  API_BEGIN(ctx)
  if (!x || !y || !fx) fail("op_stream_fx: null argument");
  if (S < 1 || frames < 1 || block_frames < 1) fail("op_stream_fx: S, frames and block_frames >= 1");
  if (channels != 1 && channels != 2) fail("op_stream_fx: channels must be 1 or 2");
  const FxPlan P = session_plan("op_stream_fx", *fx, sr, true);
  FxLive f;
  f.S = S, f.sr = sr, f.B = (long)block_frames * sr / 100;
  if (frames % f.B != 0)
    fail("op_stream_fx: frames must be a multiple of the block, block_frames * sr / 100 = " + std::to_string(f.B));
  f.L = fx_live_layout(sr, f.B);
  f.plan = live_plan(P, stage_mask);
  const long K = (long)(frames / f.B);
  const size_t nx = (size_t)S * frames * channels, ny = (size_t)S * frames * 2, ns = (size_t)S * f.L.per_stream;
  if (ny > ((size_t)1 << 31)) fail("op_stream_fx: more than 2^31 samples");
  C->arena.reserve((nx + ny + 2 * ns + fx_live_work_floats(S, f.B)) * 4 + (1 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  for (float*& q : f.state) {
    q = C->arena.alloc<float>(ns);
    RVCX_HIP(hipMemsetAsync(q, 0, ns * 4, s));
  }
  f.work = C->arena.alloc<float>(fx_live_work_floats(S, f.B));
  for (long k = 0; k < K; ++k)       // exactly a session's steps: set k & 1 is read, the other one written
    fx_live_step(f, dx + (size_t)k * f.B * channels, (long)(frames * channels), channels, (int)(k & 1), (uint64_t)k,
                 dy + (size_t)k * f.B * 2, (long)(frames * 2), s, nullptr);
  RVCX_HIP(hipMemcpyAsync(y, dy, ny * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->arena.reset();
  API_END
}

int rvcx_fx_reverb_host(const float* x, int64_t n, int sr, float room_size, float damping, float wet, float dry, float width,
                        float* y) {
  try {
    if (!x || !y) fail("fx_reverb_host: null pointer");
    if (n < 0) fail("fx_reverb_host: n < 0");
    FxPlan P;
    P.sr = sr, P.C = 2, P.reverb = true, P.room = room_size, P.damp = damping, P.wet = wet, P.dry = dry, P.width = width;
    fx_validate("fx_reverb_host", P);
    FxReverb rv = fx_reverb_setup(sr, room_size, damping, wet, dry, width);
    fx_reverb_host(rv, x, (long)n, y);
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

}  // extern "C"
