// C ABI of librvcx.so (include/rvcx.h): live-stream sessions.
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

extern "C" {

// ------------------------------------------------------------------------------------------ live streams (rvcx.h)
int rvcx_op_sola(rvcx_ctx* ctx, const float* y, const float* b_in, int Lb, int Lx, int Ls, float* out, float* b_out,
                 int32_t* offset, float* scores) {
  API_BEGIN(ctx)
  if (!y || !b_in || !out || !b_out) fail("sola: null argument");
  if (Lb < 1 || Lx < 1 || Ls < 0) fail("sola: Lb, Lx >= 1 and Ls >= 0");
  const size_t Ly = (size_t)Lb + Lx + Ls;
  C->arena.reserve((Ly + 2 * (size_t)Lx + Lb + Ls + 64) * 4 + (1 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dy = to_dev(*C, y, Ly);
  float* db = to_dev(*C, b_in, (size_t)Lx);
  float* dout = C->arena.alloc<float>((size_t)Lb);
  float* dbo = C->arena.alloc<float>((size_t)Lx);
  float* dsc = C->arena.alloc<float>((size_t)Ls + 1);
  int* doff = C->arena.alloc<int>(1);
  launch_sola(dy, (long)Ly, db, dout, Lb, dbo, doff, dsc, 1, Lb, Lx, Ls, s);
  RVCX_HIP(hipMemcpyAsync(out, dout, (size_t)Lb * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipMemcpyAsync(b_out, dbo, (size_t)Lx * 4, hipMemcpyDefault, s));
  if (offset) RVCX_HIP(hipMemcpyAsync(offset, doff, 4, hipMemcpyDefault, s));
  if (scores) RVCX_HIP(hipMemcpyAsync(scores, dsc, ((size_t)Ls + 1) * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->arena.reset();
  API_END
}

// arena bytes of one step of S streams (the stages run one after the other on the main stream: the sum is an upper bound)
static size_t stream_step_bytes(Ctx& c, const SynthModel& M, const rvcx_params& p, int S, int N, int Th, int T, long Lk,
                                long Lb, long Ls) {
  const long n = (long)N * 160;
  const size_t E = (size_t)M.cfg.input_dim;
  size_t need = f0_arena_bytes(c, p, S, n) + hubert_arena_bytes(*c.hubert, S, n) + synth_arena_bytes(M, S, T);
  need += (size_t)S * ((size_t)(N + 8) * 32 + 2 * E * Th + E * T + (size_t)M.cfg.inter_channels * T + 2 * (size_t)Lk + Lb + Ls + 64) * 4;
  need += (size_t)S * T * M.upp * 2 * 4;       // RVCX_STREAM_FULL_SYNTH: whole-length source noise and output
  if (c.index) need += index_arena_bytes(*c.index, Th);
  return need + ((size_t)64 << 20);
}

static StreamSession& get_session(rvcx_ctx* h, int id) {
  auto it = h->sessions.find(id);
  if (it == h->sessions.end()) fail("stream: unknown session " + std::to_string(id));
  return *it->second;
}

int rvcx_stream_open(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_params* p, const int32_t* sid,
                     const float* pitch, int* stream_id) {
  API_BEGIN_ONCE(ctx)
  if (!cfg || !p || !sid || !pitch || !stream_id) fail("stream_open: null argument");
  SynthModel& M = get_synth(*C, model_id);
  if (!C->hubert) fail("stream_open: hubert not loaded");
  if (p->f0_method == RVCX_F0_CREPE)
    fail("stream_open: mangio-crepe is not available to live streams (its Viterbi pass and host dither have no place in a "
         "per-block loop); use rmvpe or fcpe");
  check_f0_backend(*C, *p);
  const int S = cfg->n_streams, Fb = cfg->block_frames, Fc = cfg->context_frames, Fx = cfg->crossfade_frames,
            Fs = cfg->search_frames;
  if (S < 1 || Fb < 1 || Fx < 1 || Fs < 0 || Fc < 0) fail("stream_open: n_streams, block, cross-fade >= 1 and context, search >= 0 frames");
  const int E = M.cfg.input_dim;
  RVCX_CHECK(E == C->hubert->cfg.embed_dim || (C->hubert->has_final_proj && E == C->hubert->final_proj.cout),
             "the voice model's input_dim is neither the HuBERT's embed_dim (v2) nor its final_proj width (v1)");
  if (C->index && C->index->dim != E)
    fail("stream_open: the resident index holds " + std::to_string(C->index->dim) + "-wide vectors, the voice model takes " +
         std::to_string(E) + "-wide features");
  const long Nl = (long)Fc + Fx + Fs + Fb;
  if (Nl > 6000) fail("stream_open: more than 60 s of context");
  const int N = (int)Nl;
  const int Th = hubert_frames(*C->hubert, (int64_t)N * 160);
  if (Th <= 0) fail("stream_open: the ring is too short for the HuBERT");
  const int T = std::min(N, 2 * Th);                 // p_len clamp, pipeline.py:257-262
  const int Fk = Fb + Fx + Fs;
  if (Fk > T)
    fail("stream_open: block + cross-fade + search = " + std::to_string(Fk) + " frames exceed the " + std::to_string(T) +
         " frames a step synthesizes from");
  for (int s = 0; s < S; ++s)
    if (sid[s] < 0 || sid[s] >= M.cfg.spk_embed_dim) fail("stream_open: speaker id out of range");
  auto se = std::make_unique<StreamSession>();
  se->model_id = model_id;
  se->region = M.region;
  se->cfg = *cfg;
  se->p = *p;
  se->sid.assign(sid, sid + S);
  se->pitch.assign(pitch, pitch + S);
  se->full_synth = getenv("RVCX_STREAM_FULL_SYNTH") && atoi(getenv("RVCX_STREAM_FULL_SYNTH")) != 0;
  se->S = S, se->N = N, se->Th = Th, se->T = T, se->head = T - Fk, se->upp = M.upp, se->inter = M.cfg.inter_channels, se->E = E;
  se->Lb = (long)Fb * M.upp, se->Lx = (long)Fx * M.upp, se->Ls = (long)Fs * M.upp, se->Lk = (long)Fk * M.upp;
  RVCX_CHECK((size_t)se->inter * T < ((size_t)1 << 24) && (size_t)T * M.upp < ((size_t)1 << 24), "stream_open: step too long for its noise counters");
  {
    const size_t budget = arena_budget(*C);
    if (stream_step_bytes(*C, M, *p, S, N, Th, T, se->Lk, se->Lb, se->Ls) > budget) {
      int fit = S - 1;
      while (fit > 0 && stream_step_bytes(*C, M, *p, fit, N, Th, T, se->Lk, se->Lb, se->Ls) > budget) --fit;
      fail("stream_open: one step of " + std::to_string(S) + " streams does not fit the activation budget; the largest "
           "n_streams that fits is " + std::to_string(fit));
    }
  }
  const size_t ring_b = (size_t)S * N * 160 * 4, carry_b = (size_t)S * se->Lx * 4;
  for (int k = 0; k < 2; ++k) {
    RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se->ring[k]), ring_b));
    RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se->carry[k]), carry_b));
    RVCX_HIP(hipMemsetAsync(se->ring[k], 0, ring_b, C->stream));
    RVCX_HIP(hipMemsetAsync(se->carry[k], 0, carry_b, C->stream));
  }
  RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se->blocks), (size_t)S * Fb * 160 * 4));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  const int id = ctx->next_session++;
  ctx->sessions[id] = std::move(se);
  *stream_id = id;
  API_END
}

int rvcx_stream_step(rvcx_ctx* ctx, int stream_id, const float* const* block16k, const float* const* noise,
                     float* const* out, float* const* pre_sola, int32_t* offsets) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  StreamSession* done = nullptr;
  const int rc = api_call(ctx, true, [&](Ctx* C) {
    StreamSession& se = get_session(ctx, stream_id);
    if (!block16k || !out) fail("stream_step: null argument");
    if (se.region.expired() || se.model_id >= (int)C->synths.size() || !C->synths[se.model_id] ||
        C->synths[se.model_id]->region != se.region.lock())
      fail("stream_step: the session's voice model was unloaded; close the session");
    if (!C->hubert) fail("stream_step: hubert not loaded");
    check_f0_backend(*C, se.p);
    SynthModel& M = *C->synths[se.model_id];
    const int S = se.S, N = se.N, Th = se.Th, T = se.T, E = se.E, inter = se.inter;
    const long n = (long)N * 160, blk = (long)se.cfg.block_frames * 160, Lb = se.Lb, Lx = se.Lx, Ls = se.Ls, Lk = se.Lk;
    if (C->index && se.p.index_rate != 0.f && C->index->dim != E) fail("stream_step: the resident index does not match the voice model's input_dim");
    for (int s = 0; s < S; ++s)
      if (!block16k[s] || !out[s] || (noise && !noise[s]) || (pre_sola && !pre_sola[s])) fail("stream_step: null pointer in a table");
    C->ensure_splitk(S);
    C->arena.reserve(stream_step_bytes(*C, M, se.p, S, N, Th, T, Lk, Lb, Ls));
    C->arena.reset();
    hipStream_t st = C->stream;
    Arena& A = C->arena;
    if (se.full_synth && noise) fail("stream_step: RVCX_STREAM_FULL_SYNTH=1 sessions take no parity noise");
    const long Lsyn = se.full_synth ? (long)T * M.upp : Lk;      // samples the synthesizer writes per stream
    C->timer.make();
    hipEvent_t* ev = C->timer.ev;        // {start, F0, HuBERT, blend + mix + noise = synthesizer start, enc_p, flow, decoder, SOLA + copies}
    RVCX_HIP(hipEventRecord(ev[0], st));
    // (1) the rings move left by one block
    for (int s = 0; s < S; ++s)
      RVCX_HIP(hipMemcpyAsync(se.blocks + (size_t)s * blk, block16k[s], (size_t)blk * 4, hipMemcpyDefault, st));
    const float* ring_old = se.ring[se.cur];
    float* ring = se.ring[se.cur ^ 1];
    launch_ring_shift(ring_old, ring, se.blocks, S, n, blk, st);
    // (2) VC.get_f0 on the whole ring, B = S; pitch shift and coarse quantisation with each stream's own pitch
    int* dp = A.alloc<int>((size_t)S * T);
    float* dpf = A.alloc<float>((size_t)S * T);
    {
      const size_t mk = A.mark();
      F0Opts o;
      o.pitch = se.pitch.data();
      if (se.p.f0_method == RVCX_F0_FCPE) {          // compute_f0(x, p_len = N), then the first T frames (pipeline.py:169-181)
        int* cN = A.alloc<int>((size_t)S * N);
        float* fN = A.alloc<float>((size_t)S * N);
        o.frames = N;
        get_f0_device(*C, ring, S, n, se.p, cN, fN, N, st, o);
        launch_copy_strided(fN, dpf, S, T, N, T, st);
        launch_copy_strided(reinterpret_cast<const float*>(cN), reinterpret_cast<float*>(dp), S, T, N, T, st);
      } else {
        o.frames = T;
        get_f0_device(*C, ring, S, n, se.p, dp, dpf, T, st, o);
      }
      A.reset(mk);       // (stream order: everything later on `st` runs behind these launches)
    }
    RVCX_HIP(hipEventRecord(ev[1], st));
    // (3) VC.vc's front: HuBERT, retrieval blend, x2 upsample + protect mix
    float* phone = A.alloc<float>((size_t)S * E * T);
    float* zn = A.alloc<float>((size_t)S * inter * T);
    float* sn = A.alloc<float>((size_t)S * Lsyn);
    float* y = A.alloc<float>((size_t)S * Lsyn);
    vc_front(*C, E, S, ring, n, Th, T, dpf, se.p.index_rate, se.p.protect, phone, st, ev[2]);
    // the two Gaussian draws: parity noise (Lsyn = Lk then), or Philox(seed + s) at counters no two steps share (2^23 quads
    // per draw)
    for (int s = 0; s < S; ++s) {
      fill_noise(zn + (size_t)s * inter * T, noise ? noise[s] : nullptr, (size_t)inter * T, se.p.seed + (uint64_t)s,
                 se.step << 24, st);
      fill_noise(sn + (size_t)s * Lsyn, noise ? noise[s] + (size_t)inter * T : nullptr, (size_t)Lsyn, se.p.seed + (uint64_t)s,
                 (se.step << 24) + ((uint64_t)1 << 23), st);
    }
    // (4) the synthesizer on the tail
    SynthIO io;
    io.B = S;
    io.T = T;
    io.phone_ct = phone;
    io.pitch = dp;
    io.pitchf = dpf;
    io.sid_host = se.sid.data();
    io.z_noise = zn;
    io.src_noise = sn;
    io.out = y;
    io.skip_head = se.full_synth ? 0 : se.head;
    synth_forward(*C, M, io, ev + 3);
    // (5) SOLA per stream; the offset stays on the device
    float* dout = A.alloc<float>((size_t)S * Lb);
    float* dsc = A.alloc<float>((size_t)S * (Ls + 1));
    int* doff = A.alloc<int>((size_t)S);
    const float* tail = y + (Lsyn - Lk);                           // the last Fb + Fx + Fs frames of every row
    launch_sola(tail, Lsyn, se.carry[se.cur], dout, Lb, se.carry[se.cur ^ 1], doff, dsc, S, (int)Lb, (int)Lx, (int)Ls, st);
    for (int s = 0; s < S; ++s) {
      RVCX_HIP(hipMemcpyAsync(out[s], dout + (size_t)s * Lb, (size_t)Lb * 4, hipMemcpyDefault, st));
      if (pre_sola) RVCX_HIP(hipMemcpyAsync(pre_sola[s], tail + (size_t)s * Lsyn, (size_t)Lk * 4, hipMemcpyDefault, st));
    }
    if (offsets) RVCX_HIP(hipMemcpyAsync(offsets, doff, (size_t)S * 4, hipMemcpyDefault, st));
    RVCX_HIP(hipEventRecord(ev[7], st));
    C->snapshot_dev_err(st);
    RVCX_HIP(hipStreamSynchronize(st));
    C->check_dev_err();
    {   // rvcx_last_timing: {0, F0, HuBERT, blend + mix, enc_p, flow, decoder, SOLA + copies, total} of this step
      float* ms = C->timing;
      ms[0] = 0.f;
      for (int k = 1; k <= 7; ++k) RVCX_HIP(hipEventElapsedTime(&ms[k], ev[k - 1], ev[k]));
      RVCX_HIP(hipEventElapsedTime(&ms[8], ev[0], ev[7]));
    }
    A.reset();
    done = &se;
  });
  if (rc == 0 && done) {      // the step stands: the sets written become the session's state
    done->cur ^= 1;
    done->step++;
  }
  return rc;
}

int rvcx_stream_reset(rvcx_ctx* ctx, int stream_id) {
  API_BEGIN_ONCE(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  RVCX_HIP(hipMemsetAsync(se.ring[se.cur], 0, (size_t)se.S * se.N * 160 * 4, C->stream));
  RVCX_HIP(hipMemsetAsync(se.carry[se.cur], 0, (size_t)se.S * se.Lx * 4, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  se.step = 0;
  API_END
}

int rvcx_stream_close(rvcx_ctx* ctx, int stream_id) {
  API_BEGIN_ONCE(ctx)
  (void)get_session(ctx, stream_id);
  RVCX_HIP(hipDeviceSynchronize());
  ctx->sessions.erase(stream_id);
  API_END
}

static int64_t stream_query(rvcx_ctx* ctx, int stream_id, int what) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  auto it = ctx->sessions.find(stream_id);
  if (it == ctx->sessions.end()) return -1;
  const StreamSession& se = *it->second;
  return what == 0 ? (int64_t)se.Lb : what == 1 ? (int64_t)se.inter * se.T + se.Lk : (int64_t)se.T;
}
int64_t rvcx_stream_out_len(rvcx_ctx* ctx, int stream_id) { return stream_query(ctx, stream_id, 0); }
int64_t rvcx_stream_noise_len(rvcx_ctx* ctx, int stream_id) { return stream_query(ctx, stream_id, 1); }
int rvcx_stream_frames(rvcx_ctx* ctx, int stream_id) { return (int)stream_query(ctx, stream_id, 2); }

}  // extern "C"
