// C ABI of librvcx.so (include/rvcx.h): live-stream sessions (api_stream_fx.hip: the effects board inside them).
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

namespace rvcx {
namespace api {
StreamSession& get_session(rvcx_ctx* h, int id) {
  auto it = h->sessions.find(id);
  if (it == h->sessions.end()) fail("stream: unknown session " + std::to_string(id));
  return *it->second;
}
}  // namespace api
}  // namespace rvcx

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
                                long Lb, long Ls, long Bout = 0 /* the resampled output block, when there is one */) {
  const long n = (long)N * 160;
  const size_t E = (size_t)M.cfg.input_dim;
  size_t need = f0_arena_bytes(c, p, S, n) + hubert_arena_bytes(*c.hubert, S, n) + synth_arena_bytes(M, S, T);
  need += (size_t)S * ((size_t)(N + 8) * 32 + 2 * E * Th + E * T + (size_t)M.cfg.inter_channels * T + 2 * (size_t)Lk + Lb + Ls + 64) * 4;
  need += (size_t)S * T * M.upp * 2 * 4;       // RVCX_STREAM_FULL_SYNTH: whole-length source noise and output
  need += (size_t)S * ((size_t)Bout + 64) * 4;
  if (c.index) need += index_arena_bytes(*c.index, Th);
  return need + ((size_t)64 << 20);
}

static const char kRateRule[] =
    " must be a multiple of 100 Hz within 8000 .. 192000 (a 10 ms frame is a whole number of samples; below 8000 only beside "
    "a partner below 8000)";

// the filter tables of the sides that filter: the session's own memory, one allocation when both sides have one gain
static void build_stream_tables(Ctx& c, StreamSession& se) {
  StreamSide* sides[2] = {&se.in, &se.out};
  const size_t tb = resample_table_doubles(0) * sizeof(double);
  int k = 0;
  for (StreamSide* sd : sides) {
    if (!sd->on || !sd->g.filter) continue;
    const double gain = std::min(1.0, (double)sd->g.sr_out / (double)sd->g.sr_in);
    const bool share = sd == &se.out && se.in.on && se.in.g.filter && se.in.f.scale == gain;
    if (!share) RVCX_HIP(hipMalloc(reinterpret_cast<void**>(&se.tables[k++]), tb));
    sd->f = make_resample_filter_at(share ? se.tables[0] : se.tables[k - 1], sd->g.sr_in, sd->g.sr_out, c.stream, 0);
  }
}

int rvcx_stream_open(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_params* p, const int32_t* sid,
                     const float* pitch, int* stream_id) {
  return rvcx_stream_open_io(ctx, model_id, cfg, nullptr, p, sid, pitch, stream_id);
}

int rvcx_stream_open_io(rvcx_ctx* ctx, int model_id, const rvcx_stream_cfg* cfg, const rvcx_stream_io* io_arg,
                        const rvcx_params* p, const int32_t* sid, const float* pitch, int* stream_id) {
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
  rvcx_stream_io io{0, 1, 0, 0};
  if (io_arg) io = *io_arg;
  if (io.in_channels < 1) fail("stream_open: in_channels >= 1");
  const int in_rate = io.in_rate == 0 ? 16000 : io.in_rate, out_rate = io.out_rate == 0 ? M.cfg.sr : io.out_rate;
  const bool in_on = in_rate != 16000 || io.in_channels != 1, out_on = out_rate != M.cfg.sr;
  if (in_on && !stream_rates_ok(in_rate, 16000)) fail("stream_open: in_rate " + std::to_string(in_rate) + kRateRule);
  if (out_on && !stream_rates_ok(M.cfg.sr, out_rate)) fail("stream_open: out_rate " + std::to_string(out_rate) + kRateRule);
  auto se = std::make_unique<StreamSession>();
  se->io = io;
  se->in.on = in_on, se->out.on = out_on;
  if (in_on) se->in.g = stream_resampler_plan(in_rate, 16000, io.in_channels, Fb);
  if (out_on) {
    RVCX_CHECK((long)Fb * M.upp * 100 == (long)Fb * M.cfg.sr, "stream_open: the voice model's rate is not 100 x its hop");
    se->out.g = stream_resampler_plan(M.cfg.sr, out_rate, 1, Fb);
  }
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
    const long Bout = se->out.on ? se->out.g.B_out : 0;
    if (stream_step_bytes(*C, M, *p, S, N, Th, T, se->Lk, se->Lb, se->Ls, Bout) > budget) {
      int fit = S - 1;
      while (fit > 0 && stream_step_bytes(*C, M, *p, fit, N, Th, T, se->Lk, se->Lb, se->Ls, Bout) > budget) --fit;
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
  auto zeroed = [&](auto** q, size_t bytes) {
    RVCX_HIP(hipMalloc(reinterpret_cast<void**>(q), bytes));
    RVCX_HIP(hipMemsetAsync(*q, 0, bytes, C->stream));
  };
  for (int k = 0; k < 2; ++k) {
    zeroed(&se->blocks[k], (size_t)S * Fb * 160 * 4);
    if (out_on) zeroed(&se->native[k], (size_t)S * se->Lb * 4);
    if (in_on && se->in.g.filter) zeroed(&se->in.fifo[k], (size_t)S * se->in.g.L * sizeof(double));
    if (out_on) zeroed(&se->out.fifo[k], (size_t)S * se->out.g.L * sizeof(double));
  }
  if (in_on) zeroed(&se->stage, (size_t)S * se->in.g.B_in * io.in_channels * 4);
  build_stream_tables(*C, *se);
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
    const long Bout = se.out.on ? se.out.g.B_out : 0;
    C->arena.reserve(stream_step_bytes(*C, M, se.p, S, N, Th, T, Lk, Lb, Ls, Bout));
    C->arena.reset();
    hipStream_t st = C->stream;
    Arena& A = C->arena;
    if (se.full_synth && noise) fail("stream_step: RVCX_STREAM_FULL_SYNTH=1 sessions take no parity noise");
    const long Lsyn = se.full_synth ? (long)T * M.upp : Lk;      // samples the synthesizer writes per stream
    C->timer.make();
    hipEvent_t* ev = C->timer.ev;        // {start, F0, HuBERT, blend + mix + noise = synthesizer start, enc_p, flow, decoder, SOLA + copies}
    RVCX_HIP(hipEventRecord(ev[0], st));
    // (1) the rings move left by one block; a session with an input side first brings the caller's blocks to 16 kHz mono
    // (FIFO set cur -> the other one, like everything below that is state)
    float* blocks = se.blocks[se.cur ^ 1];
    StreamSession::DnSide& dn_in = se.dn[0];
    StreamSession::DnSide& dn_out = se.dn[1];
    StreamSession::FmSide& fm_in = se.fm[0];
    StreamSession::FmSide& fm_out = se.fm[1];
    // a session with an input noise gate or formant shift: the 16 kHz block as it came goes to the first of them
    float* raw = dn_in.d ? dn_in.stage : (fm_in.d ? fm_in.stage : blocks);
    if (se.in.on) {
      const size_t row = (size_t)se.in.g.B_in * se.in.g.channels;
      for (int s = 0; s < S; ++s)
        RVCX_HIP(hipMemcpyAsync(se.stage + (size_t)s * row, block16k[s], row * 4, hipMemcpyDefault, st));
      launch_stream_resample(se.in.g, se.in.f, se.in.fifo[se.cur], se.in.fifo[se.cur ^ 1], se.stage, (long)row, raw, blk, S,
                             se.step, st);
    } else {
      for (int s = 0; s < S; ++s)
        RVCX_HIP(hipMemcpyAsync(raw + (size_t)s * blk, block16k[s], (size_t)blk * 4, hipMemcpyDefault, st));
    }
    if (dn_in.d) {                                    // stage 16 in front of the ring, from the state it carries
      RVCX_HIP(hipEventRecord(dn_in.ev[0], st));
      dn_live_step(*dn_in.d, raw, blk, se.cur, se.step, fm_in.d ? fm_in.stage : blocks, blk, st);
      RVCX_HIP(hipEventRecord(dn_in.ev[1], st));
    }
    if (fm_in.d) {                                    // stage 19 behind it, in front of the ring
      RVCX_HIP(hipEventRecord(fm_in.ev[0], st));
      fm_live_step(*fm_in.d, fm_in.stage, blk, se.cur, se.step, blocks, blk, st);
      RVCX_HIP(hipEventRecord(fm_in.ev[1], st));
    }
    const float* ring_old = se.ring[se.cur];
    float* ring = se.ring[se.cur ^ 1];
    launch_ring_shift(ring_old, ring, blocks, S, n, blk, st);
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
    float* dout = se.out.on ? se.native[se.cur ^ 1] : A.alloc<float>((size_t)S * Lb);
    float* dsc = A.alloc<float>((size_t)S * (Ls + 1));
    int* doff = A.alloc<int>((size_t)S);
    const float* tail = y + (Lsyn - Lk);                           // the last Fb + Fx + Fs frames of every row
    launch_sola(tail, Lsyn, se.carry[se.cur], dout, Lb, se.carry[se.cur ^ 1], doff, dsc, S, (int)Lb, (int)Lx, (int)Ls, st);
    // (6) a session with an output side: the SOLA blocks leave at out_rate
    const float* dres = dout;
    long Lo = Lb;
    if (se.out.on) {
      float* r = A.alloc<float>((size_t)S * Bout);
      launch_stream_resample(se.out.g, se.out.f, se.out.fifo[se.cur], se.out.fifo[se.cur ^ 1], dout, Lb, r, Bout, S, se.step, st);
      dres = r, Lo = Bout;
    }
    // (6b) a session with an output noise gate: stage 16 on what would have left, in front of the board
    if (dn_out.d) {
      RVCX_HIP(hipEventRecord(dn_out.ev[0], st));
      dn_live_step(*dn_out.d, dres, Lo, se.cur, se.step, dn_out.stage, Lo, st);
      RVCX_HIP(hipEventRecord(dn_out.ev[1], st));
      dres = dn_out.stage;
    }
    // (6c) a session with an output formant shift: stage 19 behind the gate, in front of the board
    if (fm_out.d) {
      RVCX_HIP(hipEventRecord(fm_out.ev[0], st));
      fm_live_step(*fm_out.d, dres, Lo, se.cur, se.step, fm_out.stage, Lo, st);
      RVCX_HIP(hipEventRecord(fm_out.ev[1], st));
      dres = fm_out.stage;
    }
    // (7) a session with effects: the board on what would have left, from the state it carries; stereo leaves
    if (se.fx) {
      fx_live_step(*se.fx, dres, Lo, 1, se.cur, se.step, se.fx_out, 2 * Lo, st, ev + 8);
      dres = se.fx_out, Lo *= 2;
    }
    for (int s = 0; s < S; ++s) {
      RVCX_HIP(hipMemcpyAsync(out[s], dres + (size_t)s * Lo, (size_t)Lo * 4, hipMemcpyDefault, st));
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
      if (se.fx) {
        for (int k = 0; k < 7; ++k) RVCX_HIP(hipEventElapsedTime(&se.fx_ms[k], ev[8 + k], ev[9 + k]));
        RVCX_HIP(hipEventElapsedTime(&se.fx_ms[7], ev[8], ev[15]));
      }
      for (int k = 0; k < 2; ++k)
        if (se.dn[k].d) RVCX_HIP(hipEventElapsedTime(&se.dn_ms[k], se.dn[k].ev[0], se.dn[k].ev[1]));
      for (int k = 0; k < 2; ++k)
        if (se.fm[k].d) RVCX_HIP(hipEventElapsedTime(&se.fm_ms[k], se.fm[k].ev[0], se.fm[k].ev[1]));
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
  RVCX_HIP(hipMemsetAsync(se.blocks[se.cur], 0, (size_t)se.S * se.cfg.block_frames * 160 * 4, C->stream));
  if (se.native[se.cur]) RVCX_HIP(hipMemsetAsync(se.native[se.cur], 0, (size_t)se.S * se.Lb * 4, C->stream));
  for (StreamSide* sd : {&se.in, &se.out})
    if (sd->fifo[se.cur]) RVCX_HIP(hipMemsetAsync(sd->fifo[se.cur], 0, (size_t)se.S * sd->g.L * sizeof(double), C->stream));
  if (se.fx)        // a ring of the board is complete only over both sets
    for (float* q : se.fx->state) RVCX_HIP(hipMemsetAsync(q, 0, (size_t)se.S * se.fx->L.per_stream * 4, C->stream));
  for (StreamSession::DnSide& sd : se.dn)
    if (sd.d)
      for (float* q : sd.d->state) RVCX_HIP(hipMemsetAsync(q, 0, (size_t)se.S * sd.d->per_stream * 4, C->stream));
  for (StreamSession::FmSide& sd : se.fm)
    if (sd.d)
      for (float* q : sd.d->state) RVCX_HIP(hipMemsetAsync(q, 0, (size_t)se.S * fm_live_per_stream(*sd.d) * 4, C->stream));
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
  if (what == 3) return se.in.on ? (int64_t)se.in.g.B_in : (int64_t)se.cfg.block_frames * 160;
  if (what == 0) return se.out.on ? (int64_t)se.out.g.B_out : (int64_t)se.Lb;
  return what == 1 ? (int64_t)se.inter * se.T + se.Lk : (int64_t)se.T;
}
int64_t rvcx_stream_in_len(rvcx_ctx* ctx, int stream_id) { return stream_query(ctx, stream_id, 3); }
int64_t rvcx_stream_out_len(rvcx_ctx* ctx, int stream_id) { return stream_query(ctx, stream_id, 0); }
int64_t rvcx_stream_noise_len(rvcx_ctx* ctx, int stream_id) { return stream_query(ctx, stream_id, 1); }
int rvcx_stream_frames(rvcx_ctx* ctx, int stream_id) { return (int)stream_query(ctx, stream_id, 2); }

int rvcx_stream_resample_delay(int sr_in, int sr_out) { return stream_resample_delay(sr_in, sr_out); }

int rvcx_stream_delays(rvcx_ctx* ctx, int stream_id, int32_t* in_delay_16k, int32_t* out_delay) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  auto it = ctx->sessions.find(stream_id);
  if (it == ctx->sessions.end()) return -1;
  const StreamSession& se = *it->second;
  if (in_delay_16k)
    *in_delay_16k = (se.in.on ? se.in.g.delay : 0) + (se.dn[0].d ? se.dn[0].d->g.N : 0) + (se.fm[0].d ? se.fm[0].d->g.N : 0);
  if (out_delay)
    *out_delay = (se.out.on ? se.out.g.delay : 0) + (se.dn[1].d ? se.dn[1].d->g.N : 0) + (se.fm[1].d ? se.fm[1].d->g.N : 0);
  return 0;
}

int rvcx_stream_last_taps(rvcx_ctx* ctx, int stream_id, float* const* in16k, float* const* native) {
  API_BEGIN(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  if (native && !se.out.on)
    fail("stream_last_taps: the output of this session is not resampled -- out_hd of the step is the native block");
  const size_t blk = (size_t)se.cfg.block_frames * 160;
  for (int s = 0; s < se.S; ++s) {
    if ((in16k && !in16k[s]) || (native && !native[s])) fail("stream_last_taps: null pointer in a table");
    if (in16k) RVCX_HIP(hipMemcpyAsync(in16k[s], se.blocks[se.cur] + s * blk, blk * 4, hipMemcpyDefault, C->stream));
    if (native)
      RVCX_HIP(hipMemcpyAsync(native[s], se.native[se.cur] + (size_t)s * se.Lb, (size_t)se.Lb * 4, hipMemcpyDefault, C->stream));
  }
  RVCX_HIP(hipStreamSynchronize(C->stream));
  API_END
}

int rvcx_stream_set(rvcx_ctx* ctx, int stream_id, const float* pitch, const int32_t* sid, float index_rate, float protect) {
  API_BEGIN(ctx)
  StreamSession& se = get_session(ctx, stream_id);
  if (sid) {
    if (se.region.expired() || se.model_id >= (int)C->synths.size() || !C->synths[se.model_id] ||
        C->synths[se.model_id]->region != se.region.lock())
      fail("stream_set: the session's voice model was unloaded; close the session");
    for (int s = 0; s < se.S; ++s)
      if (sid[s] < 0 || sid[s] >= C->synths[se.model_id]->cfg.spk_embed_dim) fail("stream_set: speaker id out of range");
  }
  if (pitch)
    for (int s = 0; s < se.S; ++s)
      if (!std::isfinite(pitch[s])) fail("stream_set: pitch is not finite");
  if (!std::isnan(index_rate) && index_rate != 0.f && C->index && C->index->dim != se.E)
    fail("stream_set: the resident index holds " + std::to_string(C->index->dim) + "-wide vectors, the voice model takes " +
         std::to_string(se.E) + "-wide features");
  // every check has passed: nothing below can fail
  if (sid) se.sid.assign(sid, sid + se.S);
  if (pitch) se.pitch.assign(pitch, pitch + se.S);
  if (!std::isnan(index_rate)) se.p.index_rate = index_rate;
  if (!std::isnan(protect)) se.p.protect = protect;
  API_END
}

int rvcx_op_stream_resample(rvcx_ctx* ctx, const float* x, int S, int64_t frames, int channels, int sr_in, int sr_out,
                            int block_frames, float* y) {
  API_BEGIN(ctx)
  if (channels < 1) fail("op_stream_resample: channels >= 1");
  if (S < 1 || frames < 1 || block_frames < 1) fail("op_stream_resample: S, frames and block_frames >= 1");
  if (!x || !y) fail("op_stream_resample: null argument");
  if (!stream_rates_ok(sr_in, sr_out)) fail(std::string("op_stream_resample: each rate") + kRateRule);
  const StreamResamplerPlan g = stream_resampler_plan(sr_in, sr_out, channels, block_frames);
  if (frames % g.B_in != 0)
    fail("op_stream_resample: frames must be a multiple of the block, block_frames * sr_in / 100 = " + std::to_string(g.B_in));
  const long K = (long)(frames / g.B_in), n_out = K * g.B_out;
  const size_t nx = (size_t)S * frames * channels, ny = (size_t)S * n_out, nf = (size_t)S * g.L;
  if (nx > ((size_t)1 << 31) || ny > ((size_t)1 << 31)) fail("op_stream_resample: more than 2^31 samples");
  C->arena.reserve((nx + ny) * 4 + (2 * nf + resample_table_doubles(0)) * sizeof(double) + (1 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  double* fifo[2] = {nullptr, nullptr};
  ResampleFilter f;
  if (g.filter) {
    for (double*& q : fifo) {
      q = C->arena.alloc<double>(nf);
      RVCX_HIP(hipMemsetAsync(q, 0, nf * sizeof(double), s));
    }
    f = make_resample_filter(C->arena, sr_in, sr_out, s, 0);
  }
  for (long k = 0; k < K; ++k)       // exactly a session's steps: set k & 1 is read, the other one written
    launch_stream_resample(g, f, fifo[k & 1], fifo[(k & 1) ^ 1], dx + (size_t)k * g.B_in * channels, (long)(frames * channels),
                           dy + (size_t)k * g.B_out, n_out, S, (uint64_t)k, s);
  RVCX_HIP(hipMemcpyAsync(y, dy, ny * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->arena.reset();
  API_END
}

}  // extern "C"
