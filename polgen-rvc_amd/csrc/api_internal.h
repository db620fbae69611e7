// What the api*.hip files share: the context handle, the per-call wrapper (api_call) and a few small helpers.
#pragma once
#include "../../include/rvcx.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <unordered_map>

#include "ctx.h"
#include "denoise_live.h"
#include "effects.h"
#include "formant_live.h"
#include "layers.h"
#include "models.h"
#include "ops.h"
#include "pipeline.h"

// everything here but the handle itself (the C ABI names `struct rvcx_ctx`) lives in rvcx::api
namespace rvcx {
namespace api {

// One context = one set of streams, arenas and resident models.  The reference builds fresh model objects for every
// request (rvc/scripts/voice_conversion.py:71-100), so two Gradio worker threads never share state there; here every
// thread of a process shares the one resident context (infer/_state.py) and ctypes releases the GIL -- so every entry
// point takes the context's mutex (recursive: an entry point may call another).  Calls on one context QUEUE; throughput
// comes from rvcx_convert_batch (one call, many utterances), not from threads.  Different contexts stay concurrent.
// A conversion ticket (rvcx_convert_submit): the enqueue half of a conversion has run, the finish half runs when somebody
// waits for it (or when something else needs the context to itself).  It owns copies of the small host-side arguments; the
// audio, noise, dither and output buffers stay the caller's.
struct Ticket {
  rvcx_ticket id = 0;
  enum State { InFlight, Done, Failed } state = InFlight;
  std::string error;
  int model_id = 0;
  rvcx_params p;
  std::vector<UttIO> ios;
  std::vector<std::vector<float>> f0_rows;    // the f0-file tables `extra` pointed to
  std::vector<int64_t> n_out;                 // produced samples per utterance (what out_n receives)
  int64_t* out_n = nullptr;
  bool inject_gru = false;                    // rvcx_debug_inject(1) was pending when the ticket was submitted: it is this ticket's
  bool timing = false;
  float ms[9] = {0};
  TicketIO io;
  ConvertStatePtr st;
  bool enqueued = false;                      // ev_first / ev_done were recorded
  std::shared_ptr<Ticket> prev;               // the ticket in flight in front of this one at submit time (lead_ms)
  float lead_ms = 0.f;
  std::vector<int> mbs;
  std::vector<std::vector<long>> cuts;
  ~Ticket() {
    st.reset();
    if (io.ev_first) (void)hipEventDestroy(io.ev_first);
    if (io.ev_done) (void)hipEventDestroy(io.ev_done);
  }
};
using TicketPtr = std::shared_ptr<Ticket>;

// what one call runs: the chain fills all of it from rvcx_fx_params, a stage-level entry point one stage
struct FxPlan {
  int sr = 0, C = 0;
  bool low_rate = false;            // live sessions of reduced-size voice models: 3200 .. 7900 Hz too
  bool hp = false, comp = false, gate = false, reverb = false, lo = false, hi = false, chorus = false;
  double hp_fc = 50.0;
  double comp_ratio = 1.0, comp_thr_db = 0.0, comp_att = 1.0, comp_rel = 100.0;
  double gate_thr_db = 0.0, gate_ratio = 1.0, gate_att = 0.0, gate_rel = 0.0;
  double room = 0.0, damp = 0.0, wet = 0.0, dry = 0.0, width = 0.0;
  double lo_db = 0.0, hi_db = 0.0, lo_fc = 440.0, hi_fc = 440.0, lo_q = M_SQRT1_2, hi_q = M_SQRT1_2;
  double rate = 0.0, depth = 0.0, centre = 0.0, fb = 0.0, mix = 0.0;
};
// every refusal of a plan, before anything is written (api_fx.hip)
void fx_validate(const char* who, const FxPlan& P);
// the whole board from the eighteen add_effects values: validated with every stage on, identities switched off
FxPlan fx_board_plan(const char* who, const rvcx_fx_params& p, int sr, int channels, bool low_rate);


// A live-stream session (rvcx_stream_open): S lock-step streams of one geometry on one voice model.  Ring, carry and block
// staging are allocations of the session's own (the arena is scratch that other calls reset).  Ring and carry exist twice: a
// step reads set `cur` and writes the other one, and the sets change places once the step has succeeded -- the body of a step
// can then be repeated (range guard, BiGRU fallback) or fail without moving the session.  The same holds for the FIFOs of the
// two resamplers of a session opened with rvcx_stream_open_io, for the dense blocks and for the native tap.
//
// One side of such a session (audio.hip, launch_stream_resample): plan, filter and the FIFO sets.  The tables are the
// session's own device memory (built at open: make_resample_filter_at synchronises); two sides of one gain share them.
struct StreamSide {
  bool on = false;                         // false: that side is rvcx_stream_open's path
  StreamResamplerPlan g;
  ResampleFilter f;
  double* fifo[2] = {nullptr, nullptr};    // (S, g.L) each; only when g.filter
};
struct StreamSession {
  int model_id = 0;
  std::weak_ptr<WeightRegion> region;      // expires when the voice model is unloaded (or replaced)
  rvcx_stream_cfg cfg{};
  rvcx_params p{};
  std::vector<int> sid;
  std::vector<float> pitch;
  int S = 0, N = 0, Th = 0, T = 0, head = 0, upp = 0, inter = 0, E = 0;
  long Lb = 0, Lx = 0, Ls = 0, Lk = 0;     // block, cross-fade, search and synthesized tail in output samples
  float* ring[2] = {nullptr, nullptr};     // (S, N * 160) each
  float* carry[2] = {nullptr, nullptr};    // (S, Lx) each
  float* blocks[2] = {nullptr, nullptr};   // (S, Fb * 160) each: the step's new 16 kHz blocks, dense (set cur: the last step's)
  rvcx_stream_io io{};
  StreamSide in, out;                      // in: in_rate x in_channels -> 16 kHz mono; out: the model's rate -> out_rate
  float* stage = nullptr;                  // in.on: (S, in.g.B_in * channels), the caller's blocks as they came
  float* native[2] = {nullptr, nullptr};   // out.on: (S, Lb) each, SOLA output in front of the output resampler
  double* tables[2] = {nullptr, nullptr};  // filter tables of the sides that filter (one allocation when they share a gain)
  int cur = 0;
  uint64_t step = 0;
  // RVCX_STREAM_FULL_SYNTH=1 (read at open; tools/bench_stream.py's A/B): the synthesizer runs with skip_head = 0 and SOLA takes
  // the tail of the whole output -- what the step costs without the tail-only path (and NOT what the reference computes)
  bool full_synth = false;
  // the effects board behind the output resampler (rvcx_stream_open_fx; rvcx.h "live post-production"): its state sets change
  // places with everything else, its memory is the session's own
  std::unique_ptr<FxLive> fx;
  rvcx_fx_params fxp{};                    // the parameters in force
  float* fx_out = nullptr;                 // (S, block, 2): what the step copies out
  float fx_ms[8] = {0};                    // rvcx_stream_last_fx_ms
  // live noise reduction (rvcx_stream_open_dn; rvcx.h stage 16): side 0 on the 16 kHz block in front of the ring, side 1 behind
  // the output resampler in front of the board.  State sets as above; tables, profile and staging are the session's own
  struct DnSide {
    std::unique_ptr<DnLive> d;             // null: the side is absent
    rvcx_live_denoise_params p{};          // the parameters in force
    float* tables = nullptr;               // w (N floats), then the twiddles (N / 2 pairs)
    double* prof = nullptr;                // mode 0 at open: mu, then sd (nb doubles each)
    float* stage = nullptr;                // (S, B): side 0, the block as it came; side 1, what the side emits
    hipEvent_t ev[2] = {nullptr, nullptr};
  } dn[2];
  float dn_ms[2] = {0, 0};                 // rvcx_stream_last_dn_ms
  // live formant shift (rvcx_stream_open_fm; rvcx.h stage 19): side 0 behind the input noise gate in front of the ring, side 1
  // behind the output noise gate in front of the board.  State sets as above; tables, scratch and staging are the session's own
  struct FmSide {
    std::unique_ptr<FmLive> d;             // null: the side is absent
    rvcx_live_formant_params p{};          // the parameters in force
    float* tables = nullptr;               // w (N floats), then the twiddles (N / 2 pairs)
    float* stage = nullptr;                // (S, B): side 0, the block in front of the stage; side 1, what the side emits
    hipEvent_t ev[2] = {nullptr, nullptr};
  } fm[2];
  float fm_ms[2] = {0, 0};                 // rvcx_stream_last_fm_ms
  ~StreamSession() {
    for (FmSide& sd : fm) {
      if (sd.d)
        for (void* q : {(void*)sd.d->state[0], (void*)sd.d->state[1], (void*)sd.d->fr})
          if (q) (void)hipFree(q);
      for (void* q : {(void*)sd.tables, (void*)sd.stage})
        if (q) (void)hipFree(q);
      for (hipEvent_t e : sd.ev)
        if (e) (void)hipEventDestroy(e);
    }
    for (DnSide& sd : dn) {
      if (sd.d)
        for (void* q : {(void*)sd.d->state[0], (void*)sd.d->state[1], (void*)sd.d->acc})
          if (q) (void)hipFree(q);
      for (void* q : {(void*)sd.tables, (void*)sd.prof, (void*)sd.stage})
        if (q) (void)hipFree(q);
      for (hipEvent_t e : sd.ev)
        if (e) (void)hipEventDestroy(e);
    }
    if (fx)
      for (void* q : {(void*)fx->state[0], (void*)fx->state[1], (void*)fx->work, (void*)fx_out})
        if (q) (void)hipFree(q);
    for (void* q : {(void*)ring[0], (void*)ring[1], (void*)carry[0], (void*)carry[1], (void*)blocks[0], (void*)blocks[1],
                    (void*)stage, (void*)native[0], (void*)native[1], (void*)tables[0], (void*)tables[1], (void*)in.fifo[0],
                    (void*)in.fifo[1], (void*)out.fifo[0], (void*)out.fifo[1]})
      if (q) (void)hipFree(q);
  }
};

}  // namespace api
}  // namespace rvcx

struct rvcx_ctx {
  rvcx::Ctx c;
  std::unordered_map<int, std::unique_ptr<rvcx::api::StreamSession>> sessions;
  int next_session = 1;
  std::recursive_mutex mu;
  std::deque<rvcx::api::TicketPtr> inflight;                          // submit order; at most two
  std::unordered_map<rvcx_ticket, rvcx::api::TicketPtr> tickets;      // every ticket that has not been waited for
  std::deque<std::pair<rvcx_ticket, float>> leads;         // lead_ms of the tickets waited for last
  int fx_passes[3] = {0, 0, 0};   // rvcx_fx_last_passes: relaxation passes of the last post-production call's followers
  int fx_groups = 0;              // and the groups it ran in
  rvcx::Arena load_arena;     // rvcx_resample_f64* with tickets in flight: a buffer nobody else uses (see there)
};
namespace rvcx {
namespace api {

using CtxLock = std::unique_lock<std::recursive_mutex>;
inline CtxLock lock_ctx(rvcx_ctx* h) { return h ? CtxLock(h->mu) : CtxLock(); }

inline thread_local std::string g_last_error;

// Every entry point's body runs inside api_call():
//  * fp16-split range guard.  If a split-fp16 kernel reported an activation it could not represent
//    (Ctx::take_overflow), the FIRST offending layer of the call (launch order; every layer stamps its own device
//    word) is pinned to the exact-fp32 kernels for the life of its model and the call is repeated -- a one-off per
//    model and layer (rvcx_fp32_reruns counts the repeats, rvcx_fp32_layers the pinned layers).  If no layer can be
//    named (kernel-level test entry points pack their weights per call) or after kMaxAttempts - 1 repeats, the last
//    attempt runs everything on the exact-fp32 kernels (thread-local g_force_fp32).
//  * BiGRU cluster time-out.  The cluster kernel needs its workgroups co-resident; if a partner never showed up
//    (Ctx::check_dev_err -> GruTimeout) the call is repeated once with the single-workgroup GRU kernel.
// Bodies are written to be repeatable (they reset the arena first); load / unload entry points run once (repeat = false).
struct Fp32Scope {
  bool saved;
  explicit Fp32Scope(bool on) : saved(g_force_fp32) { g_force_fp32 = saved || on; }
  ~Fp32Scope() { g_force_fp32 = saved; }
};
struct GruScope {
  bool saved;
  explicit GruScope(bool on) : saved(g_gru_no_cluster) { g_gru_no_cluster = saved || on; }
  ~GruScope() { g_gru_no_cluster = saved; }
};
constexpr int kMaxAttempts = 6;

// every weight region of the context in a fixed order (api.hip)
std::vector<WeightRegion*> all_regions(Ctx& c, uint64_t* hash);
// pins the first layer (in launch order) whose activations left fp16 range; false: none of the resident models named one
bool localize_overflow(Ctx& c);
void reset_after_failure(Ctx& c);
// completes every ticket in flight, oldest first (api_convert.hip)
void drain_tickets(rvcx_ctx* h);

// the attempts of one call (see above); gru_plain: start on the single-workgroup GRU kernel (a ticket's re-run)
template <typename F>
void run_attempts(Ctx* C, bool repeat, bool gru_plain, F&& body) {
  {
    const int last = repeat ? kMaxAttempts - 1 : 0;
    for (int attempt = 0; attempt <= last; ++attempt) {
      Fp32Scope fp32_scope(attempt > 0 && attempt == last);
      GruScope gru_scope(gru_plain);
      C->launch_seq = 0;
      C->err_snapshot = false;
      try {
        body(C);
      } catch (const GruTimeout&) {
        if (!repeat || gru_plain) throw;
        gru_plain = true;
        C->gru_fallbacks++;
        reset_after_failure(*C);
        --attempt;
        continue;
      }
      if (attempt < last && C->take_overflow()) {
        C->fp32_reruns++;
        if (!localize_overflow(*C)) attempt = last - 1;     // nobody to pin: everything on fp32 next
        continue;
      }
      if (attempt > 0 && attempt == last) (void)C->take_overflow();   // producers of split tensors may have re-raised the bit
      break;
    }
  }
}

template <typename F>
int api_call(rvcx_ctx* ctxp, bool repeat, F&& body, bool drain = true) {
  Ctx* C = ctxp ? &ctxp->c : nullptr;
  CtxLock guard = lock_ctx(ctxp);
  try {
    if (!C) fail("null context");
    RVCX_HIP(hipSetDevice(C->device));
    // every entry point has the context to itself: tickets in flight complete first (they stay waitable).  The one
    // exception is rvcx_resample_f64*, which brings its own memory and stream order (drain = false)
    if (drain) drain_tickets(ctxp);
    if (!repeat) C->arena_budget = 0;     // loads / unloads change what is free: convert_micro_batch probes again
    run_attempts(C, repeat, false, body);
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    if (C) {
      C->last_error = e.what();
      reset_after_failure(*C);
    }
    (void)hipGetLastError();
    return -1;
  }
}

// the session of an id, or a failure (api_stream.hip)
StreamSession& get_session(rvcx_ctx* h, int id);

// Tuning / fault-injection hooks (rvcx_conv_override, rvcx_debug_inject, rvcx_bench_*) are process-wide levers a serving
// process must never meet by accident: they are refused (-2) unless the process was started with RVCX_DEBUG=1
// (read once; tests/conftest.py and tools/ set it).
bool debug_hooks_enabled();
#define REQUIRE_DEBUG(ctxp, name)                                                             \
  if (!debug_hooks_enabled()) {                                                               \
    g_last_error = name ": debug / tuning hook refused (start the process with RVCX_DEBUG=1)"; \
    if ((ctxp) != nullptr) {                                                                  \
      CtxLock dbg_guard_ = lock_ctx((rvcx_ctx*)(ctxp));                                       \
      ((rvcx_ctx*)(ctxp))->c.last_error = g_last_error;                                       \
    }                                                                                         \
    return -2;                                                                                \
  }

#define API_BEGIN(ctxp) return api_call((ctxp), true, [&](Ctx* C) {
#define API_BEGIN_ONCE(ctxp) return api_call((ctxp), false, [&](Ctx* C) {
#define API_END });

// copy n elements from host or device memory into the arena
template <typename T>
T* to_dev(Ctx& c, const T* p, size_t n) {
  T* d = c.arena.alloc<T>(n);
  RVCX_HIP(hipMemcpyAsync(d, p, n * sizeof(T), hipMemcpyDefault, c.stream));
  return d;
}

// one row of Gaussian noise: the caller's own values (parity runs), or Philox(seed) from `counter` on
inline void fill_noise(float* dst, const float* given, size_t n, uint64_t seed, uint64_t counter, hipStream_t s) {
  if (given) RVCX_HIP(hipMemcpyAsync(dst, given, n * sizeof(float), hipMemcpyDefault, s));
  else launch_randn(dst, n, seed, counter, s);
}

inline SynthModel& get_synth(Ctx& c, int id) {
  if (id < 0 || id >= (int)c.synths.size() || !c.synths[id]) fail("synth model not loaded");
  return *c.synths[id];
}

}  // namespace api
}  // namespace rvcx
