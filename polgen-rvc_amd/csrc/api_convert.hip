// C ABI of librvcx.so (include/rvcx.h): whole conversions -- synchronous calls and tickets.
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

// ticket numbers are unique in the process: a ticket of another context is simply unknown here
static std::atomic<int64_t> g_next_ticket{1};

static bool stage_timing_on() {
  static const bool timing = !getenv("RVCX_STAGE_TIMING") || atoi(getenv("RVCX_STAGE_TIMING")) != 0;
  return timing;
}

// one attempt of a synchronous conversion (the body api_call repeats)
static void convert_run(Ctx* C, int model_id, std::vector<UttIO>& ios, const rvcx_params& p, int64_t* out_n) {
  float ms[9] = {0};
  convert_batch(*C, model_id, ios, p, stage_timing_on() ? ms : nullptr);
  C->check_dev_err();
  for (int k = 0; k < 9; ++k) C->timing[k] = ms[k];
  if (out_n)
    for (size_t i = 0; i < ios.size(); ++i) out_n[i] = ios[i].out_n;
  C->arena.reset();
}

static void fill_ios(std::vector<UttIO>& ios, int B, const float* const* wav32, const double* const* wav64,
                     const int64_t* n, const rvcx_params* p, const float* const* noise, int16_t* const* out,
                     float* const* out_f32, const rvcx_utt_extra* extra) {
  if (B < 0 || (B > 0 && (!n || !p || !out || (!wav32 && !wav64)))) fail("convert_batch: null argument");
  ios.assign((size_t)B, UttIO());
  for (int i = 0; i < B; ++i) {
    UttIO& u = ios[i];
    u.wav = wav32 ? wav32[i] : nullptr;
    u.wav64 = wav64 ? wav64[i] : nullptr;
    u.n = n[i];
    u.noise = noise ? noise[i] : nullptr;
    u.out = out[i];
    u.out_f32 = out_f32 ? out_f32[i] : nullptr;
    u.seed_offset = i;
    if (extra) {
      u.inp_f0 = extra[i].inp_f0;
      u.inp_f0_rows = extra[i].inp_f0 ? extra[i].inp_f0_rows : 0;
      u.crepe_dither = extra[i].crepe_dither;
      u.crepe_dither_n = extra[i].crepe_dither ? extra[i].crepe_dither_n : 0;
    }
    if (!(u.wav || u.wav64) || !u.out) fail("convert_batch: null buffer for utterance " + std::to_string(i));
  }
}

static int convert_impl(rvcx_ctx* ctx, int model_id, int B, const float* const* wav32, const double* const* wav64,
                        const int64_t* n, const rvcx_params* p, const float* const* noise, int16_t* const* out,
                        float* const* out_f32, int64_t* out_n, const rvcx_utt_extra* extra = nullptr) {
  API_BEGIN(ctx)
  (void)get_synth(*C, model_id);
  std::vector<UttIO> ios;
  fill_ios(ios, B, wav32, wav64, n, p, noise, out, out_f32, extra);
  convert_run(C, model_id, ios, *p, out_n);
  API_END
}

// ------------------------------------------------------------------------------------------
// conversion tickets: two requests in flight per context
// ------------------------------------------------------------------------------------------
// submit = the enqueue half of a conversion on the calling thread, wait = its finish half.  The second ticket's front end
// (upload, high-pass, F0 model, HuBERT) runs on the front / HuBERT streams while the first is in its synthesizer on the main
// stream, exactly as micro-batch k + 1 of one call does; tickets of different voice models or parameters take the same
// path (nothing in the overlap depends on them being equal).  Completions are processed in submit order.

// launches and error-word readers use this word for as long as the scope lives
struct ErrWordScope {
  Ctx& c;
  int *d, *h;
  ErrWordScope(Ctx& cc, int* dev, int* host) : c(cc), d(cc.dev_err), h(cc.err_host) {
    c.dev_err = dev;
    c.err_host = host;
  }
  ~ErrWordScope() {
    c.dev_err = d;
    c.err_host = h;
  }
};

// the oldest ticket in flight: wait for the device, then either take its results or -- range guard, BiGRU time-out --
// repeat it (and what depends on it) the way the same requests would have run as synchronous calls in submit order
static void settle_oldest(rvcx_ctx* h) {
  Ctx& c = h->c;
  TicketPtr T = h->inflight.front();
  RVCX_HIP(hipSetDevice(c.device));
  if (T->st) RVCX_HIP(hipEventSynchronize(T->io.ev_done));
  if (T->prev) {
    if (T->enqueued && T->prev->enqueued) (void)hipEventElapsedTime(&T->lead_ms, T->io.ev_first, T->prev->io.ev_done);
    (void)hipGetLastError();
    T->prev.reset();
  }
  int v = T->st ? *c.slot[T->io.slot].err_host : 0;
  if (T->inject_gru) v |= kErrGruTimeout;
  if (!(v & (kErrGruTimeout | kErrH3Overflow))) {
    h->inflight.pop_front();
    try {
      if (T->st) {
        convert_finish(c, *T->st, T->timing ? T->ms : nullptr);
        const char* stage = c.slot[T->io.slot].stage;
        for (const auto& sg : T->io.staged) memcpy(sg.dst, stage + sg.off, sg.bytes);
        T->mbs = convert_state_mbs(*T->st);
        T->cuts = convert_state_cuts(*T->st);
      }
      for (size_t i = 0; i < T->ios.size(); ++i) T->n_out[i] = T->ios[i].out_n;
      if (T->out_n)
        for (size_t i = 0; i < T->ios.size(); ++i) T->out_n[i] = T->n_out[i];
      T->state = Ticket::Done;
    } catch (const std::exception& e) {
      T->state = Ticket::Failed;
      T->error = e.what();
    }
    T->st.reset();
    if (h->inflight.empty()) c.arena.reset();     // the work area is nobody's now (a synchronous call may grow the arena)
    return;
  }
  // Everything in flight completes; then the affected tickets run again through the synchronous path, oldest first.  An
  // overflow pins a layer, and a pin changes which kernels later requests run on: every later ticket was enqueued before
  // the pin and is repeated as well, whatever its own word says.  A BiGRU time-out changes no lasting state: this ticket only.
  RVCX_HIP(hipDeviceSynchronize());
  std::vector<TicketPtr> redo{T};
  if (v & kErrH3Overflow)
    for (size_t i = 1; i < h->inflight.size(); ++i) redo.push_back(h->inflight[i]);
  for (WeightRegion* r : all_regions(c, nullptr)) r->clear_overflow();    // the layers' stamp words are shared by both tickets
  ErrWordScope words(c, c.err_words, c.err_words_host);
  const bool pending_inject = c.inject_gru_timeout;     // belongs to the NEXT request (a submit that is settling us first)
  for (const TicketPtr& R : redo) {
    for (auto it = h->inflight.begin(); it != h->inflight.end(); ++it)
      if (*it == R) {
        h->inflight.erase(it);
        break;
      }
    if (R->st) RVCX_HIP(hipMemset(c.slot[R->io.slot].err, 0, sizeof(int)));
    R->st.reset();
    R->prev.reset();
    const bool plain = R == T && (v & kErrGruTimeout);
    c.inject_gru_timeout = R != T && R->inject_gru;     // a later ticket's own injected time-out: its repeat meets it
    if (plain) c.gru_fallbacks++;
    try {
      run_attempts(&c, true, plain, [&](Ctx* C) { convert_run(C, R->model_id, R->ios, R->p, R->out_n); });
      for (size_t i = 0; i < R->ios.size(); ++i) R->n_out[i] = R->ios[i].out_n;
      R->mbs = c.last_mbs;
      R->cuts = c.last_cuts;
      for (int k = 0; k < 9; ++k) R->ms[k] = c.timing[k];
      R->state = Ticket::Done;
    } catch (const std::exception& e) {
      R->state = Ticket::Failed;
      R->error = e.what();
      reset_after_failure(c);
      (void)hipGetLastError();
    }
  }
  c.inject_gru_timeout = pending_inject;
}

void rvcx::api::drain_tickets(rvcx_ctx* h) {
  while (h && !h->inflight.empty()) settle_oldest(h);
}

static int ticket_error(rvcx_ctx* ctx, const std::string& what) {
  g_last_error = what;
  if (ctx) ctx->c.last_error = what;
  return -1;
}

extern "C" {

int64_t rvcx_out_len(rvcx_ctx* ctx, int model_id, int64_t n, const rvcx_params* p) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || model_id < 0 || model_id >= (int)ctx->c.synths.size() || !ctx->c.synths[model_id]) return -1;
  return out_capacity(*ctx->c.synths[model_id], n, *p);
}

int64_t rvcx_noise_len(rvcx_ctx* ctx, int model_id, int64_t n, const rvcx_params* p) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || model_id < 0 || model_id >= (int)ctx->c.synths.size() || !ctx->c.synths[model_id]) return -1;
  return noise_len_for(ctx->c, *ctx->c.synths[model_id], n, *p);
}

int rvcx_convert_batch(rvcx_ctx* ctx, int model_id, int B, const float* const* wav16k, const int64_t* n,
                       const rvcx_params* p, const float* const* noise, int16_t* const* out, float* const* out_f32,
                       int64_t* out_n) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return convert_impl(ctx, model_id, B, wav16k, nullptr, n, p, noise, out, out_f32, out_n);
}

int rvcx_convert_batch_f64(rvcx_ctx* ctx, int model_id, int B, const double* const* wav16k, const int64_t* n,
                           const rvcx_params* p, const float* const* noise, int16_t* const* out,
                           float* const* out_f32, int64_t* out_n) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return convert_impl(ctx, model_id, B, nullptr, wav16k, n, p, noise, out, out_f32, out_n);
}

int rvcx_convert_batch_ex(rvcx_ctx* ctx, int model_id, int B, const void* const* wav16k, int wav_is_f64,
                          const int64_t* n, const rvcx_params* p, const float* const* noise,
                          const rvcx_utt_extra* extra, int16_t* const* out, float* const* out_f32, int64_t* out_n) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return convert_impl(ctx, model_id, B, wav_is_f64 ? nullptr : reinterpret_cast<const float* const*>(wav16k),
                      wav_is_f64 ? reinterpret_cast<const double* const*>(wav16k) : nullptr, n, p, noise, out, out_f32,
                      out_n, extra);
}

int rvcx_convert_submit(rvcx_ctx* ctx, int model_id, int B, const void* const* wav16k, int wav_is_f64, const int64_t* n,
                        const rvcx_params* p, const float* const* noise, const rvcx_utt_extra* extra, int16_t* const* out,
                        float* const* out_f32, int64_t* out_n, rvcx_ticket* ticket) {
  CtxLock guard = lock_ctx(ctx);
  if (!ctx) return ticket_error(nullptr, "null context");
  Ctx& c = ctx->c;
  bool inject = false;
  int slot = -1;
  try {
    if (!ticket) fail("convert_submit: null ticket pointer");
    RVCX_HIP(hipSetDevice(c.device));
    (void)get_synth(c, model_id);
    TicketPtr T = std::make_shared<Ticket>();
    fill_ios(T->ios, B, wav_is_f64 ? nullptr : reinterpret_cast<const float* const*>(wav16k),
             wav_is_f64 ? reinterpret_cast<const double* const*>(wav16k) : nullptr, n, p, noise, out, out_f32, extra);
    T->f0_rows.resize((size_t)B);
    for (int i = 0; i < B; ++i)
      if (T->ios[i].inp_f0 && T->ios[i].inp_f0_rows > 0) {      // the f0-file rows are copied; the big buffers are borrowed
        T->f0_rows[i].assign(T->ios[i].inp_f0, T->ios[i].inp_f0 + 2 * (size_t)T->ios[i].inp_f0_rows);
        T->ios[i].inp_f0 = T->f0_rows[i].data();
      }
    T->model_id = model_id;
    T->p = *p;
    T->out_n = out_n;
    T->n_out.assign((size_t)B, 0);
    T->timing = stage_timing_on();
    // two front sets, two event sets, two slots: a third ticket first completes the oldest one (it stays waitable)
    while (ctx->inflight.size() >= 2) settle_oldest(ctx);
    T->io.slot = ctx->inflight.empty() ? 0 : 1 - ctx->inflight.back()->io.slot;
    T->io.beside_predecessor = !ctx->inflight.empty();
    if (!ctx->inflight.empty()) T->prev = ctx->inflight.back();
    T->io.drain = [ctx] { drain_tickets(ctx); };
    RVCX_HIP(hipEventCreate(&T->io.ev_first));
    RVCX_HIP(hipEventCreate(&T->io.ev_done));
    inject = c.inject_gru_timeout;
    T->inject_gru = inject;
    c.inject_gru_timeout = false;
    {
      Ctx::TicketSlot& sl = c.slot[T->io.slot];
      slot = T->io.slot;
      ErrWordScope words(c, sl.err, sl.err_host);
      c.launch_seq = 0;
      c.err_snapshot = false;
      *sl.err_host = 0;
      T->st = convert_enqueue(c, model_id, T->ios, T->p, T->timing, &T->io);
      T->enqueued = T->st != nullptr;
    }
    T->id = g_next_ticket.fetch_add(1);
    ctx->inflight.push_back(T);
    ctx->tickets[T->id] = T;
    *ticket = T->id;
    return 0;
  } catch (const std::exception& e) {
    // whatever was enqueued for the failed ticket runs out (reset_after_failure waits for the device); a ticket already
    // in flight keeps its slot and is settled by its own wait
    c.inject_gru_timeout = c.inject_gru_timeout || inject;
    ticket_error(ctx, e.what());
    reset_after_failure(c);
    // launches of the failed ticket may have raised the slot's word: the next ticket of that slot must not inherit it
    if (slot >= 0) (void)hipMemset(c.slot[slot].err, 0, sizeof(int));
    (void)hipGetLastError();
    return -1;
  }
}

int rvcx_convert_wait(rvcx_ctx* ctx, rvcx_ticket t) {
  CtxLock guard = lock_ctx(ctx);
  if (!ctx) return ticket_error(nullptr, "null context");
  static const char* kUnknown = "convert_wait: unknown ticket (already waited for, or a ticket of another context)";
  try {
    auto it = ctx->tickets.find(t);
    if (it == ctx->tickets.end()) return ticket_error(ctx, kUnknown);
    TicketPtr T = it->second;
    if (T->state == Ticket::InFlight && T->st) {
      // block on the device WITHOUT the context's mutex: another thread's submit must be able to fill the pipeline
      hipEvent_t ev = T->io.ev_done;
      guard.unlock();
      (void)hipSetDevice(ctx->c.device);
      const hipError_t rc = hipEventSynchronize(ev);
      guard.lock();
      if (rc != hipSuccess) fail(std::string("convert_wait: ") + hipGetErrorString(rc));
    }
    it = ctx->tickets.find(t);
    if (it == ctx->tickets.end()) return ticket_error(ctx, kUnknown);   // another thread waited for it meanwhile
    while (T->state == Ticket::InFlight) {        // completions settle in submit order: everything older goes first
      if (ctx->inflight.empty()) fail("internal: a ticket in flight is not in the list");
      settle_oldest(ctx);
    }
    ctx->tickets.erase(it);
    Ctx& c = ctx->c;
    c.last_mbs = T->mbs;
    c.last_cuts = T->cuts;
    for (int k = 0; k < 9; ++k) c.timing[k] = T->ms[k];
    ctx->leads.emplace_back(T->id, T->lead_ms);
    if (ctx->leads.size() > 256) ctx->leads.pop_front();
    if (T->state == Ticket::Failed) return ticket_error(ctx, T->error);
    return 0;
  } catch (const std::exception& e) {
    return ticket_error(ctx, e.what());
  }
}

int rvcx_convert_poll(rvcx_ctx* ctx, rvcx_ticket t) {
  CtxLock guard = lock_ctx(ctx);
  if (!ctx) return ticket_error(nullptr, "null context");
  auto it = ctx->tickets.find(t);
  if (it == ctx->tickets.end()) return ticket_error(ctx, "convert_poll: unknown ticket");
  const Ticket& T = *it->second;
  if (T.state != Ticket::InFlight || !T.st) return 1;
  (void)hipSetDevice(ctx->c.device);
  const hipError_t rc = hipEventQuery(T.io.ev_done);
  if (rc == hipSuccess) return 1;
  (void)hipGetLastError();
  return rc == hipErrorNotReady ? 0 : ticket_error(ctx, std::string("convert_poll: ") + hipGetErrorString(rc));
}

int rvcx_convert_inflight(rvcx_ctx* ctx) {
  CtxLock guard = lock_ctx(ctx);
  if (!ctx) return -1;
  (void)hipSetDevice(ctx->c.device);
  int k = 0;
  for (const TicketPtr& T : ctx->inflight)
    if (T->st && hipEventQuery(T->io.ev_done) != hipSuccess) ++k;
  (void)hipGetLastError();
  return k;
}

float rvcx_ticket_lead_ms(rvcx_ctx* ctx, rvcx_ticket t) {
  CtxLock guard = lock_ctx(ctx);
  if (!ctx) return NAN;
  for (auto it = ctx->leads.rbegin(); it != ctx->leads.rend(); ++it)
    if (it->first == t) return it->second;
  return NAN;
}

int rvcx_micro_batch(rvcx_ctx* ctx, int model_id, int64_t n, const rvcx_params* p) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !p || model_id < 0 || model_id >= (int)ctx->c.synths.size() || !ctx->c.synths[model_id] ||
      !ctx->c.hubert)
    return -1;
  try {
    return convert_micro_batch(ctx->c, model_id, n, *p);
  } catch (const std::exception& e) {
    ctx->c.last_error = e.what();
    return -1;
  }
}

int64_t rvcx_bucket_length(rvcx_ctx* ctx, int model_id, int64_t n, const rvcx_params* p) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !p || model_id < 0 || model_id >= (int)ctx->c.synths.size() || !ctx->c.synths[model_id]) return -1;
  try {
    return bucket_length(n, *p, make_geometry(*p, ctx->c.synths[model_id]->cfg.sr));
  } catch (const std::exception& e) {
    ctx->c.last_error = e.what();
    return -1;
  }
}

int rvcx_last_micro_batches(rvcx_ctx* ctx, int32_t* counts, int cap) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  const auto& v = ctx->c.last_mbs;
  for (int i = 0; i < (int)v.size() && i < cap && counts; ++i) counts[i] = v[i];
  return (int)v.size();
}

int64_t rvcx_last_cuts(rvcx_ctx* ctx, int64_t* out, int64_t cap) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  int64_t k = 0;
  auto put = [&](int64_t v) {
    if (out && k < cap) out[k] = v;
    ++k;
  };
  for (const auto& cuts : ctx->c.last_cuts) {
    put((int64_t)cuts.size());
    for (long t : cuts) put(t);
  }
  return k;
}

}  // extern "C"
