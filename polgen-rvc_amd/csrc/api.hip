// C ABI of librvcx.so (include/rvcx.h): context lifecycle, counters and debug hooks, model loading, weight regions.  Nothing throws
// across this boundary.
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

bool rvcx::api::localize_overflow(Ctx& c) {
  WeightRegion* best_r = nullptr;
  int best = 0, best_i = -1;
  for (WeightRegion* r : all_regions(c, nullptr)) {
    int i = -1;
    const int v = r->first_overflow(&i);       // also clears the region's words
    if (v > best) {
      best = v;
      best_i = i;
      best_r = r;
    }
  }
  if (!best_r) return false;
  best_r->drop_flag(best_i);
  return true;
}

void rvcx::api::reset_after_failure(Ctx& c) {
  (void)hipDeviceSynchronize();    // side streams may still use arena memory
  c.arena.reset();
  c.arena_f0.reset();
  c.arena_hub.reset();
}

// RVCX_DEBUG=1, read once (REQUIRE_DEBUG)
bool rvcx::api::debug_hooks_enabled() {
  static const bool on = [] {
    const char* e = getenv("RVCX_DEBUG");
    return e && atoi(e) != 0;
  }();
  return on;
}

// every weight region of the context in a fixed order: HuBERT, RMVPE, FCPE, voice models by id, index
std::vector<WeightRegion*> rvcx::api::all_regions(Ctx& c, uint64_t* hash) {
  std::vector<WeightRegion*> r;
  uint64_t h = 1469598103934665603ull;
  auto add = [&](WeightRegion* w, uint64_t tag) {
    h = (h ^ tag) * 1099511628211ull;
    h = (h ^ (w ? w->layout_hash() : 0)) * 1099511628211ull;
    if (w) r.push_back(w);
  };
  add(c.hubert ? c.hubert->region.get() : nullptr, 1);
  add(c.rmvpe ? c.rmvpe->region.get() : nullptr, 2);
  add(c.fcpe ? c.fcpe->region.get() : nullptr, 4);
  add(c.crepe ? c.crepe->region.get() : nullptr, 5);
  for (size_t i = 0; i < c.synths.size(); ++i) add(c.synths[i] ? c.synths[i]->region.get() : nullptr, 16 + i);
  add(c.index ? c.index->region.get() : nullptr, 3);
  if (hash) *hash = h;
  return r;
}

static TensorTable make_table(const rvcx_tensor* tbl, int n) {
  TensorTable t;
  for (int i = 0; i < n; ++i) {
    HostTensor h;
    h.data = tbl[i].data;
    h.dtype = tbl[i].dtype;
    for (int d = 0; d < tbl[i].ndim; ++d) h.shape.push_back(tbl[i].shape[d]);
    t.add(tbl[i].name, std::move(h));
  }
  return t;
}

extern "C" {

const char* rvcx_version(void) { return "rvcx 0.1.0 (gfx950)"; }

int rvcx_create(int device, rvcx_ctx** out) {
  try {
    int n = 0;
    RVCX_HIP(hipGetDeviceCount(&n));
    if (n <= 0) fail("no HIP device visible: librvcx has no CPU fallback");
    if (device < 0 || device >= n) fail("device index out of range");
    RVCX_HIP(hipSetDevice(device));
    auto* h = new rvcx_ctx();
    h->c.device = device;
    RVCX_HIP(hipStreamCreateWithFlags(&h->c.stream, hipStreamNonBlocking));
    // Exactly four streams (main, F0 / front, two auxiliaries) and no more: HIP multiplexes a process's streams onto four
    // hardware queues, and a stream that shares one pays for it on every launch.  Rounds 2-3 gave HuBERT a fifth, CU-masked
    // stream ("masked streams get their own queue" -- not in this process): its 143 launches ran at twice their stand-alone
    // time whenever the F0 model was busy too, 4 ms per call in the batched workloads (round 4: HuBERT rides aux[0], which is
    // idle while the front end runs; C3 1220 -> 1290x, C5 1055 -> 1203x; tools/stream_queue_probe.hip shows the sharing).
    {
      // RMVPE ends in a latency-bound serial GRU: give its stream dispatch priority over HuBERT's wide kernels
      int lo = 0, hi = 0;
      RVCX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      const bool prio = !getenv("RVCX_F0_PRIORITY") || atoi(getenv("RVCX_F0_PRIORITY")) != 0;
      RVCX_HIP(hipStreamCreateWithPriority(&h->c.stream2, hipStreamNonBlocking, prio ? hi : lo));
    }
    RVCX_HIP(hipStreamCreateWithFlags(&h->c.aux[0], hipStreamNonBlocking));
    {
      // RVCX_HUBERT_CUS = N (round 6 probe, with RVCX_HUBERT_ON=aux1 RVCX_HUBERT_GATE=0): aux[1] -- unused by the default two
      // branch streams, created fourth like before so that it shares its hardware queue with the main stream, which idles
      // during a single clip's front end -- is confined to the first N CUs (bit i = XCD i mod 8, CU i / 8:
      // tools/cu_mask_probe.hip), for a HuBERT that runs beside the whole F0 model on its own part of the chip
      const int cus = getenv("RVCX_HUBERT_CUS") ? atoi(getenv("RVCX_HUBERT_CUS")) : 0;
      if (cus > 0 && cus < 256) {
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < cus; ++i) mask[i >> 5] |= 1u << (i & 31);
        RVCX_HIP(hipExtStreamCreateWithCUMask(&h->c.aux[1], 8, mask));
      } else {
        RVCX_HIP(hipStreamCreateWithFlags(&h->c.aux[1], hipStreamNonBlocking));
      }
    }
    for (auto& e : h->c.ev_aux) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&h->c.ev_fork, hipEventDisableTiming));
    for (auto& e : h->c.ev_src) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&h->c.ev_join, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&h->c.ev_hub, hipEventDisableTiming));
    for (auto& e : h->c.ev_hubdone) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : h->c.ev_syn) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&h->c.ev_io, hipEventDisableTiming));
    for (auto& e : h->c.ev_front) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : h->c.ev_done) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    conv_init();
    resblock_pair_init();
    gemm_init();
    // Round 6: TWO branch streams (main + aux[0]) by default.  With the third (aux[1]) in use the process has four busy
    // streams besides the null stream, and the main stream's ~110 small TextEncoder / flow launches of a single clip run
    // 0.4 ms slower (the hardware-queue sharing of DESIGN "Batching and streams"): C2 1145 - 1151 -> 1179 - 1182x, C5 1276 -
    // 1280 -> 1291 - 1292x, C3 level (tools/sweep_c2_knobs.sh; all on the main stream: C2 1169 - 1177, C5 1219).
    h->c.resblock_streams = getenv("RVCX_RESBLOCK_STREAMS") ? atoi(getenv("RVCX_RESBLOCK_STREAMS")) : 2;
    // RVCX_SERIAL=1: every launch on the one main stream (rocprofv3 kernel durations are then each launch's own)
    h->c.serial_env = getenv("RVCX_SERIAL") && atoi(getenv("RVCX_SERIAL")) != 0;
    h->c.serial = h->c.serial_env;
    RVCX_HIP(hipMalloc(&h->c.err_words, 3 * sizeof(int)));
    RVCX_HIP(hipMemset(h->c.err_words, 0, 3 * sizeof(int)));
    RVCX_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->c.err_words_host), 3 * sizeof(int), hipHostMallocDefault));
    h->c.dev_err = h->c.err_words;
    h->c.err_host = h->c.err_words_host;
    for (int i = 0; i < 3; ++i) h->c.err_words_host[i] = 0;
    for (int i = 0; i < 2; ++i) {
      h->c.slot[i].err = h->c.err_words + 1 + i;
      h->c.slot[i].err_host = h->c.err_words_host + 1 + i;
    }
    h->c.arena.reserve((size_t)256 << 20);
    {
      // One-time work a serving process should not pay inside its first request (round 2: 88 ms in the first call's
      // high-pass stage): the code object is loaded on the first launch, and every stream / hardware queue is
      // created on its first use.  One trivial launch per stream, then wait.
      float* w = h->c.arena.alloc<float>(256);
      hipStream_t ss[] = {h->c.stream, h->c.stream2, h->c.aux[0], h->c.aux[1]};
      for (hipStream_t s : ss)
        if (s) launch_randn(w, 64, 1, 0, s);
      RVCX_HIP(hipDeviceSynchronize());
      h->c.arena.reset();
    }
    *out = h;
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

void rvcx_destroy(rvcx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  {
    CtxLock guard = lock_ctx(ctx);
    try {
      drain_tickets(ctx);      // the callers' buffers receive what was in flight
    } catch (const std::exception&) {
    }
  }
  (void)hipDeviceSynchronize();
  ctx->sessions.clear();       // open live-stream sessions close with the context
  delete ctx;
}

const char* rvcx_last_error(rvcx_ctx* ctx) {
  // a copy per calling thread: another thread's failing call may replace the context's string at any time
  static thread_local std::string copy;
  if (!ctx) return g_last_error.c_str();
  CtxLock guard = lock_ctx(ctx);
  copy = ctx->c.last_error;
  return copy.c_str();
}

void* rvcx_stream(rvcx_ctx* ctx) { CtxLock ctx_guard_ = lock_ctx(ctx); return ctx ? (void*)ctx->c.stream : nullptr; }

int rvcx_device_info(int device, char* name, int name_cap, int64_t* total_bytes) {
  try {
    int n = 0;
    RVCX_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) fail("device index out of range");
    hipDeviceProp_t prop;
    RVCX_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_cap > 0) {
      snprintf(name, (size_t)name_cap, "%s", prop.name);
    }
    if (total_bytes) *total_bytes = (int64_t)prop.totalGlobalMem;
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

int rvcx_mem_info(rvcx_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes) {
  API_BEGIN_ONCE(ctx)
  size_t f = 0, t = 0;
  RVCX_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  API_END
}

int64_t rvcx_fp32_reruns(rvcx_ctx* ctx) { CtxLock ctx_guard_ = lock_ctx(ctx); return ctx ? (int64_t)ctx->c.fp32_reruns : -1; }

int64_t rvcx_fp32_layers(rvcx_ctx* ctx) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  int64_t n = 0;
  for (WeightRegion* r : all_regions(ctx->c, nullptr)) n += r->dropped();
  return n;
}

int rvcx_fp32_pinned(rvcx_ctx* ctx, char* buf, int cap) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !buf || cap <= 0) return -1;
  Ctx& c = ctx->c;
  std::string t;
  if (c.hubert) t += c.hubert->region->pinned_text("hubert");
  if (c.rmvpe) t += c.rmvpe->region->pinned_text("rmvpe");
  if (c.fcpe) t += c.fcpe->region->pinned_text("fcpe");
  if (c.crepe) t += c.crepe->region->pinned_text("crepe");
  for (size_t i = 0; i < c.synths.size(); ++i)
    if (c.synths[i]) t += c.synths[i]->region->pinned_text("voice model " + std::to_string(i));
  const int n = (int)std::min<size_t>(t.size(), (size_t)cap - 1);
  memcpy(buf, t.data(), (size_t)n);
  buf[n] = 0;
  return (int)t.size();
}

int64_t rvcx_gru_fallbacks(rvcx_ctx* ctx) { CtxLock ctx_guard_ = lock_ctx(ctx); return ctx ? (int64_t)ctx->c.gru_fallbacks : -1; }

int rvcx_gru_publish_probe(rvcx_ctx* ctx) {
  int state = -1;
  const int rc = api_call(ctx, false, [&](Ctx*) {
    (void)bigru_probe_publish();
    state = bigru_probe_state();
  });
  return rc ? -2 : state;
}

int64_t rvcx_index_exhaustive(rvcx_ctx* ctx) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || !ctx->c.index || !ctx->c.index->exhaustive) return -1;
  int v = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  (void)hipMemcpy(&v, ctx->c.index->exhaustive, sizeof(int), hipMemcpyDeviceToHost);
  (void)hipMemset(ctx->c.index->exhaustive, 0, sizeof(int));
  return v;
}

int rvcx_debug_inject(rvcx_ctx* ctx, int what) {
  REQUIRE_DEBUG(ctx, "rvcx_debug_inject")
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (ctx && what == 2) {          // read and clear the raw device error word (debugging builds set extra bits)
    int v = 0;
    (void)hipMemcpy(&v, ctx->c.dev_err, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipMemset(ctx->c.dev_err, 0, sizeof(int));
    return v;
  }
  if (ctx && what == 3) {          // the next BiGRU cluster launch of this thread loses a member: its partners really time out
    g_gru_drop_member = 1;
    return 0;
  }
  if (!ctx || what != 1) return -1;
  ctx->c.inject_gru_timeout = true;
  return 0;
}

double rvcx_flop_counter(rvcx_ctx* ctx, int reset) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return 0.0;
  double f = ctx->c.flops;
  if (reset) ctx->c.flops = 0.0;
  return f;
}

int rvcx_load_synth(rvcx_ctx* ctx, const rvcx_synth_cfg* cfg, const rvcx_tensor* tbl, int n, int* model_id) {
  API_BEGIN_ONCE(ctx)
  TensorTable t = make_table(tbl, n);
  auto m = synth_load(*C, *cfg, t);
  int id = -1;
  for (size_t i = 0; i < C->synths.size(); ++i)
    if (!C->synths[i]) id = (int)i;
  if (id < 0) {
    C->synths.emplace_back();
    id = (int)C->synths.size() - 1;
  }
  C->synths[id] = std::move(m);
  *model_id = id;
  API_END
}

int rvcx_unload_synth(rvcx_ctx* ctx, int model_id) {
  API_BEGIN_ONCE(ctx)
  if (model_id < 0 || model_id >= (int)C->synths.size()) fail("bad model id");
  RVCX_HIP(hipDeviceSynchronize());
  C->synths[model_id].reset();   // frees the model's weight region
  API_END
}

int rvcx_synth_upp(rvcx_ctx* ctx, int model_id) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx || model_id < 0 || model_id >= (int)ctx->c.synths.size() || !ctx->c.synths[model_id]) return -1;
  return ctx->c.synths[model_id]->upp;
}

int rvcx_weights_regions(rvcx_ctx* ctx, int cap, void** dev_ptrs, int64_t* nbytes, uint64_t* layout_hash) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  Ctx* C = ctx ? &ctx->c : nullptr;
  try {
    if (!C) fail("null context");
    RVCX_HIP(hipSetDevice(C->device));
    int k = 0;
    for (WeightRegion* r : all_regions(*C, layout_hash))
      for (int i = 0; i < r->n_chunks(); ++i, ++k)
        if (k < cap) {
          dev_ptrs[k] = r->chunk_base(i);
          nbytes[k] = (int64_t)r->chunk_used(i);
        }
    return k;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    if (C) C->last_error = e.what();
    return -1;
  }
}

int rvcx_weights_clone(rvcx_ctx* ctx, rvcx_ctx* src) {
  // both contexts' mutexes, acquired deadlock-free (two threads cloning A <- B and B <- A)
  CtxLock ga, gb;
  if (ctx && src && ctx != src) {
    ga = CtxLock(ctx->mu, std::defer_lock);
    gb = CtxLock(src->mu, std::defer_lock);
    std::lock(ga, gb);
  }
  API_BEGIN_ONCE(ctx)
  if (!src) fail("weights_clone: null source context");
  if (src->c.device != C->device) fail("weights_clone: contexts live on different devices (use the RCCL broadcast)");
  uint64_t ha = 0, hb = 0;
  std::vector<WeightRegion*> ra = all_regions(src->c, &ha), rb = all_regions(*C, &hb);
  if (ha != hb || ra.size() != rb.size()) fail("weights_clone: the two contexts hold different model layouts");
  RVCX_HIP(hipDeviceSynchronize());
  for (size_t r = 0; r < ra.size(); ++r) {
    if (ra[r]->n_chunks() != rb[r]->n_chunks()) fail("weights_clone: chunk lists differ");
    for (int i = 0; i < ra[r]->n_chunks(); ++i) {
      if (ra[r]->chunk_used(i) != rb[r]->chunk_used(i)) fail("weights_clone: chunk sizes differ");
      RVCX_HIP(hipMemcpy(rb[r]->chunk_base(i), ra[r]->chunk_base(i), ra[r]->chunk_used(i), hipMemcpyDeviceToDevice));
    }
    rb[r]->adopt();
  }
  API_END
}

int rvcx_weights_adopt(rvcx_ctx* ctx) {
  API_BEGIN_ONCE(ctx)
  RVCX_HIP(hipDeviceSynchronize());
  for (WeightRegion* r : all_regions(*C, nullptr)) r->adopt();
  API_END
}

int rvcx_load_rmvpe(rvcx_ctx* ctx, const rvcx_rmvpe_cfg* cfg, const rvcx_tensor* tbl, int n) {
  API_BEGIN_ONCE(ctx)
  TensorTable t = make_table(tbl, n);
  C->rmvpe = rmvpe_load(*C, *cfg, t);
  (void)bigru_probe_publish();   // the BiGRU's publish assumption, checked once per device while it is idle (gru.hip)
  API_END
}

int rvcx_load_crepe(rvcx_ctx* ctx, const rvcx_tensor* tbl, int n) {
  API_BEGIN_ONCE(ctx)
  TensorTable t = make_table(tbl, n);
  C->crepe = crepe_load(*C, t);
  API_END
}

int rvcx_load_fcpe(rvcx_ctx* ctx, const rvcx_fcpe_cfg* cfg, const rvcx_tensor* tbl, int n) {
  API_BEGIN_ONCE(ctx)
  TensorTable t = make_table(tbl, n);
  C->fcpe = fcpe_load(*C, *cfg, t);
  API_END
}

int rvcx_load_hubert(rvcx_ctx* ctx, const rvcx_hubert_cfg* cfg, const rvcx_tensor* tbl, int n) {
  API_BEGIN_ONCE(ctx)
  TensorTable t = make_table(tbl, n);
  C->hubert = hubert_load(*C, *cfg, t);
  API_END
}

int rvcx_load_index(rvcx_ctx* ctx, const float* big_npy, int64_t n, int dim) {
  API_BEGIN_ONCE(ctx)
  if (!big_npy || n == 0) {
    C->index.reset();
  } else {
      C->index = index_load(*C, big_npy, n, dim);
  }
  API_END
}

int rvcx_load_index_ivf(rvcx_ctx* ctx, const float* big_npy, int64_t n, int dim, const float* centroids, int nlist,
                        const int32_t* assign, int nprobe) {
  API_BEGIN_ONCE(ctx)
  if (!big_npy || n <= 0 || !centroids || nlist <= 0 || !assign) fail("load_index_ivf: null argument");
  if (nprobe != 1) fail("load_index_ivf: only nprobe = 1 (what RVC index files carry) is implemented");
  C->index = index_load(*C, big_npy, n, dim, centroids, nlist, assign);
  API_END
}

// The per-launch profile is PROCESS-wide state (conv.hip): the two hooks below serialise against each other on one mutex, but
// launches of ANOTHER context that run while a profile is open are recorded into it too (rvcx.h says so).
static std::mutex g_profile_mu;

int rvcx_conv_profile(rvcx_ctx* ctx, int begin, int64_t* launches, double* flops, double* ms, int32_t* bm,
                      int32_t* bn, int32_t* kind, int cap) {
  std::lock_guard<std::mutex> prof_guard(g_profile_mu);
  API_BEGIN_ONCE(ctx)
  C->serial = begin != 0 || C->serial_env;
  if (begin) {
    conv_profile_begin();
  } else {
    ConvProfile p;
    conv_profile_end(&p);
    for (int t = 0; t < cap && t < ConvProfile::kMaxTiles; ++t) {
      launches[t] = p.launches[t];
      flops[t] = p.flops[t];
      ms[t] = p.ms[t];
      bm[t] = p.bm[t];
      bn[t] = p.bn[t];
      kind[t] = p.halo[t];
    }
  }
  API_END
}

const char* rvcx_conv_profile_csv(rvcx_ctx*) {
  std::lock_guard<std::mutex> g(g_profile_mu);
  return conv_profile_csv();
}

int rvcx_last_timing(rvcx_ctx* ctx, float* ms9) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  for (int k = 0; k < 9; ++k) ms9[k] = ctx->c.timing[k];
  return 0;
}

// ------------------------------------------------------------------------------------------
// entry points not implemented yet return an error (never a silent fallback)
// ------------------------------------------------------------------------------------------
#define NOT_IMPL(ctxp, name)                    \
  do {                                          \
    g_last_error = name ": not implemented";    \
    if (ctxp) (ctxp)->c.last_error = g_last_error; \
    return -1;                                  \
  } while (0)

int rvcx_rmvpe_frames(int64_t n) { return (int)(1 + n / 160); }
int rvcx_fcpe_frames(int64_t n) { return (int)(1 + n / 160); }

}  // extern "C"
