// What the post-production ABI files share (api_fx, api_loudness, api_pitch, api_denoise, api_formant, api_stream_denoise):
// the call driver around a stage's kernel sequence.  A stage file keeps its own checks, its item_bytes formula and what it
// reserves, its kernel sequence in stream order and its meaning of the nine rvcx_last_timing slots; everything else is here.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <utility>

#include "api_internal.h"
#include "pitch.h"

namespace rvcx {
namespace api {

// the host twins have no context: the message goes where rvcx_last_error(NULL) reads it
template <typename F>
int host_call(F&& body) {
  try {
    body();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -1;
  }
}

// ---- refusals: `who` is the entry point's name as rvcx_last_error shows it ------------------------------------------------------
// live: the range of the live gate (denoise_live.h), which reaches down to the reduced-size voice models' rates
inline void check_rate(const char* who, int sr, bool live = false) {
  if (!(live ? dn_live_rate_ok(sr) : fx_rate_ok(sr)))
    fail(std::string(who) + ": the sample rate must be a multiple of 100 Hz within " + (live ? "3200" : "8000") + " .. 192000");
}
inline void check_channels(const char* who, int channels) {
  if (channels != 1 && channels != 2) fail(std::string(who) + ": channels must be 1 or 2");
}
inline void check_frames(const char* who, int64_t n, const char* text = "every item needs 1 .. 2^30 frames") {
  if (n < 1 || n > (int64_t)1 << 30) fail(std::string(who) + ": " + text);
}
// the tables of a batched call: x, n and whichever further tables (y) must hold a pointer for every item
template <typename X, typename... Y>
void check_items(const char* who, int B, X* const* x, const int64_t* n, Y* const*... y) {
  if (B < 1 || !x || !n || (... || !y)) fail(std::string(who) + ": null argument or B < 1");
  for (int b = 0; b < B; ++b) {
    if (!x[b] || (... || !y[b])) fail(std::string(who) + ": null pointer in a table");
    check_frames(who, n[b]);
  }
}
inline void check_finite(const char* who, std::initializer_list<double> values, const char* what = "a value") {
  for (double v : values)
    if (!std::isfinite(v)) fail(std::string(who) + ": " + what + " is not finite");
}
inline void check_range(const char* who, float f, double lo, double hi, const char* name) {
  if (!((double)f >= lo && (double)f <= hi))
    fail(std::string(who) + ": " + name + " must lie in " + std::to_string(lo) + " .. " + std::to_string(hi));
}
// an item is never cut into segments: alone (own_bytes, tables included) it has to fit the arena budget
inline void check_item_fits(const char* who, Ctx& c, int b, int64_t n, size_t own_bytes) {
  const size_t budget = arena_budget(c);
  if (own_bytes > budget)
    fail(std::string(who) + ": item " + std::to_string(b) + " of " + std::to_string((long)n) + " frames needs " +
         std::to_string(own_bytes) + " bytes, the arena budget is " + std::to_string(budget) + " (one item is not cut into segments)");
}

// ---- row strides -------------------------------------------------------------------------------------------------------------------
inline long pad256(long n) { return (std::max<long>(n, 1) + 255) / 256 * 256; }
// whole chunks of the scans.  (The clamp to one frame is for callers that have not refused n < 1 yet; the chain has.)
inline long fx_ld(int64_t n) { return (long)((std::max<int64_t>(n, 1) + kFxChunk - 1) / kFxChunk) * kFxChunk; }

// ---- groups ------------------------------------------------------------------------------------------------------------------------
// items per group: what the activation budget holds beside the tables at the worst item's size, B and RVCX_MAX_BATCH at the most,
// one at the least.  (The variable is read on every call: the tests change it within one process.)
inline int fx_group_size(Ctx& c, int B, size_t worst_item_bytes, size_t table_bytes) {
  const char* cap = getenv("RVCX_MAX_BATCH");
  const size_t most = cap ? (size_t)std::max(1, atoi(cap)) : (size_t)B, budget = arena_budget(c);
  const size_t fit = (budget > table_bytes ? budget - table_bytes : 0) / worst_item_bytes;
  return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(most, (size_t)B), fit));
}

// host side of the plain row lengths of a group: the Cc rows of item i hold n[i] frames each
inline std::vector<int> row_lengths(const int64_t* n, int Bg, int Cc) {
  std::vector<int> len((size_t)Bg * Cc);
  for (size_t r = 0; r < len.size(); ++r) len[r] = (int)n[r / Cc];
  return len;
}

// ---- staging: a group's items lie interleaved one per slot of ld frames, the kernels see one plane of ld frames per row --------
// in: item(i) -> {where item i lies (host or device memory), its frames}; a null pointer or no frames: slot i is left as it is
template <typename F>
void stage_in(F&& item, int Bg, int Cc, long ld, float* stage, float* rows, const int* dlen, hipStream_t s) {
  for (int i = 0; i < Bg; ++i) {
    const std::pair<const float*, int64_t> it = item(i);
    if (it.first && it.second > 0)
      RVCX_HIP(hipMemcpyAsync(stage + (size_t)i * ld * Cc, it.first, (size_t)it.second * Cc * 4, hipMemcpyDefault, s));
  }
  launch_fx_deinterleave(stage, rows, dlen, Bg, Cc, ld, s);
}
// out: item(i) -> {where item i goes, its frames}
template <typename F>
void stage_out(const float* rows, const int* dlen, int Bg, int Cc, long ld, float* stage, hipStream_t s, F&& item) {
  launch_fx_interleave(rows, stage, dlen, Bg, Cc, ld, s);
  for (int i = 0; i < Bg; ++i) {
    const std::pair<float*, int64_t> it = item(i);
    RVCX_HIP(hipMemcpyAsync(it.first, stage + (size_t)i * ld * Cc, (size_t)it.second * Cc * 4, hipMemcpyDefault, s));
  }
}

// the window and the twiddles of the N-point transform (pitch.h); upload() after every arena reset
struct StftTables {
  std::vector<float> w;
  std::vector<float2> tw;
  explicit StftTables(int N) { fx_stretch_tables(N, w, tw); }
  void upload(Ctx& c, const float*& dw, const float2*& dtw) const {
    dw = to_dev(c, w.data(), w.size());
    dtw = to_dev(c, tw.data(), tw.size());
  }
};

// ---- timing: the context's events, and the nine slots of rvcx_last_timing summed over the groups ------------------------------
struct FxTimer {
  hipEvent_t* ev;
  hipStream_t s;
  float ms[9] = {0};
  explicit FxTimer(Ctx& c) : s(c.stream) {
    c.timer.make();
    ev = c.timer.ev;
  }
  void mark(int k) { RVCX_HIP(hipEventRecord(ev[k], s)); }
  // after the group's synchronisation: the interval between two events into a slot (returns it)
  float add(int slot, hipEvent_t a, hipEvent_t b) {
    float t = 0.f;
    RVCX_HIP(hipEventElapsedTime(&t, a, b));
    ms[slot] += t;
    return t;
  }
  float add(int slot, int a, int b) { return add(slot, ev[a], ev[b]); }
  // `count` consecutive intervals from event a on into the slots from `slot` on
  void add_each(int slot, int a, int count) {
    for (int k = 0; k < count; ++k) add(slot + k, a + k, a + k + 1);
  }
  void store(Ctx& c) const { std::copy(ms, ms + 9, c.timing); }
};

// ---- skip: nothing is launched, every output is its input bit for bit ----------------------------------------------------------
inline void copy_through(int B, const float* const* x, const int64_t* n, int Cc, float* const* y) {
  for (int b = 0; b < B; ++b)
    if (y[b] != x[b]) RVCX_HIP(hipMemcpy(y[b], x[b], (size_t)n[b] * Cc * 4, hipMemcpyDefault));
}
inline void fx_skip(rvcx_ctx* h, int B, const float* const* x, const int64_t* n, int Cc, float* const* y) {
  copy_through(B, x, n, Cc, y);
  std::fill(h->c.timing, h->c.timing + 9, 0.f);
  h->fx_groups = 0;
}

// ---- host twins are mono: channel c of a signal as a plane, and the loop over the channels ---------------------------------
inline void take_plane(const float* x, int64_t n, int Cc, int c, std::vector<float>& plane) {
  plane.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) plane[i] = x[i * Cc + c];
}
// mono(c, plane) -> the n_out frames of channel c's result
template <typename F>
void host_planes(const float* x, int64_t n, int Cc, float* y, int64_t n_out, F&& mono) {
  std::vector<float> plane;
  for (int c = 0; c < Cc; ++c) {
    take_plane(x, n, Cc, c, plane);
    const float* res = mono(c, plane.data());
    for (int64_t i = 0; i < n_out; ++i) y[i * Cc + c] = res[i];
  }
}

}  // namespace api
}  // namespace rvcx
