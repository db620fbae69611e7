// Live formant shift (include/rvcx.h stage 19): stage 17 without a source, made causal on stage 16's grid, so that a live-stream
// session can run it inside a step at either edge.  formant_live.hip holds the kernels, the step and the host twin;
// api_stream_formant.hip the entry points.  The pointwise rules are stage 17's (formant.h), the frame's chain is the one stage 17
// runs (formant_device.h), geometry, frame count and window sum are stage 16's (denoise_live.h).
//
// State of one stream, in floats from its start (fixed by the rate at open):
//   fifo   N floats: the last N samples received, oldest first
//   tail   N floats: the overlap-add sums of the N samples that follow the last one emitted
// A frame has no recurrence across frames, so there is nothing else.  It exists twice: a step reads one set and writes the other
// whole.  Nothing is a stored position: a step derives the frames it completes from its counter alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "denoise_live.h"
#include "formant.h"

namespace rvcx {

constexpr int kFmLiveKpt = 9;            // bins a lane owns at the largest N (4096: 2049 bins over 256 lanes)
constexpr int kFmLiveCpt = 3;            // kept quefrencies per lane at nc = N / 8 = 512 (q = 0 .. nc)

// amount == 0 or ratio == 1: the side emits the delayed input; frames and sums keep running
inline bool fm_live_off(const FxFormantValues& v) { return v.amount == 0.f || v.ratio == 1.f; }

struct FmLive {
  int S = 0, sr = 0, nc = 0;
  long B = 0;                            // samples per block and row
  FxStretchGeom g{};                     // dn_live_geom(sr)
  FxFormantValues v{};
  float* state[2] = {nullptr, nullptr};  // (S, 2 N) each: fifo, then tail
  float* fr = nullptr;                   // (S, B / H + 2, N): the windowed frames of a step
  const float* w = nullptr;              // N
  const float2* tw = nullptr;            // N / 2
};
inline long fm_live_per_stream(const FmLive& d) { return 2L * d.g.N; }
inline long fm_live_slots(const FmLive& d) { return d.B / d.g.H + 2; }

// Taps (optional, E and g (S, T, nb), s (S, T)): the frames t < T a step completes
struct FmLiveTaps {
  float* E = nullptr;
  float* g = nullptr;
  float* s = nullptr;
  long T = 0;
};
// One block of every stream.  x: S rows of B samples, ldx apart; y: S rows of B samples, ldy apart (y may not alias x).  Reads
// state[cur], writes state[cur ^ 1]; step: blocks since sample 0.  Two launches (one when the step completes no frame), no
// atomics, no host synchronisation.
void fm_live_step(const FmLive& d, const float* x, long ldx, int cur, uint64_t step, float* y, long ldy, hipStream_t s,
                  const FmLiveTaps* taps = nullptr);

// ---- host twin: one channel, the whole signal.  y receives n samples, delayed by N.  Optional taps for the T =
// dn_live_frames(n) frames: D (T, nb) float pairs, E and g (T, nb), s (T).  nc is checked by the caller
void fm_live_host(const float* x, long n, int sr, const FxFormantValues& v, float* y, float* D, float* E, float* g, float* s);

}  // namespace rvcx
