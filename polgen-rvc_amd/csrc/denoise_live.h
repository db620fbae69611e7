// Live noise reduction (include/rvcx.h stage 16): the causal spectral gate a live-stream session runs at either edge of a step.
// denoise_live.hip holds the kernels, the step and the host twin; api_stream_denoise.hip the entry points.  The pointwise rules
// are stage 15's (denoise_device.h), window and transform stage 13's (pitch.h, fft_device.h).
//
// State of one stream, in floats from its start (fixed by rate and widths at open, whatever the other parameters):
//   fifo   N floats: the last N samples received, oldest first
//   tail   N floats: the overlap-add sums of the N samples that follow the last one emitted
//   ring   nt x nb floats: the frequency-smoothed rows of the last nt frames, frame t at row t mod nt
//   f      nb doubles (2 nb floats, 8-byte aligned): the floor of the last frame
// It exists twice: a step reads one set and writes the other whole.  Nothing is a stored position: a step derives the frames
// it completes from its counter alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "pitch.h"

namespace rvcx {

constexpr int kDnLiveMaxNf = 64, kDnLiveMaxNt = 32;
constexpr int kDnLiveStatChunk = 64;     // profile frames per partial sum of mu and sd (stage 15's)
constexpr int kDnLiveLaneBins = 9;       // bins a lane owns at the largest N (4096: 2049 bins over 256 lanes)

// N = the smallest power of two with 48 N >= sr, never below 512
inline FxStretchGeom dn_live_geom(int sr) {
  int N = 512, l = 9;
  while (48L * N < sr) N *= 2, ++l;
  return {N, N / 4, N / 2 + 1, l};
}
inline bool dn_live_rate_ok(int sr) { return sr >= 3200 && sr <= 192000 && sr % 100 == 0; }
// half-widths in double (a caller checks the range before it narrows them)
inline double dn_live_nf(double hz, int N, int sr) { return std::floor(hz * (double)N / (2.0 * (double)sr)); }
inline double dn_live_nt(double ms, int sr, int H) { return std::floor(ms * (double)sr / (1000.0 * (double)H)); }
inline double dn_live_c(int H, int sr, double tc) { return std::exp(-(double)H / ((double)sr * tc)); }
// frames complete once n samples have arrived: frame t needs the samples below t H + N / 2
inline long dn_live_frames(long n, int N, int H) { return n >= N / 2 ? (n - N / 2) / H + 1 : 0; }
// sum of w^2 over the frames t >= 0 that cover sample j >= 0, in ascending t (the live formant stage divides by it too)
__host__ __device__ inline double dn_live_den(const float* w, long j, int N, int H) {
#pragma clang fp contract(off)           // every product rounded, whatever the including file has set
  const long a = (j - N / 2 + H) / H, tlo = a > 0 ? a : 0, thi = (j + N / 2) / H;
  double den = 0.0;
  for (long t = tlo; t <= thi; ++t) {
    const long i = j + N / 2 - t * H;
    if (i < 0 || i >= N) continue;                     // (never: the bounds of tlo and thi)
    den += (double)w[i] * (double)w[i];
  }
  return den;
}

struct DnLiveValues {                    // rvcx_live_denoise_params without the signal's shape and the widths
  int mode;
  float strength, n_std, knee_db, thresh_mult, slope;
  double c_up, c_dn;                     // mode 1: exp(-H / (sr time_constant_s)), exp(-H / (sr fall_time_s))
};

struct DnLive {
  int S = 0, sr = 0, nf = 0, nt = 0;
  long B = 0;                            // samples per block and row
  FxStretchGeom g{};
  DnLiveValues v{};
  long off_tail = 0, off_ring = 0, off_f = 0, per_stream = 0;   // floats
  float* state[2] = {nullptr, nullptr};  // (S, per_stream) each
  float* acc = nullptr;                  // (S, N + B): the sums a step works on
  const float* w = nullptr;              // N
  const float2* tw = nullptr;            // N / 2
  const double* mu = nullptr;            // mode 0: nb each, one profile for all streams of the side
  const double* sd = nullptr;
};
// fills the offsets from g, nt (S, B set): what open allocates
void dn_live_layout(DnLive& d);

// One block of every stream.  x: S rows of B samples, ldx apart; y: S rows of B samples, ldy apart (y may not alias x).  Reads
// state[cur], writes state[cur ^ 1]; step: blocks since sample 0.  One launch, no atomics, no host synchronisation.  Taps
// (optional, each (S, T_tap, nb), frame t of stream s at (s T_tap + t) nb): S, f (doubles) and m of the frames completed.
struct DnLiveTaps {
  float* S = nullptr;
  double* f = nullptr;
  float* m = nullptr;
  long T = 0;
};
void dn_live_step(const DnLive& d, const float* x, long ldx, int cur, uint64_t step, float* y, long ldy, hipStream_t s,
                  const DnLiveTaps* taps = nullptr);
// mode 0: mu and sd (nb doubles each, on the device) from the smoothed power S (Tp, nb) of the noise clip
void launch_dn_live_stats(const float* S, long Tp, int nb, double* mu, double* sd, hipStream_t s);

// ---- host twin: one channel, the whole signal.  y receives n samples, delayed by N.  Optional taps for the T =
// dn_live_frames(n) frames: D (T, nb) float pairs, S (T, nb), f (T, nb) doubles, m (T, nb); mu, sd (nb, in: mode 0)
struct DnLiveHostPlan {
  int sr, nf, nt;
  DnLiveValues v;
};
void dn_live_host(const float* x, long n, const DnLiveHostPlan& P, const double* mu, const double* sd, float* y, float* D, float* S,
                  double* f, float* m);
// mu and sd of a noise clip of n samples (n >= N / 2): stage 16's analysis on the clip, stage 15's statistics
void dn_live_profile_host(const float* clip, long n, const DnLiveHostPlan& P, double* mu, double* sd);

}  // namespace rvcx
