// Formant shift and envelope transfer (include/rvcx.h stages 17 and 18): a true-envelope estimate per frame, replaced by a
// warped copy of an envelope.  formant.hip holds the kernels, their launchers and the host twin; api_formant.hip the entry
// points.  Geometry, window and transform are stage 13's (pitch.h, fft_device.h).
//
// Device layout: planar rows as in effects.h (row r = item * C + channel, len[r] samples at the front of ld floats).  A row
// with a source has it in the same row of a second plane.  Per row the stage keeps the windowed frames alone: Tf = T_max
// frames of N floats.  Spectra, envelopes and gains never leave the workgroup (the taps aside).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "pitch.h"

// A2, eps, L, W, g and the energy terms are defined with every rounding written out, so contraction is off from here on in
// whichever file includes this one
#pragma clang fp contract(off)

namespace rvcx {

constexpr int kFormantKpt = 17;          // bins per lane of a 256-lane workgroup at nb = 4097
constexpr int kFormantCpt = 5;           // kept quefrencies per lane at nc = N / 8 = 1024 (q = 0 .. nc)
constexpr int kFormantMaxIter = 16;

struct FxFormantValues {                 // rvcx_fx_formant_params without the signal's shape
  float ratio, amount, quefrency_ms, max_gain_db;
  int iterations, keep_energy;
};
inline double fx_formant_nc(double ms, int sr) { return std::floor(ms * (double)sr / 1000.0); }
inline double fx_formant_limit(double max_gain_db) { return max_gain_db * 2.302585092994045684 / 20.0; }

// ---- the pointwise rules, one text for the kernel and the host twin
__host__ __device__ inline float fm_a2(float re, float im) {
  const float rr = re * re, ii = im * im;
  return rr + ii;
}
__host__ __device__ inline float fm_eps(float top) {
  const float a = 1e-10f * top;
  return a + 1e-20f;
}
__host__ __device__ inline float fm_log(float a2, float eps) {
  const float s = a2 + eps;
  return 0.5f * logf(s);
}
// W[k] from the target envelope (es(i): bin i as float), in double, rounded once
template <typename F>
__host__ __device__ inline float fm_warp(F es, int k, int nb, double ratio) {
  const double u = (double)k / ratio, fi = floor(u);
  if (fi >= (double)(nb - 1)) return es(nb - 1);
  const int i = (int)fi;
  const double f = u - fi, lo = (1.0 - f) * (double)es(i), hi = f * (double)es(i + 1);
  return (float)(lo + hi);
}
__host__ __device__ inline float fm_gain(float W, float E, float amount, double limit) {
  double d = (double)amount * ((double)W - (double)E);
  d = d > limit ? limit : (d < -limit ? -limit : d);
  return expf((float)d);
}
// the two terms a bin adds to e0 and e1
__host__ __device__ inline void fm_energy(float a2, float g, bool edge, double& e0, double& e1) {
  const double c = edge ? 1.0 : 2.0, gg = (double)g * (double)g, t = gg * (double)a2;
  e0 += c * (double)a2;
  e1 += c * t;
}
__host__ __device__ inline float fm_scale(double e0, double e1) { return e1 == 0.0 ? 1.f : (float)sqrt(e0 / e1); }

struct FxFormantTaps {                   // device pointers, row 0 only; each optional
  float2* D;                             // (T, nb)
  float* E;                              // (T, nb)
  float* Es;
  float* g;
  float* s;                              // (T)
};
struct FxFormantDev {
  FxStretchGeom g;
  FxFormantValues v;
  int nc;
  double limit;                          // max_gain_db ln(10) / 20
  int R;
  long ld, Tf;                           // floats per input row, frames per row
  const int* len;                        // R ints on the device
  const int* has_src;                    // R ints: 1 when the row has a source
  const float* x;                        // (R, ld)
  const float* src;                      // (R, ld) or null when no row has a source
  const float* w;
  const float2* tw;
  float* fr;                             // (R, Tf, N): the windowed frames
  FxFormantTaps taps;
};
inline size_t fx_formant_row_bytes(const FxStretchGeom& g, long Tf) { return (size_t)Tf * g.N * sizeof(float); }

// the frames of every row (ev[0] behind them), then the overlap-add into y (R rows, ld_y apart; ev[1] behind it)
void launch_formant(const FxFormantDev& d, float* y, long ld_y, hipStream_t s, hipEvent_t* ev);

// ---- host twin: one channel.  src == null: the item's own envelope is the target.  Optional taps: D (T, nb) float pairs,
// E, Es, g (T, nb), s (T)
void fx_formant_host(const float* x, long n, const float* src, int sr, const FxFormantValues& v, float* y, float* D, float* E,
                     float* Es, float* g, float* s);
// the true envelope of one frame from its L (nb = N / 2 + 1 floats)
void fx_formant_envelope_host(const float* L, int N, int nc, int iterations, float* E);

}  // namespace rvcx
