// Noise reduction (include/rvcx.h stage 15): a soft spectral gate, from a noise profile (mode 0) or adaptive (mode 1).
// denoise.hip holds the kernels, their launchers and the host twin; api_denoise.hip the entry points.  Geometry, window and
// transform are stage 13's (pitch.h, fft_device.h).
//
// Device layout: planar rows as in effects.h (row r = item * C + channel, len[r] samples at the front of ld floats).  Per row
// and bin of its Tf = T_max frames: D (8 bytes, float pairs; the synthesis writes each frame's N windowed samples over the
// frame's own nb pairs, which it has read), A2 (4 bytes; the mask m takes its place once S exists), S (4 bytes) and, in mode 1
// only, the forward floor f (8 bytes, double): 16 bytes per bin in mode 0, 24 in mode 1.  Noise clips are rows of a second
// set that holds A2 and S alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "pitch.h"

namespace rvcx {

constexpr int kDenoiseTileT = 16;        // frames per smoothing tile
constexpr int kDenoiseTileK = 64;        // bins per smoothing tile
constexpr int kDenoiseStatChunk = 64;    // profile frames per partial sum of mu and sd
constexpr int kDenoiseMaxNf = 64, kDenoiseMaxNt = 16;

struct FxDenoiseValues {                 // rvcx_fx_denoise_params without the signal's shape
  int mode;
  float strength, n_std, knee_db, thresh_mult, slope, time_constant_s, freq_smooth_hz, time_smooth_ms;
};
// half-widths in double (a caller checks the range before it narrows them)
inline double fx_denoise_nf(double hz, int N, int sr) { return std::floor(hz * (double)N / (2.0 * (double)sr)); }
inline double fx_denoise_nt(double ms, int sr, int H) { return std::floor(ms * (double)sr / (2000.0 * (double)H)); }
inline double fx_denoise_c(int H, int sr, double tc) { return std::exp(-(double)H / ((double)sr * tc)); }

struct FxDenoiseRows {                   // one set of rows: the items, or their noise clips
  int R;
  long ld, Tf;                           // floats per input row, frames per row
  const int* len;                        // R ints on the device
  const float* x;                        // (R, ld)
  float2* D;                             // (R, Tf, nb) or null (noise clips)
  float* A2;                             // (R, Tf, nb): A2, then m
  float* S;                              // (R, Tf, nb)
};
struct FxDenoiseDev {
  FxStretchGeom g;
  FxDenoiseValues v;
  int nf, nt;
  double c;                              // mode 1: exp(-H / (sr time_constant_s))
  const float* w;
  const float2* tw;
  FxDenoiseRows it, nz;                  // nz.R == 0 without a clip
  const int* prof;                       // mode 0, per item row: its row of nz, or -1 for the item's own frames
  double* mu;                            // mode 0: (R, nb)
  double* sd;
  double* f;                             // mode 1: (R, Tf, nb)
  double* b;                             // mode 1, taps only: (R, Tf, nb), else null
};
// bytes per row of the arrays above (x and y planes not counted)
size_t fx_denoise_row_bytes(const FxStretchGeom& g, long Tf, int mode, bool item, bool want_b);

// D (items), A2 of both sets, then S of both sets; ev (optional, 2 events): behind the transforms and behind the smoothing
void launch_denoise_analysis(const FxDenoiseDev& d, hipStream_t s, hipEvent_t* ev);
// mode 0: mu and sd (ev[0] behind them), then m; mode 1: f, b and m in one launch (ev[0] behind it, ev[1] right after)
void launch_denoise_mask(const FxDenoiseDev& d, hipStream_t s, hipEvent_t* ev);
// g from m, Y = g D, the windowed frames (over D), ev[0], the overlap-add into y (R rows, ld_y apart), ev[1]
void launch_denoise_synthesis(const FxDenoiseDev& d, float* y, long ld_y, hipStream_t s, hipEvent_t* ev);

// ---- host twin: one channel.  noise == null: the item's own frames are the profile (mode 0).  Optional taps: D (T, nb) float
// pairs, S (T, nb), mu and sd (nb doubles, mode 0), b (T, nb) doubles (mode 1), m (T, nb)
void fx_denoise_host(const float* x, long n, const float* noise, long n_noise, int sr, const FxDenoiseValues& v, float* y,
                     float* D, float* S, double* mu, double* sd, double* b, float* m);
// the smoothing alone on a (T, nb) array, float32 in the defined order
void fx_denoise_smooth_host(const float* A2, long T, int nb, int nf, int nt, float* S);

}  // namespace rvcx
