// Key change for the backing track (include/rvcx.h stages 13 and 14): the phase-locked vocoder on integer phases and the
// pitch shift built on it.  pitch.hip holds the kernels, their launchers and the host twin; api_pitch.hip the entry points;
// audio.hip the resampler behind stage 14 (one channel plane through kaiser_exact_taps).
//
// Device layout: planar rows as in effects.h (row r = item * C + channel, len[r] samples at the front of ld floats).  Per row
// the analysis holds Tf = T_max + 2 frames of nb bins (A2, TH, own; D only for the taps); the synthesis runs in segments of
// output frames: R for the segment's frames, the windowed frames fr in S + 3 slots (slots 0 .. 2: the last three frames of
// the segment before), and the chunk maps of the scan.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "ops.h"

namespace rvcx {

struct FxStretchGeom {
  int N, H, nb, logN;
};
inline FxStretchGeom fx_stretch_geom(int sr) {      // the smallest power of two with 24 N >= sr
  int N = 2, l = 1;
  while (24L * N < sr) N *= 2, ++l;
  return {N, N / 4, N / 2 + 1, l};
}
inline long fx_stretch_len(long n, long P, long Q) { return (n * P + Q / 2) / Q; }
inline long fx_stretch_T(long n, int H) { return n / H + 1; }
inline long fx_stretch_J(long T, long P, long Q) { return (T * P + Q - 1) / Q; }
inline bool fx_stretch_ratio_ok(long P, long Q) { return Q >= 1 && Q <= (1L << 20) && 2 * P >= Q && P <= 2 * Q; }
// P of stage 14: floor(sr 2^(s/12) + 0.5), formed in double
long fx_pitch_P(int sr, double semitones);

constexpr int kStretchChunk = 32;        // output frames whose maps one workgroup composes (rvcx_fx_stretch_chunk)
constexpr int kStretchSegment = 512;     // output frames per segment
constexpr int kStretchKpt = 17;          // bins per lane of a 256-lane workgroup at nb = 4097

// the window (N floats) and the twiddles e^(-2 pi i k / N), k < N / 2, both formed in double and rounded once
void fx_stretch_tables(int N, std::vector<float>& w, std::vector<float2>& tw);

struct FxStretchDev {                    // what every launch of one group needs
  FxStretchGeom g;
  long P, Q;
  int R;                                 // rows
  long ld;                               // floats per input row
  long Tf;                               // analysis frames per row (T_max + 2)
  int S, Lc;                             // segment and chunk length in output frames
  const int* len;                        // R ints on the device
  const float* w;                        // window
  const float2* tw;                      // twiddles
  float2* D;                             // (R, Tf, nb) or null
  float* A2;                             // (R, Tf, nb)
  uint32_t* TH;                          // (R, Tf, nb)
  int* own;                              // (R, Tf, nb)
  uint32_t* Rseg;                        // (R, S, nb): R_j of the segment's frames
  uint32_t* Rcarry;                      // (R, nb): R at the segment's first frame
  int* par;                              // (R, nch, nb), nch = ceil(S / Lc)
  uint32_t* off;                         // (R, nch, nb)
  uint32_t* Rstart;                      // (R, nch + 1, nb)
  float* fr;                             // (R, S + 3, N)
  float* tmp3;                           // (R, 3, N): the carried frames on their way to the front
};
// bytes of the arrays above for one row (x and y planes not counted)
size_t fx_stretch_row_bytes(const FxStretchGeom& g, long Tf, int S, int Lc, bool want_D);

// analysis of all rows: D (optional), A2, TH, then own
void launch_stretch_analysis(const FxStretchDev& d, const float* rows, hipStream_t s, hipEvent_t* ev);
// the segment of output frames [s0, s0 + S): scan (R_s0 from Rcarry, which then receives R at the next segment's start),
// inverse transforms, and the overlap-add of every sample the segment completes into y (R rows, ld_y apart).
// ev (optional, 4 events): recorded behind the scan, the inverse transforms and the overlap-add (ev[0] in front)
void launch_stretch_segment(const FxStretchDev& d, long s0, float* y, long ld_y, hipStream_t s, hipEvent_t* ev);

// ---- audio.hip: the resampler of stage 14 on one channel plane (float32 in and out, the sum in double, kaiser_hq)
void launch_resample_plane_f32(const ResampleFilter& f, const float* x, long n, float* y, long n_out, hipStream_t s);
void resample_plane_host(int sr_in, int sr_out, const float* x, long n, float* y, long n_out);

// ---- host twin: one channel, x (n) -> y (fx_stretch_len).  Optional taps: D (T + 2, nb) float pairs, own and TH (T + 2, nb),
// R (J, nb)
void fx_stretch_host(const float* x, long n, int sr, long P, long Q, float* y, float* D, int32_t* own, uint32_t* TH, uint32_t* R);
// own of one frame from its A2 (13.2), shared by the twin and the tests of the rule
void fx_stretch_own_host(const float* A2, int nb, int32_t* own);

}  // namespace rvcx
