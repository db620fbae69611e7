// Post-production (include/rvcx.h "post-production"): the vocal effects chain and the cover mix.  effects.hip holds the
// kernels, their launchers, the coefficient formulas and the sequential host twins; api_fx.hip the entry points;
// effects_live.hip the board of a live session (state carried across blocks); effects_device.h the step functions all share.
//
// Device layout: planar rows.  Row r = item * C + channel holds len[r] samples at the front of ld floats (ld a multiple of
// kFxChunk, the tail zero).  Every kernel takes one row per blockIdx.y and cuts it into chunks counted from the row's first
// sample, so a row's result depends on nothing but the row (and, for the reverb, its partner).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace rvcx {

constexpr int kFxChunk = 1024;       // samples a lane walks alone in the scan and follower kernels (rvcx_fx_chunk)

struct FxBiquad {                    // normalised by a0; transposed direct form II
  float b0, b1, b2, a1, a2;
};
// kind 0: the first-order high-pass of stage 1 (b2 = a2 = 0), 1: low shelf, 2: high shelf (audio-EQ-cookbook, rvcx.h)
FxBiquad fx_coeffs(int kind, int sr, double fc, double Q, double gain_db);
float fx_cte(double ms, int sr);                         // exp(-2 pi 1000 / (ms sr)), 0 below 1e-3 ms
inline int fx_delay(int sr, int D) { return (int)((int64_t)sr * D / 44100); }
inline bool fx_rate_ok(int sr) { return sr >= 8000 && sr <= 192000 && sr % 100 == 0; }

struct FxReverb {                    // what the three reverb kernels need, formed on the host in double, rounded once
  int comb[2][8], ap[2][4];          // delays in samples per side
  float fb, d, omd;                  // feedback, damping d and 1 - d
  float w1, w2, dry2;                // 1.5 wet (1 + width), 1.5 wet (1 - width), 2 dry
};
FxReverb fx_reverb_setup(int sr, double room, double damping, double wet, double dry, double width);

struct FxChorus {
  double w, srk, centre, dep10;      // 2 pi rate / sr, sr / 1000, centre delay in ms, 10 depth
  float fb, mix, omm;                // feedback, mix and 1 - mix
  int T;                             // floor(tau_min) - 1: samples of one row that do not depend on each other
};
FxChorus fx_chorus_setup(int sr, double rate, double depth, double centre_ms, double feedback, double mix);

// ---- launchers (all on stream s; R rows, ld floats apart; len: R ints on the device) -----------------------------------
// stage (item b: n[b] frames of C interleaved floats at b * ld * C) <-> planar rows; the planar tail [len, ld) is zeroed
void launch_fx_deinterleave(const float* stage, float* rows, const int* len, int B, int C, long ld, hipStream_t s);
void launch_fx_interleave(const float* rows, float* stage, const int* len, int B, int C, long ld, hipStream_t s);
// y = biquad(x) per row: zero-state chunk responses, one carry scan per row, the chunks again from their true states.
// scratch: 2 * R * (ld / kFxChunk) float2
void launch_fx_biquad(const FxBiquad& q, const float* x, float* y, const int* len, int R, long ld, float* scratch,
                      hipStream_t s);
// env = follower(|x| or x^2) per row (rvcx.h), by relaxation over chunks; returns the passes that ran a chunk.
// state: 3 * R * (ld / kFxChunk) floats + 64 ints.  Synchronises s once per pass.
int launch_fx_follower(const float* x, float* env, const int* len, const int* len_host, int R, long ld, int square,
                       int sqrt_out, float c_att, float c_rel, float* state, hipStream_t s);
// y = x * g(env): gate = 0 the compressor's gain, 1 the noise gate's; thr linear, expo the exponent of e / thr
void launch_fx_gain(const float* x, const float* env, float* y, int R, long ld, int gate, float thr, float expo, hipStream_t s);
// Freeverb on stereo items (rows 2 b, 2 b + 1): combs (B * 2 * 8 rows of ld) -> ap (B * 2 rows) -> y
void launch_fx_reverb(const FxReverb& rv, const float* x, float* combs, float* ap, float* y, const int* len, int B, long ld,
                      hipStream_t s);
// d: R rows of ld floats of scratch (the delay line; unused when feedback == 0)
void launch_fx_chorus(const FxChorus& ch, const float* x, float* d, float* y, const int* len, int R, long ld, hipStream_t s);
// out[i] = sat(gain(v[i]) + gain(inst[i] or 0)): nv / ni interleaved int16 samples
void launch_fx_mix(const int16_t* v, long nv, const int16_t* inst, long ni, double gv, double gi, int16_t* out, hipStream_t s);

// ---- sequential float32 twins on the host ------------------------------------------------------------------------------
void fx_highpass_host(const FxBiquad& q, const float* x, long n, float* y);
void fx_biquad_host(const FxBiquad& q, const float* x, long n, float* y);
void fx_follower_host(const float* x, long n, int square, int sqrt_out, float c_att, float c_rel, float* env);
void fx_gain_host(const float* x, const float* env, long n, int gate, float thr, float expo, float* y);
void fx_comb_host(const float* in, long n, int D, float fb, float d, float* out);
void fx_allpass_host(const float* in, long n, int D, float* out);
void fx_chorus_host(const FxChorus& ch, const float* x, long n, float* y);
void fx_mix_host(const int16_t* v, long nv, const int16_t* inst, long ni, double gv, double gi, int16_t* out);
// the whole reverb on one stereo item, x and y (n, 2) interleaved: fx_comb_host / fx_allpass_host and the mix FMAs
void fx_reverb_host(const FxReverb& rv, const float* x, long n, float* y);

// ---- loudness, true peak, limiter, master (loudness.hip; rvcx.h stages 9 - 12) ------------------------------------------------
// The K-weighting filter keeps DOUBLE coefficients and state on both sides: 1 + a1 + a2 of its high-pass is 1.6e-6 at
// 192 kHz, below what float32 coefficients resolve.
struct FxKWeight {
  double sb0, sb1, sb2, sa1, sa2;    // shelf
  double hb0, hb1, hb2, ha1, ha2;    // high-pass (b = 1, -2, 1, not normalised)
};
FxKWeight fx_kweight(int sr);
constexpr int kTpTaps = 24;          // taps of each non-trivial phase of the 4x interpolator (12 samples either way)
struct FxTpTaps {
  float h[3][kTpTaps];               // h[p - 1][j] = h(j - 12 + p / 4): the tap of x[n + 12 - j]; accumulated j = 0 .. 23
};
const FxTpTaps& fx_tp_taps();
inline long fx_momentary_len(long n, int sr) { return std::max(0L, n / (sr / 10) - 3); }
inline int fx_lookahead(int sr, double ms) { return (int)(ms * sr / 1000.0); }
constexpr int kFxMaxLookahead = 1920;   // 10 ms at 192 kHz: what the sliding-minimum tile holds

// L per item from planar rows (len: B * C ints, a row per channel).  scratch: fx_loudness_scratch_bytes.  lufs: B doubles on
// the device; mom (optional): B rows of mom_ld floats.  ev (optional, 4 events): behind local, carry, apply + energy, gates.
size_t fx_loudness_scratch_bytes(int B, int C, long ld, int sr);
void launch_fx_loudness(const FxKWeight& k, const float* rows, const int* len, int B, int C, long ld, int sr, void* scratch,
                        double* lufs, float* mom, long mom_ld, hipStream_t s, hipEvent_t* ev);
// p[n] (optional: B rows of ld, one per ITEM) and the bits of max p per item (peak: B words, zeroed here)
void launch_fx_truepeak(const float* rows, const int* len, int B, int C, long ld, float* p, uint32_t* peak, hipStream_t s);
// s[n] of stage 11 from p: B rows of ld (ilen / ilen_host: B ints); u, e: B x ld scratch; state as launch_fx_follower's;
// smin: the bits of min s per item (B words, set here).  Returns the follower's passes.
int launch_fx_limit_gain(const float* p, const int* ilen, const int* ilen_host, int B, long ld, float c, int W, float c_rel,
                         float* u, float* e, float* state, float* sgain, uint32_t* smin, hipStream_t s);
// y = x s (sgain null: s = 1) -> planar y (optional, may be x), interleaved float stage (optional), interleaved int16 (optional)
void launch_fx_limit_apply(const float* rows, const float* sgain, const int* len, int B, int C, long ld, float* y, float* stage,
                           int16_t* pcm, hipStream_t s);
// v = fl(gv v) + fl(gi inst) over len_v (inst zero past len_i); gv, gi: B floats on the device
void launch_fx_master_mix(float* v, const float* inst, const int* len_v, const int* len_i, const float* gv, const float* gi, int B,
                          int C, long ld, hipStream_t s);
void launch_fx_scale(float* rows, const float* g, int B, int C, long ld, hipStream_t s);   // rows of item b times g[b]

// host twins: x (n, C) interleaved.  mom (optional): fx_momentary_len floats.  p (optional): n floats.
double fx_loudness_host(const FxKWeight& k, const float* x, long n, int C, int sr, float* mom);
float fx_truepeak_host(const float* x, long n, int C, float* p);                  // max p[n] (0 when n == 0)
void fx_limit_gain_host(const float* p, long n, float c, int W, float c_rel, float* sgain);
double fx_db20(float peak);                                   // 20 log10, -infinity at 0
double fx_gain_to(double target, double L);                   // 10^((target - L) / 20); 1 when L is not finite
// stage 11 whole (peak_out: max p in front of the stage, smin_out: min s; both optional) and stage 12 whole, one item
void fx_limit_host(const float* x, long n, int C, int sr, double ceiling_db, double lookahead_ms, double release_ms, float* y,
                   float* gain, float* peak_out, float* smin_out);
void fx_master_host(const float* vocal, long n_v, const float* inst, long n_i, int sr, double target_lufs, double vocal_offset_lu,
                    double ceiling_dbtp, int16_t* out, double* report7);

// ---- the board inside a live session (effects_live.hip; rvcx.h "live post-production") --------------------------------------
// Every stage runs sequentially in sample order from state the session carries, so a step's output is the stage on the whole
// signal whatever the cut.  State exists twice: a step reads one set and writes the other.
inline bool fx_live_rate_ok(int sr, bool low) { return fx_rate_ok(sr) || (low && sr >= 3200 && sr < 8000 && sr % 100 == 0); }

// what a step launches: on[k] says whether stage k + 1 runs; the rest is formed on the host in double and rounded once
struct FxLivePlan {
  bool on[7] = {false, false, false, false, false, false, false};
  FxBiquad hp{}, lo{}, hi{};
  float comp_ca = 0, comp_cr = 0, comp_thr = 1, comp_expo = 0;
  float gate_c0 = 0, gate_c50 = 0, gate_ca = 0, gate_cr = 0, gate_thr = 1, gate_expo = 0;
  FxReverb rv{};
  FxChorus ch{};
};

// A stream's state, in floats from its start (fixed by rate and block, whatever the parameters): the scalar slots below, then
// the delay lines (each indexed by the global sample index mod its length) and one chorus ring per channel.
constexpr int kFxlBiquad = 0;      // stage j in {high-pass, low shelf, high shelf}, channel c: (s1, s2) at 4 j + 2 c
constexpr int kFxlFollow = 12;     // compressor e at c, gate r at 2 + c, gate e at 4 + c
constexpr int kFxlLast = 18;       // the combs' one-pole states at 8 side + comb
constexpr int kFxlLines = 34;
struct FxLiveLayout {
  int comb[2][8], ap[2][4];        // (a side's all-pass lines follow each other)
  long chorus[2];
  long cap;                        // chorus ring: sr + 2 (the longest delay the board accepts, 1000 ms) + two blocks
  long per_stream;
};
FxLiveLayout fx_live_layout(int sr, long block);

struct FxLive {
  int S = 0, sr = 0;
  long B = 0;                      // samples per block and row
  FxLiveLayout L{};
  FxLivePlan plan;
  float* state[2] = {nullptr, nullptr};   // (S, L.per_stream) each
  float* work = nullptr;                  // fx_live_work_floats(S, B): two planes of 2 S rows and the 16 S comb rows
};
inline size_t fx_live_work_floats(int S, long B) { return (size_t)20 * S * B; }
// One block of every stream through the stages that are on.  src: S rows of B frames of C interleaved floats, src_stride
// floats apart; out: S rows of (B, 2), out_stride floats apart.  Reads state[cur], writes state[cur ^ 1]; step: blocks since
// sample 0.  No host synchronisation.  ev (optional, 8 events): recorded in front of stage 1 and behind every stage -- the
// load is counted with the high-pass, the interleave with the chorus.
void fx_live_step(const FxLive& f, const float* src, long src_stride, int C, int cur, uint64_t step, float* out,
                  long out_stride, hipStream_t s, hipEvent_t* ev);

}  // namespace rvcx
