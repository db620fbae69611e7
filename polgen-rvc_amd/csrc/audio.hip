// Sample-rate conversion on the device: stands for the two librosa.resample calls of the path --
// load_audio (rvc/lib/my_utils.py:12-13: file rate -> 16 kHz, float64) and VC.pipeline's resample_sr branch
// (rvc/infer/pipeline.py:453-454: tgt_sr -> resample_sr on the float32 output).
//
// librosa.resample's default res_type is "soxr_hq" (librosa >= 0.10; the reference pins no version).  libsoxr is not
// vendored by the reference and its coefficients are not published as a formula, but its HQ recipe is (soxr.c,
// soxr_quality_spec: 20-bit precision): linear phase, pass-band flat to 0.9136 x Nyquist(out), stop-band from 1.0 x
// Nyquist(out) at -120.4 dB.  Round 6 -- the DEFAULT filter here ("kaiser_hq") is a Kaiser-windowed sinc DESIGNED TO THOSE
// TARGETS: cut-off at the middle of the transition band (roll-off 0.9568), beta 12.82 (125 dB), 96 zero crossings per wing
// (the Kaiser length for a 0.0864 x Nyquist transition), 2048 table samples per crossing with linear interpolation
// (table error -141 dB), every tap evaluated at its EXACT table position (p_i = (frac + i scale) 2048: no integer
// table step, so no constant gain error).  Measured (tests/test_resample_spec.py): +-0.001 dB to 7.31 kHz, below
// -127 dB from 8.0 kHz at 44.1 k / 48 k -> 16 k -- inside soxr_hq's published targets; the sample-level difference to
// any other filter meeting them is bounded by the ripple / stop-band figures outside the 7.31 ... 8 kHz transition band.
// resampy's published "kaiser_best" (librosa's default before 0.10: 64 zero crossings, 512 table samples, roll-off
// 0.9475937167399596, beta 14.769656459379492, integer table step int(scale * 512)) stays selectable (RVCX_RESAMPLER=
// kaiser_best, rvcx_resample_f64_kind) in its published arithmetic.  oracle/audio.py restates both in numpy.
//
// One lane per output sample, left wing then right wing; ~2 x 290 taps per sample at 48 -> 16 kHz.
// A 30 s stereo 48 kHz upload becomes 16 kHz mono in ~0.1 ms instead of ~1 s of host time -- at 1000x real time the
// conversion itself takes 30 ms, so a host-side resampler would be the whole request.
//
// Live-stream sessions (rvcx.h, "live streams at the sound card's rate") run the same filter statefully, inside the step:
// per stream a FIFO of past input in double, every output sample computed from its global index with the tap loop the
// one-shot kernel uses (kaiser_exact_taps), so that what a session emits is the one-shot result on the whole signal, delayed
// by stream_resample_delay() samples, however the signal was cut into blocks.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "ops.h"
#include "pitch.h"

namespace rvcx {

namespace {

struct FilterSpec {
  int zeros, precision;
  double rolloff, beta;
  bool exact;          // taps at their exact table positions (kaiser_hq); false: resampy's integer table step
};
constexpr FilterSpec kSpecs[2] = {
    {96, 11, 0.9568, 12.82, true},                                   // 0: kaiser_hq -- designed to soxr_hq's published targets
    {64, 9, 0.9475937167399596, 14.769656459379492, false},          // 1: resampy's published kaiser_best
};

long double bessel_i0(long double x) {          // power series: converges in < 60 terms for x <= 15
  long double s = 1.0L, t = 1.0L;
  const long double q = x * x / 4.0L;
  for (int k = 1; k < 200; ++k) {
    t *= q / ((long double)k * k);
    s += t;
    if (t < s * 1e-22L) break;
  }
  return s;
}

std::vector<double> make_base_window(const FilterSpec& F) {
  const int table = 1 << F.precision, n = F.zeros * table;
  std::vector<double> win((size_t)n + 1);
  const long double i0b = bessel_i0((long double)F.beta);
  const double pi = 3.14159265358979323846;
  for (int i = 0; i <= n; ++i) {
    const double xz = (double)i / table;                          // np.linspace(0, num_zeros, n + 1)
    const double arg = F.rolloff * xz;
    const double sinc = arg == 0.0 ? 1.0 : std::sin(pi * arg) / (pi * arg);
    // np.kaiser(2 n + 1, beta)[n + i]: alpha = n, argument beta * sqrt(1 - (i / n)^2)
    const long double r = (long double)i / n;
    const long double taper = bessel_i0((long double)F.beta * sqrtl(std::max(0.0L, 1.0L - r * r))) / i0b;
    win[i] = (double)taper * (F.rolloff * sinc);
  }
  return win;
}

// the right half of the filter at gain 1, formed once per kind: 2e5 Bessel series in long double take 0.1 s, more than a whole
// stage-14 call on the device
const std::vector<double>& base_window(int kind) {
  if (kind == 0) {
    static const std::vector<double> hq = make_base_window(kSpecs[0]);
    return hq;
  }
  static const std::vector<double> best = make_base_window(kSpecs[1]);
  return best;
}

// interp_win (right half of the filter) and interp_delta (its forward difference), optionally scaled by `gain`
void build_window(int kind, double gain, std::vector<double>& win, std::vector<double>& delta) {
  const FilterSpec& F = kSpecs[kind];
  const int table = 1 << F.precision, n = F.zeros * table, nwin = n + 1;
  win = base_window(kind);
  delta.assign(nwin, 0.0);
  for (double& v : win) v *= gain;            // taper * (rolloff * sinc) * gain, in this order as before
  // exact tap positions: the last tap of a wing can lie within rounding of the window's edge, where a Kaiser window is not
  // zero (1e-8 of the peak) -- the final table sample is zero, so the weight runs out continuously (oracle/audio.py)
  if (F.exact) win[n] = 0.0;
  for (int i = 0; i < n; ++i) delta[i] = win[i + 1] - win[i];
}

// The tap loop of kaiser_hq for ONE output sample at input position `time_register`: tap i of the left wing sits at table
// position (frac + i scale) table (floor + linear interpolation per tap), the left wing stops at input index 0, the right wing
// in front of n_orig.  X(i) is input sample i as a double.  The one-shot kernel and the streaming kernel below both call this
// one function: what a session emits is the one-shot filter, tap for tap.
template <typename TAcc, typename XF>
__host__ __device__ __forceinline__ TAcc kaiser_exact_taps(const ResampleFilter& f, double time_register, long n_orig, XF X) {
  const double* __restrict__ win = f.win;
  const double* __restrict__ delta = f.delta;
  const long n = (long)time_register;
  const double frac = f.scale * (time_register - (double)n);
  TAcc acc = (TAcc)0;
  const double step = f.scale * f.table;
  double p0 = frac * f.table;
  for (long i = 0; i <= n; ++i) {
    const double p = p0 + (double)i * step;
    const long idx = (long)p;
    if (idx >= f.nwin - 1) break;
    const double w = win[idx] + (p - (double)idx) * delta[idx];
    acc = (TAcc)((double)acc + w * X(n - i));
  }
  p0 = (f.scale - frac) * f.table;
  for (long k = 0; n + k + 1 < n_orig; ++k) {
    const double p = p0 + (double)k * step;
    const long idx = (long)p;
    if (idx >= f.nwin - 1) break;
    const double w = win[idx] + (p - (double)idx) * delta[idx];
    acc = (TAcc)((double)acc + w * X(n + k + 1));
  }
  return acc;
}

template <typename TIn, typename TOut, typename TAcc>
__global__ void resample_kernel(const TIn* __restrict__ x, long n_orig, long x_stride, int channels, TOut* __restrict__ y,
                                long n_out, const ResampleFilter f) {
  const long t = blockIdx.x * 256L + threadIdx.x;
  if (t >= n_out) return;
  const double* __restrict__ win = f.win;
  const double* __restrict__ delta = f.delta;
  // `channels` > 1: the input is interleaved (frames, channels) and is averaged on the fly (librosa.to_mono)
  auto X = [&](long i) -> double {
    if (channels == 1) return (double)x[i * x_stride];
    double s = 0.0;
    for (int c = 0; c < channels; ++c) s += (double)x[i * x_stride + c];
    return s / channels;
  };
  const double time_register = (double)t * f.time_increment;
  if (f.exact) {
    y[t] = (TOut)kaiser_exact_taps<TAcc>(f, time_register, n_orig, X);
    return;
  }
  const long n = (long)time_register;
  double frac = f.scale * (time_register - (double)n);
  TAcc acc = (TAcc)0;
  // resampy's published loop: a common fractional offset, an INTEGER table step
  const int index_step = f.index_step;
  double index_frac = frac * f.table;
  int offset = (int)index_frac;
  double eta = index_frac - offset;
  long i_max = min(n + 1, (long)((f.nwin - offset) / index_step));
  for (long i = 0; i < i_max; ++i) {
    const double w = win[offset + i * index_step] + eta * delta[offset + i * index_step];
    acc = (TAcc)((double)acc + w * X(n - i));
  }
  frac = f.scale - frac;
  index_frac = frac * f.table;
  offset = (int)index_frac;
  eta = index_frac - offset;
  const long k_max = min(n_orig - n - 1, (long)((f.nwin - offset) / index_step));
  for (long k = 0; k < k_max; ++k) {
    const double w = win[offset + k * index_step] + eta * delta[offset + k * index_step];
    acc = (TAcc)((double)acc + w * X(n + k + 1));
  }
  y[t] = (TOut)acc;
}

// ---- streaming (live-stream sessions, rvcx.h): per stream a FIFO of the last L = H + B_in mono samples in double
// (the mean over channels is formed once, in double, exactly as X() above forms it; a float32 sample is a double exactly).
// grid-stride over (S, L): dst row = src row moved left by B_in frames, the new block (S rows of B_in interleaved frames,
// x_bs floats apart) mixed and appended.  src != dst: the two sets of a session.
__global__ void stream_fifo_roll_kernel(const double* __restrict__ src, double* __restrict__ dst, const float* __restrict__ x,
                                        long x_bs, int channels, long L, long B_in, long total) {
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long s = idx / L, j = idx - s * L;
    double v;
    if (j < L - B_in) {
      v = src[idx + B_in];
    } else {
      const float* q = x + s * x_bs + (j - (L - B_in)) * channels;
      if (channels == 1) {
        v = (double)q[0];
      } else {
        double a = 0.0;
        for (int c = 0; c < channels; ++c) a += (double)q[c];
        v = a / channels;
      }
    }
    dst[idx] = v;
  }
}

// grid (ceil(B_out / 256), S): lane i of stream s emits global output sample t = t0 + i (0 where t < 0) from the FIFO row,
// whose element 0 is global input sample `base` (negative while the session is young: those indices are never taps, the left
// wing stops at 0) and whose end is the n_recv samples received so far (the right wing stops there).
__global__ void stream_resample_kernel(const double* __restrict__ fifo, long L, long base, long n_recv, long t0,
                                       float* __restrict__ y, long y_bs, long B_out, const ResampleFilter f) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= B_out) return;
  const double* __restrict__ row = fifo + (long)blockIdx.y * L;
  const long t = t0 + i;
  float v = 0.f;
  if (t >= 0) {
    auto X = [&](long g) -> double {
      const long j = g - base;
      return (j >= 0 && j < L) ? row[j] : 0.0;      // (never outside: stream_resampler_plan's H; the test keeps a slip in bounds)
    };
    v = (float)kaiser_exact_taps<double>(f, (double)t * f.time_increment, n_recv, X);
  }
  y[(long)blockIdx.y * y_bs + i] = v;
}

// equal rates: no filter (librosa.resample returns its input), only the mono mix, rounded once to float32
__global__ void stream_mix_kernel(const float* __restrict__ x, long x_bs, int channels, float* __restrict__ y, long y_bs,
                                  long B) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= B) return;
  const float* q = x + (long)blockIdx.y * x_bs + i * channels;
  double a = 0.0;
  for (int c = 0; c < channels; ++c) a += (double)q[c];
  y[(long)blockIdx.y * y_bs + i] = (float)(channels == 1 ? a : a / channels);
}

}  // namespace

long resample_out_len(long n, int sr_in, int sr_out) { return (long)((double)n * ((double)sr_out / (double)sr_in)); }

int resample_default_kind() {
  static const int k = [] {
    const char* e = getenv("RVCX_RESAMPLER");
    return (e && std::string(e) == "kaiser_best") ? 1 : 0;
  }();
  return k;
}

size_t resample_table_doubles(int kind) {
  RVCX_CHECK(kind == 0 || kind == 1, "resample: unknown filter kind");
  return 2 * ((size_t)kSpecs[kind].zeros * ((size_t)1 << kSpecs[kind].precision) + 1);
}

ResampleFilter make_resample_filter_at(double* d, int sr_in, int sr_out, hipStream_t s, int kind) {
  if (kind < 0) kind = resample_default_kind();
  RVCX_CHECK(kind == 0 || kind == 1, "resample: unknown filter kind");
  const FilterSpec& F = kSpecs[kind];
  ResampleFilter f;
  const double ratio = (double)sr_out / (double)sr_in;
  f.scale = std::min(1.0, ratio);
  f.time_increment = 1.0 / ratio;
  f.table = 1 << F.precision;
  f.nwin = F.zeros * f.table + 1;
  f.exact = F.exact ? 1 : 0;
  f.index_step = (int)(f.scale * f.table);
  RVCX_CHECK(f.index_step >= 1, "resample: ratio too small");
  std::vector<double> win, delta;
  build_window(kind, ratio < 1.0 ? ratio : 1.0, win, delta);
  RVCX_HIP(hipMemcpyAsync(d, win.data(), (size_t)f.nwin * sizeof(double), hipMemcpyHostToDevice, s));
  RVCX_HIP(hipMemcpyAsync(d + f.nwin, delta.data(), (size_t)f.nwin * sizeof(double), hipMemcpyHostToDevice, s));
  RVCX_HIP(hipStreamSynchronize(s));          // the host vectors die with this frame
  f.win = d;
  f.delta = d + f.nwin;
  return f;
}

ResampleFilter make_resample_filter(Arena& A, int sr_in, int sr_out, hipStream_t s, int kind) {
  if (kind < 0) kind = resample_default_kind();
  return make_resample_filter_at(A.alloc<double>(resample_table_doubles(kind)), sr_in, sr_out, s, kind);
}

void launch_resample_f64(const ResampleFilter& f, const double* x, long n, int channels, double* y, long n_out,
                         hipStream_t s) {
  if (n_out <= 0) return;
  hipLaunchKernelGGL((resample_kernel<double, double, double>), dim3((unsigned)cdiv64(n_out, 256)), dim3(256), 0, s, x, n,
                     (long)channels, channels, y, n_out, f);
}

void launch_resample_f32(const ResampleFilter& f, const float* x, long n, float* y, long n_out, hipStream_t s) {
  if (n_out <= 0) return;
  // float32 in -> float32 out with a float32 running sum: what the published loop does on a float32 array
  hipLaunchKernelGGL((resample_kernel<float, float, float>), dim3((unsigned)cdiv64(n_out, 256)), dim3(256), 0, s, x, n, 1L, 1,
                     y, n_out, f);
}

// ---- one channel plane, float32 in and out, the running sum in double (rvcx.h stage 14): kaiser_hq, the same tap loop
void launch_resample_plane_f32(const ResampleFilter& f, const float* x, long n, float* y, long n_out, hipStream_t s) {
  RVCX_CHECK(f.exact, "resample plane: kaiser_hq only");
  if (n_out <= 0) return;
  hipLaunchKernelGGL((resample_kernel<float, float, double>), dim3((unsigned)cdiv64(n_out, 256)), dim3(256), 0, s, x, n, 1L, 1,
                     y, n_out, f);
}

// the host path of the same plane: the tables of build_window in host memory, kaiser_exact_taps sample by sample
void resample_plane_host(int sr_in, int sr_out, const float* x, long n, float* y, long n_out) {
  const FilterSpec& F = kSpecs[0];
  const double ratio = (double)sr_out / (double)sr_in;
  std::vector<double> win, delta;
  build_window(0, ratio < 1.0 ? ratio : 1.0, win, delta);
  ResampleFilter f;
  f.scale = std::min(1.0, ratio);
  f.time_increment = 1.0 / ratio;
  f.table = 1 << F.precision;
  f.nwin = (int)win.size();
  f.exact = 1;
  f.win = win.data();
  f.delta = delta.data();
  for (long t = 0; t < n_out; ++t)
    y[t] = (float)kaiser_exact_taps<double>(f, (double)t * f.time_increment, n, [&](long i) { return (double)x[i]; });
}

// ---- streaming: rules, geometry and the two launches of a step
bool stream_rates_ok(int sr_in, int sr_out) {
  auto one = [](int r, int other) { return r > 0 && r % 100 == 0 && r <= 192000 && (r >= 8000 || other < 8000); };
  return one(sr_in, sr_out) && one(sr_out, sr_in);
}

int stream_resample_delay(int sr_in, int sr_out) {
  if (!stream_rates_ok(sr_in, sr_out)) return -1;
  if (sr_in == sr_out) return 0;
  return sr_out > sr_in ? (int)((96L * sr_out + sr_in - 1) / sr_in) : 96;      // ceil(96 max(1, sr_out / sr_in))
}

StreamResamplerPlan stream_resampler_plan(int sr_in, int sr_out, int channels, int block_frames) {
  RVCX_CHECK(stream_rates_ok(sr_in, sr_out) && channels >= 1 && block_frames >= 1, "stream resampler: bad geometry");
  StreamResamplerPlan g;
  g.sr_in = sr_in, g.sr_out = sr_out, g.channels = channels;
  g.B_in = (long)block_frames * (sr_in / 100);
  g.B_out = (long)block_frames * (sr_out / 100);
  g.delay = stream_resample_delay(sr_in, sr_out);
  g.filter = sr_in != sr_out;
  if (!g.filter) return g;
  // History.  Step k (R = (k + 1) B_in frames received) emits t in [k B_out - d, (k + 1) B_out - d).  For t >= 0 the tap loop
  // reads input n - i (left) and n + k' + 1 (right) with n = floor(t inc), inc = sr_in / sr_out, while (frac + i scale) < 96:
  // at most W = ceil(96 / scale) taps per wing, one more if the last bit of p rounds down (its weight is the table's zero end).
  // The computed n is the real floor, or one less where t inc is an integer that rounds below itself; so for the first sample
  // of a step n >= (k B_out - d) inc - 1 = k B_in - d inc - 1 and the lowest index read is >= k B_in - ceil(d inc) - 1 - W.
  // The FIFO's first element is global sample R - L = k B_in - H, so H = ceil(d inc) + W + 2 leaves one sample to spare.
  // No tap lies at or beyond R: the right wing stops in front of n_recv = R (and the delay makes that bound idle).
  const long d_in = ((long)g.delay * sr_in + sr_out - 1) / sr_out;
  const long W = sr_out < sr_in ? (96L * sr_in + sr_out - 1) / sr_out : 96;
  g.H = d_in + W + 2;
  g.L = g.H + g.B_in;
  return g;
}

void launch_stream_resample(const StreamResamplerPlan& g, const ResampleFilter& f, const double* fifo_cur, double* fifo_next,
                            const float* x, long x_bs, float* y, long y_bs, int S, uint64_t step, hipStream_t s) {
  if (!g.filter) {
    hipLaunchKernelGGL(stream_mix_kernel, dim3((unsigned)cdiv64(g.B_out, 256), S), dim3(256), 0, s, x, x_bs, g.channels, y, y_bs,
                       g.B_out);
    return;
  }
  const long tot = (long)S * g.L;
  hipLaunchKernelGGL(stream_fifo_roll_kernel, dim3((unsigned)std::min<long>(cdiv64(tot, 256), 1 << 16)), dim3(256), 0, s,
                     fifo_cur, fifo_next, x, x_bs, g.channels, g.L, g.B_in, tot);
  const long n_recv = ((long)step + 1) * g.B_in;
  hipLaunchKernelGGL(stream_resample_kernel, dim3((unsigned)cdiv64(g.B_out, 256), S), dim3(256), 0, s, fifo_next, g.L,
                     n_recv - g.L, n_recv, (long)step * g.B_out - g.delay, y, y_bs, g.B_out, f);
}

}  // namespace rvcx
