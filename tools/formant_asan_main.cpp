// Stand-alone sanitizer pass over the host twins of include/rvcx.h stages 17 and 18 (CPU only; `make host-asan-formant` builds
// it against build/asan/librvcx_asan.so with AddressSanitizer + UBSan and runs it).  It walks the shapes at which the twin
// takes another path: one sample, H - 1, H, a length that is no multiple of the hop, every N from 512 to 8192, nc = 1 and
// nc = N / 8, 0 and 16 iterations, both ends of ratio, a source, stereo, the taps, the skip and a few refusals.  The arrays
// are exactly as long as the header says, so that a write or read past them is an error here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rvcx.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "formant_asan_main: %s\n", what);
    ++failures;
  }
}

static std::vector<float> tone(int64_t n, int channels, int sr, unsigned seed) {
  std::vector<float> x((size_t)n * channels);
  unsigned s = seed * 2654435761u + 1u;
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < channels; ++c) {
      s = s * 1664525u + 1013904223u;
      const double noise = ((double)(s >> 8) / 16777216.0 - 0.5) * 0.02;
      x[(size_t)i * channels + c] = (float)(0.3 * std::sin(6.283185307179586 * (220.0 + 70.0 * c) * (double)i / sr) +
                                            0.1 * std::sin(6.283185307179586 * 1500.0 * (double)i / sr) + noise);
    }
  return x;
}

static rvcx_fx_formant_params params(int sr, int channels) {
  rvcx_fx_formant_params p;
  p.sample_rate = sr, p.channels = channels;
  p.ratio = 1.26f, p.amount = 1.f, p.quefrency_ms = 1.5f, p.iterations = 8, p.max_gain_db = 24.f, p.keep_energy = 1;
  return p;
}

static void run(int sr, int64_t n, int channels, rvcx_fx_formant_params p, bool with_src, bool taps) {
  int64_t T = 0;
  int32_t N = 0, nc = 0;
  expect(rvcx_fx_formant_frames(n, sr, p.quefrency_ms, &T, &N, &nc) == 0, "fx_formant_frames refused a valid shape");
  const size_t nb = (size_t)N / 2 + 1;
  const std::vector<float> x = tone(n, channels, sr, 1), src = tone(n, channels, sr, 2);
  std::vector<float> y((size_t)n * channels, 7.f);
  std::vector<float> D, E, Es, g, s;
  if (taps) D.resize((size_t)T * nb * 2), E.resize((size_t)T * nb), Es.resize((size_t)T * nb), g.resize((size_t)T * nb), s.resize((size_t)T);
  const int rc = rvcx_fx_formant_host(x.data(), n, with_src ? src.data() : nullptr, &p, y.data(), taps ? D.data() : nullptr,
                                      taps ? E.data() : nullptr, taps ? Es.data() : nullptr, taps ? g.data() : nullptr,
                                      taps ? s.data() : nullptr);
  expect(rc == 0, "fx_formant_host refused a valid call");
  for (float v : y) expect(std::isfinite(v), "a sample of y is not finite");
  for (float v : g) expect(std::isfinite(v) && v > 0.f, "a gain is not positive");
}

int main() {
  for (int sr : {8000, 16000, 44100, 96000, 192000}) {
    int64_t T = 0;
    int32_t N = 0, nc = 0;
    rvcx_fx_formant_frames(1, sr, 1.5f, &T, &N, &nc);
    const int H = N / 4;
    for (int64_t n : {(int64_t)1, (int64_t)H - 1, (int64_t)H, (int64_t)5 * H + 3, (int64_t)2 * N + 1}) {
      run(sr, n, 1, params(sr, 1), false, true);
      run(sr, n, 1, params(sr, 1), true, true);
    }
    run(sr, 3 * (int64_t)H + 1, 2, params(sr, 2), true, false);
    rvcx_fx_formant_params p = params(sr, 1);
    p.quefrency_ms = (float)(1000.0 * 1.01 / sr), p.iterations = 0, p.ratio = 0.5f;                     // nc = 1
    run(sr, 2 * (int64_t)N, 1, p, false, true);
    p.quefrency_ms = (float)(1000.0 * (N / 8 + 0.01) / sr), p.iterations = 16, p.ratio = 2.f, p.keep_energy = 0;   // nc = N / 8
    run(sr, 2 * (int64_t)N, 1, p, true, true);
  }
  {  // the envelope of one frame, alone
    for (int N : {512, 8192}) {
      std::vector<float> L((size_t)N / 2 + 1), E((size_t)N / 2 + 1);
      for (size_t k = 0; k < L.size(); ++k) L[k] = (float)(-5.0 + 3.0 * std::sin(0.37 * (double)k));
      expect(rvcx_fx_formant_envelope_host(L.data(), N, N / 8, 16, E.data()) == 0, "envelope_host refused nc = N / 8");
      expect(rvcx_fx_formant_envelope_host(L.data(), N, 1, 0, E.data()) == 0, "envelope_host refused nc = 1");
      expect(rvcx_fx_formant_envelope_host(L.data(), N, N / 8 + 1, 8, E.data()) == -1, "envelope_host took nc > N / 8");
    }
  }
  {  // stage 18, the skips and the refusals (nothing is written)
    const int sr = 8000;
    const int64_t n = 1000;
    const std::vector<float> x = tone(n, 2, sr, 3);
    std::vector<float> y((size_t)n * 2, 7.f);
    rvcx_fx_formant_params p = params(sr, 2);
    expect(rvcx_fx_pitch_shift_formant_host(x.data(), n, 2, sr, 4.0, &p, y.data()) == 0, "stage 18 refused a valid call");
    expect(rvcx_fx_pitch_shift_formant_host(x.data(), n, 2, sr, -7.0, nullptr, y.data()) == 0, "stage 18 refused null parameters");
    expect(rvcx_fx_pitch_shift_formant_host(x.data(), n, 2, sr, 0.0, &p, y.data()) == 0 && y == x, "stage 18 at 0 is not the input");
    p.ratio = 1.f;
    y.assign(y.size(), 7.f);
    expect(rvcx_fx_formant_host(x.data(), n, nullptr, &p, y.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0 && y == x,
           "the skip at ratio 1 is not the input");
    y.assign(y.size(), 7.f);
    p.ratio = 2.5f;
    expect(rvcx_fx_formant_host(x.data(), n, nullptr, &p, y.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "ratio 2.5 was taken");
    p = params(sr, 2), p.quefrency_ms = 9.f;
    expect(rvcx_fx_formant_host(x.data(), n, nullptr, &p, y.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "nc > N / 8 was taken");
    p = params(sr, 2);
    expect(rvcx_fx_formant_host(x.data(), 0, nullptr, &p, y.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "n = 0 was taken");
    for (float v : y) expect(v == 7.f, "a refusal wrote to y");
  }
  if (failures) return 1;
  std::puts("formant_asan_main: ok");
  return 0;
}
