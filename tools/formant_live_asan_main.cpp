// Stand-alone sanitizer pass over the host twin of include/rvcx.h stage 19 (CPU only; `make host-asan-formant-live` builds it
// against build/asan/librvcx_asan.so with AddressSanitizer + UBSan and runs it).  It walks the shapes at which the twin takes
// another path: no complete frame (n < N / 2), exactly one, a length that ends inside a hop, n shorter and longer than the
// delay, every N from 512 to 4096, nc = 1 and nc = N / 8, 0 and 16 iterations, both ends of ratio, the two ways of being off,
// with and without the taps, the frame count and a few refusals.  The arrays are exactly as long as the header says, so that a
// write or read past them is an error here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rvcx.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "formant_live_asan_main: %s\n", what);
    ++failures;
  }
}

static std::vector<float> tone(int64_t n, int sr, unsigned seed) {
  std::vector<float> x((size_t)n);
  unsigned s = seed * 2654435761u + 1u;
  for (int64_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    const double noise = ((double)(s >> 8) / 16777216.0 - 0.5) * 0.02;
    x[(size_t)i] = (float)(0.3 * std::sin(6.283185307179586 * 220.0 * (double)i / sr) +
                           0.1 * std::sin(6.283185307179586 * 1500.0 * (double)i / sr) + noise);
  }
  return x;
}

static rvcx_live_formant_params params() {
  rvcx_live_formant_params p;
  p.sample_rate = 0, p.channels = 0;
  p.ratio = 1.26f, p.amount = 1.f, p.quefrency_ms = 1.5f, p.iterations = 8, p.max_gain_db = 24.f, p.keep_energy = 1;
  return p;
}

static void run(int sr, int64_t n, rvcx_live_formant_params p, bool taps, bool off) {
  int64_t T = 0;
  int32_t N = 0, nc = 0;
  expect(rvcx_stream_formant_frames(n, sr, p.quefrency_ms, &T, &N, &nc) == 0, "stream_formant_frames refused a valid shape");
  expect(rvcx_stream_formant_delay(sr) == N, "the delay is not N");
  expect(T == (n >= N / 2 ? (n - N / 2) / (N / 4) + 1 : 0), "the frame count is not stage 16's");
  const size_t nb = (size_t)N / 2 + 1;
  const std::vector<float> x = tone(n, sr, 1);
  std::vector<float> y((size_t)n, 7.f);
  std::vector<float> D, E, g, s;
  if (taps) D.resize((size_t)T * nb * 2), E.resize((size_t)T * nb), g.resize((size_t)T * nb), s.resize((size_t)T);
  const int rc = rvcx_fx_formant_live_host(x.data(), n, sr, &p, y.data(), taps ? D.data() : nullptr, taps ? E.data() : nullptr,
                                           taps ? g.data() : nullptr, taps ? s.data() : nullptr);
  expect(rc == 0, "fx_formant_live_host refused a valid call");
  for (int64_t i = 0; i < n; ++i) {
    expect(std::isfinite(y[(size_t)i]), "a sample of y is not finite");
    if (i < N) expect(y[(size_t)i] == 0.f, "a sample in front of the delay is not zero");
    else if (off) expect(y[(size_t)i] == x[(size_t)(i - N)], "off is not the delayed input");
  }
  for (float v : g) expect(std::isfinite(v) && v > 0.f, "a gain is not positive");
}

int main() {
  for (int sr : {3200, 8000, 16000, 24100, 48000, 96000, 192000}) {
    const int N = rvcx_stream_formant_delay(sr), H = N / 4;
    expect(N >= 512 && N <= 4096 && 48L * N >= sr, "N is not stage 16's");
    for (int64_t n : {(int64_t)1, (int64_t)N / 2 - 1, (int64_t)N / 2, (int64_t)N / 2 + H - 1, (int64_t)N / 2 + H, (int64_t)N - 1,
                      (int64_t)N, (int64_t)N + 1, (int64_t)2 * N + 5 * H + 3}) {
      run(sr, n, params(), true, false);
      run(sr, n, params(), false, false);
    }
    rvcx_live_formant_params p = params();
    p.sample_rate = sr, p.channels = 1;
    p.quefrency_ms = (float)(1000.0 * 1.01 / sr), p.iterations = 0, p.ratio = 0.5f;                     // nc = 1
    run(sr, 2 * (int64_t)N + 7, p, true, false);
    p.quefrency_ms = (float)(1000.0 * (N / 8 + 0.01) / sr), p.iterations = 16, p.ratio = 2.f, p.keep_energy = 0;   // nc = N / 8
    run(sr, 2 * (int64_t)N + 7, p, true, false);
    p = params(), p.amount = 0.f;
    run(sr, 2 * (int64_t)N + 7, p, true, true);
    p = params(), p.ratio = 1.f;
    run(sr, 2 * (int64_t)N + 7, p, false, true);
  }
  {  // the refusals (nothing is written)
    const int sr = 16000;
    const int64_t n = 2000;
    const std::vector<float> x = tone(n, sr, 3);
    std::vector<float> y((size_t)n, 7.f);
    rvcx_live_formant_params p = params();
    p.ratio = 2.5f;
    expect(rvcx_fx_formant_live_host(x.data(), n, sr, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "ratio 2.5 was taken");
    p = params(), p.quefrency_ms = 4.1f;                    // nc = 65 > N / 8 = 64 on the live grid
    expect(rvcx_fx_formant_live_host(x.data(), n, sr, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "nc > N / 8 was taken");
    int64_t T = 0;
    expect(rvcx_stream_formant_frames(n, sr, 4.1f, &T, nullptr, nullptr) == -1, "stream_formant_frames took nc > N / 8");
    p = params(), p.sample_rate = 8000;
    expect(rvcx_fx_formant_live_host(x.data(), n, sr, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "another rate was taken");
    p = params(), p.channels = 2;
    expect(rvcx_fx_formant_live_host(x.data(), n, sr, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "two channels were taken");
    p = params();
    expect(rvcx_fx_formant_live_host(x.data(), 0, sr, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "n = 0 was taken");
    expect(rvcx_fx_formant_live_host(x.data(), n, 22050, &p, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "22050 Hz was taken");
    expect(rvcx_fx_formant_live_host(x.data(), n, sr, nullptr, y.data(), nullptr, nullptr, nullptr, nullptr) == -1, "null parameters were taken");
    expect(rvcx_stream_formant_delay(22050) == -1, "the delay of a refused rate");
    for (float v : y) expect(v == 7.f, "a refusal wrote to y");
  }
  if (failures) return 1;
  std::puts("formant_live_asan_main: ok");
  return 0;
}
