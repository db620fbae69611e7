"""CPU: the host twin of include/rvcx.h stages 13 and 14 (rvcx_fx_stretch_host, rvcx_fx_pitch_shift_host: no context, no
GPU) against the float64 restatement of tests/stretch_reference.py, link by link so that a near-tie in a peak decision cannot
decide a test: owners from the twin's own D, the integer recurrence from the twin's own owners and phases, the waveform from
the twin's own D, owners, phases and R; then the stage whole, the identity at P = Q, the skip rule, the errors, the length
formulas and the peak rules on built spectra.

Shapes: sr = 8000 (N = 512, H = 128, nb = 257), lengths 1, 127, 128, 511, 512, 513 and 4000, P / 8000 in {8000, 4000, 16000,
9514, 7551} (every frame once, skipped by two, used twice, mixed steps)."""
import ctypes as C

import numpy as np
import pytest

import stretch_reference as R
from stretch_reference import rms, signal, sine_peak_hz, tones, unit_diff

SR = 8000
RATIOS = (8000, 4000, 16000, 9514, 7551)
LENGTHS = (1, 127, 128, 511, 512, 513, 4000)

# TH of the twin (atan2f, then rint in double) against float64 atan2 of the same float32 D, in units of 2^-32 turn: measured
# 166 on this file's signals -- one float32 step of an angle near pi is 2^-22 rad = 163 units, which is what atan2f may be off
# by.  Bar 3x, condition 2^-20 turn.
BAR_TH, CONDITION_TH = 500, 1 << 12
# waveform of the twin against the float64 synthesis from the twin's own D, own, TH and R, relative to the item's peak:
# measured 6.0e-8, the rounding of y to float32 (2^-24) and nothing else.  Bar 3x, condition 1e-4.
BAR_Y, CONDITION_Y = 2e-7, 1e-4
# the stage whole against the restatement that starts from x (its own rfft, its own atan2): relative RMS difference measured
# 7.7e-7 (a phase unit is 1.5e-9 rad; 166 of them on a partial move it by 2.4e-7).  Bar 3x, condition the project's 1e-3.
BAR_E2E, CONDITION_E2E = 2.5e-6, 1e-3
assert BAR_TH <= CONDITION_TH and BAR_Y <= CONDITION_Y and BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


@pytest.mark.parametrize("P", RATIOS)
def test_twin_against_restatement_link_by_link(P):
    L = _L()
    worst = dict(th=0, y=0.0)
    for i, n in enumerate(LENGTHS):
        x = signal(n, 11 + i)
        y, t = L.fx_stretch_host(x, SR, P, SR, taps=True)
        T, J = R.frames(n, SR, P, SR)
        assert y.shape == (R.stretch_len(n, P, SR),) and t["D"].shape == (T + 2, 257, 2) and t["R"].shape == (J, 257)
        D32 = R.pairs_to_complex(t["D"])
        assert not D32[T:].any() and not t["TH"][T:].any()                     # frames T and T + 1 are all zero
        dd = np.abs(R.analysis(x, SR) - D32.astype(np.complex128)).max()
        assert dd <= 1e-6 * max(np.abs(D32).max(), 1e-30) + 1e-30, (n, dd)     # D is the float64 transform rounded once
        assert np.array_equal(t["own"], R.owners(D32)), n
        worst["th"] = max(worst["th"], unit_diff(t["TH"], R.th_of(D32, as_float32=False)))
        assert np.array_equal(t["R"], R.scan(t["own"], t["TH"], J, P, SR)), n
        ref = R.stretch(x, SR, P, SR, D32=D32, own=t["own"], TH=t["TH"], R=t["R"])["y"]
        worst["y"] = max(worst["y"], float(np.abs(y - ref).max()) / 0.5)
    print(f"P {P}: TH {worst['th']} units, waveform {worst['y']:.3e} of the peak")
    assert worst["th"] <= BAR_TH and worst["y"] <= BAR_Y, worst


def test_stage_whole_identity_level_and_pitch():
    """the three signals of 16000 samples at every shift: twin against the all-float64 restatement, level kept within
    0.98 .. 1.02 (measured with the real resampler: 0.9912 .. 1.0008), the sine's peak within 0.5 Hz of 440 P / sr (measured
    0.002 Hz); P = Q returns the input to rounding"""
    L = _L()
    worst, lo, hi, hz = 0.0, 9.0, 0.0, 0.0
    for name, x in tones().items():
        x = x.astype(np.float32)
        n = x.shape[0]
        y = L.fx_stretch_host(x, SR, SR, SR)
        assert np.abs(y - x).max() <= 1e-5 * np.abs(x).max(), name
        for s in (-12, -5, 0.37, 3, 7, 12):
            yh, yr = L.fx_pitch_shift_host(x, SR, s), R.pitch_shift(x, SR, s)
            assert yh.shape == x.shape
            worst = max(worst, rms(yh - yr) / rms(yr))
            ratio = rms(yh[2000:n - 2000]) / rms(x[2000:n - 2000])
            lo, hi = min(lo, ratio), max(hi, ratio)
            if name == "sine":
                hz = max(hz, abs(sine_peak_hz(yh, SR) - 440.0 * R.pitch_ratio(SR, s) / SR))
    print(f"twin vs float64: {worst:.3e} relative RMS; level {lo:.4f} .. {hi:.4f}; sine peak off by {hz:.4f} Hz")
    assert worst <= BAR_E2E and 0.98 <= lo and hi <= 1.02 and hz <= 0.5, (worst, lo, hi, hz)


def test_stereo_is_the_twin_per_channel():
    L = _L()
    x = np.stack([signal(1000, 3), signal(1000, 4)], axis=1)
    y = L.fx_stretch_host(x, SR, 9514, SR)
    z = L.fx_pitch_shift_host(x, SR, -5)
    for c in range(2):
        assert np.array_equal(y[:, c], L.fx_stretch_host(np.ascontiguousarray(x[:, c]), SR, 9514, SR))
        assert np.array_equal(z[:, c], L.fx_pitch_shift_host(np.ascontiguousarray(x[:, c]), SR, -5))


def test_skip_rule():
    L = _L()
    x = signal(777, 5)
    assert L.fx_pitch_ratio(SR, 0.0) == SR and L.fx_pitch_ratio(SR, 1e-4) == SR and L.fx_pitch_ratio(SR, 12) == 2 * SR
    for s in (0.0, 1e-4, -1e-4):                      # P == sr: the output is the input bit for bit
        assert np.array_equal(L.fx_pitch_shift_host(x, SR, s).view(np.uint32), x.view(np.uint32))
    assert not np.array_equal(L.fx_pitch_shift_host(x, SR, 0.02), x)


def test_errors_write_nothing():
    L = _L()
    lib = L.lib()
    x = signal(600, 6)
    y = np.full(2400, 7.0, np.float32)

    def refused(rc, what):
        assert rc == -1 and what in (lib.rvcx_last_error(None) or b"").decode(), (rc, lib.rvcx_last_error(None))
        assert (y == 7.0).all()

    def shift(s, sr=SR, ch=1):
        return lib.rvcx_fx_pitch_shift_host(x.ctypes.data, 600 // max(ch, 1), ch, sr, C.c_double(s), y.ctypes.data, None, None, None, None)

    def stretch(P, Q, sr=SR, ch=1):
        return lib.rvcx_fx_stretch_host(x.ctypes.data, 600 // max(ch, 1), ch, sr, P, Q, y.ctypes.data, None, None, None, None)

    refused(shift(12.01), "semitones")
    refused(shift(-13.0), "semitones")
    refused(shift(float("nan")), "finite")
    refused(shift(float("inf")), "finite")
    refused(shift(3.0, sr=7000), "sample rate")
    refused(shift(3.0, sr=8050), "sample rate")
    refused(shift(3.0, ch=3), "channels")
    refused(stretch(3999, 8000), "Q / 2 <= P")
    refused(stretch(16001, 8000), "Q / 2 <= P")
    refused(stretch(1, 0), "Q")
    refused(stretch(1 << 20, (1 << 20) + 1), "Q")
    refused(stretch(8000, 8000, sr=200000), "sample rate")
    refused(stretch(8000, 8000, ch=0), "channels")
    # 2^30 frames stretched by two no longer fit the int lengths of the rows: refused before anything is read
    refused(lib.rvcx_fx_stretch_host(x.ctypes.data, 1 << 30, 1, SR, 16000, 8000, y.ctypes.data, None, None, None, None), "2^31")
    assert L.fx_stretch_len(100, 3999, 8000) == -1 and L.fx_pitch_ratio(SR, 12.5) == -1
    with pytest.raises(L.RvcxError):
        L.fx_stretch_frames(100, SR, 1, 3)


def test_length_formulas():
    L = _L()
    for sr, N in ((8000, 512), (16000, 1024), (44100, 2048), (48000, 2048), (192000, 8192)):
        assert R.geometry(sr)[0] == N
        for n in (1, N // 4 - 1, N // 4, 12345):
            for s in (-12, -5, 0.37, 3, 12):
                P = R.pitch_ratio(sr, s)
                assert L.fx_pitch_ratio(sr, s) == P
                assert L.fx_stretch_frames(n, sr, P, sr) == R.frames(n, sr, P, sr) + (N,)
                assert L.fx_stretch_len(n, P, sr) == R.stretch_len(n, P, sr) == (n * P + sr // 2) // sr
    assert L.fx_stretch_len(3, 1, 2) == 2 and L.fx_stretch_len(3, 2, 1) == 6 and L.fx_stretch_len(1, 7551, 8000) == 1
    assert L.fx_stretch_chunk() >= 1


def _own(mag):
    """own of a built spectrum from the twin and from the restatement (real bins: equal magnitudes give equal A2)"""
    L = _L()
    D = np.asarray(mag, np.float32).astype(np.complex64)
    got = L.fx_stretch_own_host(D)
    assert np.array_equal(got, R.own_of(R.a2_of(D)))
    return got


def _tent(nb, peaks, level=1.0):
    """a floor that falls away from the nearest of `peaks` (so that no floor bin is a peak), and `level` at the peaks"""
    k = np.arange(nb)
    m = 0.1 - 1e-4 * np.abs(k[:, None] - np.asarray(peaks)[None, :]).min(axis=1)
    m[list(peaks)] = level
    return m


def test_peak_rules_on_built_spectra():
    """13.2 on built spectra.  The rule is > towards the two lower bins and >= towards the two upper ones, a neighbour outside
    counting as smaller.  Read literally it makes bin 0 of a flat non-zero spectrum a peak (its lower neighbours lie outside,
    its upper ones are equal) and the LOWER bin of a two-bin plateau the peak; the sentence that introduced these cases said
    "no peak" and "the upper bin".  The rule is the definition; these are its results in the twin and in the restatement (the
    device's owner kernel is compared with the restatement on real spectra: link 2 of tests/test_gpu_pitch.py)."""
    nb = 257
    k = np.arange(nb)
    # an all-zero frame has no peak: own = identity
    assert np.array_equal(_own(np.zeros(nb)), k)
    # a flat non-zero spectrum: bin 0 alone is a peak
    assert np.array_equal(_own(np.ones(nb)), np.zeros(nb, np.int32))
    # a floor without a peak of its own: everything goes to the one true peak
    assert np.array_equal(_own(_tent(nb, [100])), np.full(nb, 100))
    # a plateau of two equal bins: one peak, the lower bin (50 >= 51 holds, 51 > 50 does not)
    assert np.array_equal(_own(_tent(nb, [50, 51])), np.full(nb, 50))
    # a bin at equal distance between two peaks goes to the lower one
    own = _own(_tent(nb, [40, 50]))
    assert own[45] == 40 and own[46] == 50 and own[44] == 40 and own[0] == 40 and own[nb - 1] == 50
    assert set(own.tolist()) == {40, 50}
    # peaks at bins 0 and nb - 1
    own = _own(_tent(nb, [0, nb - 1]))
    assert own[0] == 0 and own[nb - 1] == nb - 1 and own[128] == 0 and own[129] == nb - 1 and set(own.tolist()) == {0, nb - 1}
    # equal bins two apart: 62 > 60 fails, 60 >= 62 holds -- only 60 is a peak
    m = _tent(nb, [60, 62])
    m[61] = 0.05
    assert np.array_equal(_own(m), np.full(nb, 60))
    # the second neighbours count: a bin below its second lower neighbour is no peak
    m = _tent(nb, [80])
    m[82], m[81] = 0.9, 0.01           # 82 > 81 holds, 82 > 80 fails
    assert np.array_equal(_own(m), np.full(nb, 80))


def test_zero_frame_between_loud_ones():
    """0.2 s of exact zeros in the middle: the frames inside have A2 = 0, TH = 0 and own = identity, on both sides, and the
    recurrence passes through them"""
    L = _L()
    x = signal(8000, 9)
    x[3000:4600] = 0.0
    y, t = L.fx_stretch_host(x, SR, 9514, SR, taps=True)
    D32 = R.pairs_to_complex(t["D"])
    quiet = [f for f in range(t["own"].shape[0]) if not D32[f].any()]
    assert len(quiet) >= 8 + 2
    for f in quiet:
        assert np.array_equal(t["own"][f], np.arange(257)) and not t["TH"][f].any()
    assert np.array_equal(t["own"], R.owners(D32))
    assert np.array_equal(t["R"], R.scan(t["own"], t["TH"], t["R"].shape[0], 9514, SR))
    ref = R.stretch(x, SR, 9514, SR, D32=D32, own=t["own"], TH=t["TH"], R=t["R"])["y"]
    assert np.abs(y - ref).max() <= BAR_Y * 0.5
    assert np.abs(y[stretch_mid(3000, 4600)]).max() <= 1e-6


def stretch_mid(a, b, P=9514, Q=SR, guard=750):
    """output samples that lie well inside the stretched image of the zero stretch [a, b)"""
    return slice(a * P // Q + guard, b * P // Q - guard)


# ---- the host pass under the sanitizers -----------------------------------------------------------------------------------------
_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "pitch.h"
using namespace rvcx;
int main() {
  double sum = 0.0;
  const int rates[2] = {8000, 48000};
  const long lens[7] = {1, 127, 128, 511, 513, 2049, 4000};
  const double shifts[5] = {-12.0, -5.0, 0.37, 7.0, 12.0};
  for (int sr : rates)
    for (long n : lens)
      for (double s : shifts) {
        const FxStretchGeom g = fx_stretch_geom(sr);
        const long P = fx_pitch_P(sr, s), T = fx_stretch_T(n, g.H), J = fx_stretch_J(T, P, sr), ns = fx_stretch_len(n, P, sr);
        std::vector<float> x((size_t)n), y((size_t)ns + 1), out((size_t)n);
        for (long i = 0; i < n; ++i) x[i] = 0.4f * (float)std::sin(0.05 * i) + 0.1f * (float)std::sin(0.61 * i);
        std::vector<float> D((size_t)(T + 2) * g.nb * 2);
        std::vector<int32_t> own((size_t)(T + 2) * g.nb);
        std::vector<uint32_t> TH((size_t)(T + 2) * g.nb), R((size_t)J * g.nb);
        fx_stretch_host(x.data(), n, sr, P, sr, y.data(), D.data(), own.data(), TH.data(), R.data());
        fx_stretch_host(x.data(), n, sr, P, sr, y.data(), nullptr, nullptr, nullptr, nullptr);
        const long no = std::min<long>(resample_out_len(ns, (int)P, sr), n);
        resample_plane_host((int)P, sr, y.data(), ns, out.data(), no);
        for (long i = 0; i < no; ++i) sum += out[i];
      }
  std::printf("PITCH_HOST_ASAN_OK %.6f\n", sum);
  return 0;
}
"""


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """the host pass of pitch.hip and audio.hip with a main of its own, linked with the sanitizers against tools/hipstub"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not shutil.which("hipcc") or not os.path.exists(clang):
        pytest.skip("no hipcc / ROCm clang++ here")
    csrc = os.path.join(root, "polgen-rvc_amd", "csrc")
    main = tmp_path / "pitch_main.hip"
    main.write_text(_MAIN)
    exe = tmp_path / "pitch_asan"
    fatbins = tmp_path / "fatbins.c"
    # host pass only (no device code is built), the sanitizers named for the host side alone
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    flags = ["--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wno-pass-failed", "-Wno-unused-result", "-fno-omit-frame-pointer",
             *san, "-I", csrc]
    objs = []
    for src in (os.path.join(csrc, "pitch.hip"), os.path.join(csrc, "audio.hip"), str(main),
                os.path.join(root, "tools", "hipstub", "hipstub.cpp")):
        obj = tmp_path / (os.path.basename(src) + ".o")
        subprocess.run(["hipcc", *flags, "-x", "hip", "-c", src, "-o", str(obj)], check=True, capture_output=True, text=True, timeout=600)
        objs.append(str(obj))
    nm = subprocess.run(["nm", *objs], check=True, capture_output=True, text=True).stdout
    names = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    fatbins.write_text("".join(f"char {n}[64] = {{0}};\n" for n in names))
    link = [clang, "-fsanitize=address,undefined", "-fno-gpu-sanitize", *objs, "-x", "c", str(fatbins), "-o", str(exe)]    # host objects only
    subprocess.run(link, check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PITCH_HOST_ASAN_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
