"""CPU: include/rvcx.h stages 9 - 12 -- the host twins against the float64 restatement (tests/loudness_reference.py), the
conformance signals of BS.1770 / EBU Tech 3341, the limiter's guarantee, the refusals, and the twins under ASan + UBSan in a
stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import loudness_reference as R
import polgen_rvc_amd  # noqa: F401
from polgen_rvc_amd import _lib, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# |L(host twin) - L(float64 restatement)|: measured 4.5e-14 LU at worst over the cases below (LABNOTES 21: both sides run
# the recurrence in double on the same float32 samples and differ by the order of operations); the bar is 3x that, and the
# condition is a tenth of a meter's display step.
BAR_LU = 1.35e-13
CONDITION_LU = 0.01
assert BAR_LU <= CONDITION_LU


def _clip(index, seconds, sr, channels):
    x = S.make_clip(index, seconds, sr)
    return x if channels == 1 else np.stack([x, 0.7 * S.make_clip(index + 1, seconds, sr)], axis=1).astype(np.float32)


def test_kweight_coefficients_are_the_recommendations_table():
    c = _lib.fx_kweight_coeffs(48000)
    assert np.all(np.abs(c - R.TABLE_48K) <= 1e-12 * np.abs(R.TABLE_48K)), c - R.TABLE_48K
    for sr in (8000, 44100, 192000):
        assert np.all(np.abs(_lib.fx_kweight_coeffs(sr) - R.kweight_coeffs(sr)) <= 1e-12)


@pytest.mark.parametrize("sr", [8000, 44100, 48000, 192000])
@pytest.mark.parametrize("channels", [1, 2])
def test_loudness_host_vs_float64(sr, channels):
    x = _clip(3, 2.0, sr, channels)
    L, mom = _lib.fx_loudness_host(x, sr, momentary=True)
    Lr, momr = R.loudness(x, sr)
    d, dm = abs(L - Lr), float(np.abs(mom.astype(np.float64) - momr.astype(np.float32)).max())
    print(f"sr {sr} C {channels}: L {L:.6f} ref {Lr:.6f} |dL| {d:.3e}  momentary max |dl| {dm:.3e}")
    assert mom.shape == momr.shape == (_lib.fx_momentary_len(x.shape[0], sr),)
    assert d <= BAR_LU and dm <= BAR_LU + 4e-6        # + the float32 rounding of a value of up to 64 dB in magnitude


def test_conformance_997_hz_left_only():
    x = R.sine(997.0, 5.0, 48000, 0.0)
    x[:, 1] = 0.0
    L = _lib.fx_loudness_host(x, 48000)
    assert abs(L - (-3.01)) <= 0.01 and abs(R.loudness(x, 48000)[0] - (-3.01)) <= 0.01, L


@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_conformance_ebu_tech_3341(case):
    x, want = R.ebu_case(case)
    L = _lib.fx_loudness_host(x, 48000)
    print(f"EBU 3341 case {case}: {L:.4f} LUFS (float64 restatement {R.loudness(x, 48000)[0]:.4f})")
    assert abs(L - want) <= 0.1, L


def test_short_and_silent_items_read_minus_infinity():
    assert _lib.fx_loudness_host(np.ones(3199, np.float32), 8000) == -np.inf
    assert _lib.fx_loudness_host(np.zeros(16000, np.float32), 8000) == -np.inf
    assert np.isfinite(_lib.fx_loudness_host(np.ones(3200, np.float32), 8000))
    assert _lib.fx_loudness_host(np.zeros(0, np.float32), 8000) == -np.inf


def test_true_peak_taps_and_phase_zero():
    taps = _lib.fx_truepeak_taps()
    assert np.abs(taps - R.interp_taps()[1:]).max() <= 2.0 ** -24           # formed in double, rounded once
    x = _clip(5, 0.25, 8000, 2)
    tp, p = _lib.fx_truepeak_host(x, want_p=True)
    assert np.all(p >= np.abs(x).max(axis=1))                       # phase 0 is the sample itself
    tpr, pr = R.true_peak(x)
    assert np.abs(p - pr).max() <= 24 * 2.0 ** -23 * np.abs(x).max() * np.abs(R.interp_taps()).sum(axis=1).max()
    assert abs(tp - tpr) <= 1e-4
    # an impulse: x[n - m] is the impulse at m = n - 30, so the phases at n are half the taps of index n - 18, exactly
    d = np.zeros(64, np.float32)
    d[30] = 0.5
    _, pd = _lib.fx_truepeak_host(d, want_p=True)
    want = np.zeros(64, np.float32)
    want[18:42] = 0.5 * np.abs(taps).max(axis=0)
    want[30] = 0.5
    assert np.array_equal(pd, want)


def test_true_peak_between_the_samples():
    sr = 48000
    x = R.sine(sr / 4.0, 0.1, sr, 0.0, phase=np.pi / 4, channels=1)[:, 0]
    # 5 ms raised-cosine edges: a tone switched on at full level is not band-limited, and its edge overshoots (0.108 dBTP on
    # the float64 restatement as well); the statement is about the tone
    edge = np.hanning(2 * 240 + 1)[:240].astype(np.float32)
    x[:240] *= edge
    x[-240:] *= edge[::-1]
    tp = _lib.fx_truepeak_host(x)
    assert abs(R.true_peak(x)[0]) <= 0.01
    sample_peak = 20 * np.log10(np.abs(x).max())
    print(f"sr/4 tone at 45 degrees: sample peak {sample_peak:.4f} dB, true peak {tp:.4f} dBTP")
    assert abs(sample_peak - (-3.01)) <= 0.01 and abs(tp) <= 0.01
    assert _lib.fx_truepeak_host(np.zeros(100, np.float32)) == -np.inf


@pytest.mark.parametrize("sr", [8000, 48000])
def test_limiter_gain_never_exceeds_the_bound(sr):
    x = R.limiter_signal(sr)
    ceiling = -1.0
    c = np.float32(10.0 ** (ceiling / 20.0))
    _, p = _lib.fx_truepeak_host(x, want_p=True)
    y, s = _lib.fx_limit_host(x, sr, ceiling)
    with np.errstate(divide="ignore"):
        r = np.minimum(np.float32(1.0), c / p)
    assert r.dtype == np.float32 and np.all(s <= r), float((s - r).max())
    assert np.abs(y).max() <= float(c) * (1 + 2.0 ** -22)
    assert np.array_equal(y, x * s) and s.min() < 0.5
    print(f"sr {sr}: W {int(2 * sr / 1000)}, min s {s.min():.4f}, output true peak {_lib.fx_truepeak_host(y):.4f} dBTP "
          f"for a {ceiling} dB ceiling")
    # float64 restatement of the gain curve from the same p
    W = int(2.0 * sr / 1000.0)
    rr = np.concatenate([np.minimum(1.0, float(c) / np.maximum(p.astype(np.float64), 1e-300)), np.ones(W)])
    g = np.lib.stride_tricks.sliding_window_view(rr, W + 1).min(axis=1)
    e, prev, cr = np.zeros(len(g)), 0.0, float(_lib.fx_cte(100.0, sr))
    for i, u in enumerate(1.0 - g):
        prev = u if u > prev else u + cr * (prev - u)
        e[i] = prev
    q = np.concatenate([np.full(W, 1.0 - e[0]), 1.0 - e])
    s64 = np.lib.stride_tricks.sliding_window_view(q, W + 1).mean(axis=1)
    assert np.abs(s - s64).max() <= 1e-5


def test_limiter_passes_a_signal_under_the_ceiling_bit_for_bit():
    x = (0.5 * _clip(7, 0.5, 8000, 2)).astype(np.float32)
    assert _lib.fx_truepeak_host(x) < -1.0
    y, s = _lib.fx_limit_host(x, 8000, -1.0)
    assert y.tobytes() == x.tobytes() and np.all(s == 1.0)


def test_master_host_reaches_the_target():
    sr = 8000
    v, m = _clip(1, 3.0, sr, 2), (0.1 * _clip(9, 2.5, sr, 2)).astype(np.float32)
    out, rep = _lib.fx_master_host(v, m, sr, -23.0, 2.0, -1.0)
    print(rep)
    assert out.shape == (v.shape[0], 2) and out.dtype == np.int16
    if rep["min_gain"] == 1.0:
        assert abs(rep["lufs"] - (-23.0)) <= 0.1
    L = _lib.fx_loudness_host(out.astype(np.float32) / 32768.0, sr)
    assert abs(L - rep["lufs"]) <= 0.01 and rep["true_peak_db"] <= -1.0 + 0.1
    _, rep0 = _lib.fx_master_host(v, np.zeros((0, 2), np.float32), sr, -23.0, 0.0, -1.0)
    assert rep0["instrumental_lufs"] == -np.inf and abs(rep0["mix_lufs"] - (-23.0)) <= 1e-3


def test_refusals_write_nothing():
    x = np.full(4000, 0.25, np.float32)
    y = np.full(4000, 7.0, np.float32)
    for kw in (dict(sr=7999), dict(sr=48050), dict(ceiling_db=0.5), dict(ceiling_db=np.nan), dict(lookahead_ms=11.0),
               dict(lookahead_ms=-1.0), dict(release_ms=np.inf), dict(release_ms=-2.0)):
        args = dict(sr=8000, ceiling_db=-1.0, lookahead_ms=2.0, release_ms=100.0)
        args.update(kw)
        with pytest.raises(_lib.RvcxError):
            _lib.fx_limit_host(x, out=y, **args)
        assert np.all(y == 7.0), kw
    with pytest.raises(_lib.RvcxError):
        _lib.fx_loudness_host(x, 8001)
    with pytest.raises(_lib.RvcxError):
        _lib.fx_loudness_host(np.zeros((100, 3), np.float32), 8000)
    with pytest.raises(_lib.RvcxError):
        _lib.fx_kweight_coeffs(500)
    out = np.full((4000, 2), 5, np.int16)
    st = np.stack([x, x], axis=1)
    for kw in (dict(target_lufs=1.0), dict(ceiling_dbtp=0.1), dict(vocal_offset_lu=np.nan), dict(target_lufs=-np.inf), dict(sr=100)):
        args = dict(sr=8000, target_lufs=-16.0, vocal_offset_lu=0.0, ceiling_dbtp=-1.0)
        args.update(kw)
        with pytest.raises(_lib.RvcxError):
            _lib.fx_master_host(st, st, out=out, **args)
        assert np.all(out == 5), kw


_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "effects.h"
using namespace rvcx;
int main() {
  const int rates[3] = {8000, 44100, 192000};
  const long lens[] = {0, 1, 3, 11, 12, 13, 25, 799, 3199, 3200, 3999, 4000, 4097};
  double sum = 0.0;
  for (int sr : rates) {
    const FxKWeight k = fx_kweight(sr);
    for (long n : lens)
      for (int C = 1; C <= 2; ++C) {
        std::vector<float> x((size_t)n * C), y((size_t)n * C), g((size_t)n), p((size_t)n), mom((size_t)fx_momentary_len(n, sr));
        for (size_t i = 0; i < x.size(); ++i) x[i] = 0.9f * std::sin(0.37f * (float)i) + ((i % 97) == 3 ? 1.5f : 0.f);
        const double L = fx_loudness_host(k, x.data(), n, C, sr, mom.data());
        if (std::isfinite(L)) sum += L;
        sum += fx_truepeak_host(x.data(), n, C, p.data());
        fx_limit_host(x.data(), n, C, sr, -1.0, 2.0, 100.0, y.data(), g.data(), nullptr, nullptr);
        fx_limit_host(x.data(), n, C, sr, -6.0, 0.0, 0.0, y.data(), nullptr, nullptr, nullptr);
        if (C == 2) {
          std::vector<int16_t> out((size_t)n * 2);
          double rep[7];
          fx_master_host(x.data(), n, x.data(), n / 2, sr, -16.0, 1.0, -1.0, out.data(), rep);
          fx_master_host(x.data(), n, nullptr, 0, sr, -23.0, 0.0, -3.0, out.data(), nullptr);
        }
      }
  }
  std::printf("LOUDNESS_HOST_ASAN_OK %.6f %d\n", sum, (int)fx_tp_taps().h[0][0]);
  return 0;
}
"""


def test_host_twins_are_clean_under_asan_and_ubsan(tmp_path):
    """the host pass of loudness.hip and effects.hip with a main of its own, linked with the sanitizers against tools/hipstub"""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "polgen-rvc_amd", "csrc")
    main = tmp_path / "loudness_main.hip"
    main.write_text(_MAIN)
    exe = tmp_path / "loudness_asan"
    fatbins = tmp_path / "fatbins.c"
    # host pass only (no device code is built), the sanitizers named for the host side alone
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    flags = ["--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wno-pass-failed", "-Wno-unused-result", "-fno-omit-frame-pointer",
             *san, "-I", csrc]
    objs = []
    for src in (os.path.join(csrc, "loudness.hip"), os.path.join(csrc, "effects.hip"), str(main),
                os.path.join(ROOT, "tools", "hipstub", "hipstub.cpp")):
        obj = tmp_path / (os.path.basename(src) + ".o")
        subprocess.run(["hipcc", *flags, "-x", "hip", "-c", src, "-o", str(obj)], check=True, capture_output=True, text=True, timeout=600)
        objs.append(str(obj))
    nm = subprocess.run(["nm", *objs], check=True, capture_output=True, text=True).stdout
    names = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    fatbins.write_text("".join(f"char {n}[64] = {{0}};\n" for n in names))
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no ROCm clang++ here")
    link = [clang, "-fsanitize=address,undefined", "-fno-gpu-sanitize", *objs, "-x", "c", str(fatbins), "-o", str(exe)]    # host objects only
    subprocess.run(link, check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LOUDNESS_HOST_ASAN_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
