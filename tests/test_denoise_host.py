"""CPU: include/rvcx.h stage 15 (noise reduction) -- the host twin and the smoothing twin against the float64 restatement
(tests/denoise_reference.py), the skip rule, every error, and the behaviour conditions on the restatement and on the twin.

The twin transforms and synthesises in double and applies the float32 roundings of D, A2, S, l and m as defined, so it
differs from the restatement (float64 behind A2) by float32 rounding only.  Bars from the number formats: S is a sum of at
most 129 x 33 non-negative float32 terms taken one by one, relative error <= (129 + 33 + 3) x 2^-24 = 1e-5 (measured 3.8e-7);
m follows S through a sigmoid whose slope is at most 1 / (4 knee_db) per dB, or slope / 4 per unit of r: with the float32
log10f, expf and the relative 1e-5 of S the bound is 1e-4 (measured 5e-7); y is rounded once, so its relative RMS difference
is bounded by that of m plus 2^-24, 1e-4 (measured 8.5e-8)."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as R
from stretch_reference import rms, signal

SR = 8000
BAR_S, BAR_M, BAR_Y = 1e-5, 1e-4, 1e-4


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def _twin(x, sr, noise=None, **kw):
    L = _L()
    return L.fx_denoise_host(x, sr, L.FxDenoiseParams.make(sr, 1, **kw), noise=noise)


@pytest.mark.parametrize("mode", (0, 1))
def test_host_twin_against_the_restatement(mode):
    L = _L()
    worst = dict(S=0.0, m=0.0, y=0.0, stat=0.0, b=0.0)
    for i, n in enumerate((1, 127, 128, 511, 512, 513, 4000)):
        x = signal(n, 10 + i)
        for clip in ((None, signal(700, 30 + i)) if mode == 0 else (None,)):
            y, t = L.fx_denoise_host(x, SR, L.FxDenoiseParams.make(SR, 1, mode=mode), noise=clip, taps=True)
            T, N, nf, nt = L.fx_denoise_frames(n, SR)
            assert (T, N) == (R.frames(n, SR), 512) and (nf, nt) == R.half_widths(SR) and t["D"].shape == (T, 257, 2)
            ref = R.denoise(x, SR, noise=clip, mode=mode)
            D32 = R.pairs_to_complex(t["D"])
            assert np.array_equal(D32, ref["D"])              # both round the float64 transform once
            worst["S"] = max(worst["S"], float(np.abs(t["S"] - ref["S"]).max() / ref["S"].max()),
                             float((np.abs(t["S"] - ref["S"]) / np.maximum(ref["S"], 1e-30)).max()))
            if mode == 0:
                worst["stat"] = max(worst["stat"], float(np.abs(t["mu"] - ref["mu"]).max()), float(np.abs(t["sd"] - ref["sd"]).max()))
            else:
                worst["b"] = max(worst["b"], float((np.abs(t["b"] - ref["b"]) / np.maximum(ref["b"], 1e-30)).max()))
            worst["m"] = max(worst["m"], float(np.abs(t["m"] - ref["m"]).max()))
            worst["y"] = max(worst["y"], rms(y - ref["y"]) / rms(ref["y"]))
    print(f"mode {mode}: {worst}")
    assert worst["S"] <= BAR_S and worst["m"] <= BAR_M and worst["y"] <= BAR_Y, worst
    assert worst["stat"] <= 1e-4 and worst["b"] <= 1e-5, worst     # dB and relative: float32 log10f, sqrtf behind the S above


def test_stereo_twin_is_its_two_channels():
    L = _L()
    a, b, za, zb = signal(1500, 1), signal(1500, 2), signal(400, 3), signal(400, 4)
    st, clip = np.stack([a, b], axis=1), np.stack([za, zb], axis=1)
    p = L.FxDenoiseParams.make(SR, 2, mode=0)
    y = L.fx_denoise_host(st, SR, p, noise=clip)
    assert np.array_equal(y[:, 0], L.fx_denoise_host(a, SR, p, noise=za)) and np.array_equal(y[:, 1], L.fx_denoise_host(b, SR, p, noise=zb))


@pytest.mark.parametrize("nf,nt", ((0, 0), (1, 0), (0, 1), (16, 2), (64, 16)))
@pytest.mark.parametrize("T", (1, 2, 40))
def test_smoothing_twin_against_the_restatement(nf, nt, T):
    """T <= nt included: there the edge rule does all the work"""
    L = _L()
    A2 = (np.random.default_rng(T * 100 + nf + nt).standard_normal((T, 257)) ** 2).astype(np.float32)
    A2[:, 100:110] = 0.0
    S, ref = L.fx_denoise_smooth_host(A2, nf, nt), R.smooth(A2, nf, nt)
    err = float((np.abs(S - ref) / np.maximum(ref, 1e-30)).max())
    print(f"nf {nf} nt {nt} T {T}: {err:.3e}")
    assert err <= BAR_S
    if nf == 0 and nt == 0:
        assert np.array_equal(S, A2)                           # neither axis is touched
    one = L.fx_denoise_smooth_host(np.ones((T, 257), np.float32), nf, nt)
    assert np.array_equal(one, np.ones((T, 257), np.float32))  # renormalised at every edge: a wrong edge weight moves this by 1e-2


def test_strength_zero_returns_the_input():
    L = _L()
    x = np.stack([signal(999, 5), signal(999, 6)], axis=1)
    for mode in (0, 1):
        y = L.fx_denoise_host(x, SR, L.FxDenoiseParams.make(SR, 2, mode=mode, strength=0.0))
        assert np.array_equal(y.view(np.uint32), x.view(np.uint32))


def test_errors_write_nothing():
    L = _L()
    lib = L.lib()
    x, z = signal(600, 6), signal(300, 7)
    y = np.full(600, 7.0, np.float32)

    def refused(what, n=600, noise=None, n_noise=0, sr=SR, ch=1, **kw):
        p = L.FxDenoiseParams.make(sr, ch, **kw)
        rc = lib.rvcx_fx_denoise_host(x.ctypes.data, n, None if noise is None else noise.ctypes.data, n_noise, C.byref(p),
                                      y.ctypes.data, None, None, None, None, None, None)
        msg = (lib.rvcx_last_error(None) or b"").decode()
        assert rc == -1 and what in msg, (rc, msg, kw)
        assert (y == 7.0).all()

    for name, bad in (("strength", (-0.01, 1.01)), ("n_std", (-1.0, 10.5)), ("knee_db", (0.05, 21.0)),
                      ("thresh_mult", (-0.1, 20.5)), ("slope", (0.05, 101.0)), ("time_constant_s", (0.01, 31.0))):
        for v in bad:
            refused(name, **{name: v})
        for v in (float("nan"), float("inf")):
            refused("finite", **{name: v})
    refused("negative", freq_smooth_hz=-1.0)
    refused("negative", time_smooth_ms=-1.0)
    refused("finite", freq_smooth_hz=float("inf"))
    refused("64 bins", freq_smooth_hz=65 * 2 * SR / 512.0)              # nf = 65
    refused("16 frames", time_smooth_ms=17 * 2000 * 128 / SR + 1.0)     # nt = 17
    refused("mode", mode=2)
    refused("sample rate", sr=7000)
    refused("channels", ch=3)
    refused("frames", n=0)
    refused("noise clip", mode=1, noise=z, n_noise=300)                 # the adaptive mode takes none
    refused("noise clip", mode=0, noise=z, n_noise=0)
    with pytest.raises(L.RvcxError, match="channel"):                   # a clip of another channel count
        L.fx_denoise_host(x, SR, L.FxDenoiseParams.make(SR, 1, mode=0), noise=np.stack([z, z], axis=1))
    with pytest.raises(L.RvcxError):
        L.fx_denoise_smooth_host(np.ones((3, 257), np.float32), 65, 0)
    with pytest.raises(L.RvcxError):
        L.fx_denoise_frames(0, SR)
    assert L.fx_denoise_host(x, SR, L.FxDenoiseParams.make(SR, 1, freq_smooth_hz=64 * 2 * SR / 512.0)).shape == (600,)   # nf = 64 runs


# Behaviour: the conditions of the issue (level within 0.99 .. 1.01, SNR gain >= 6 dB, noise only >= 12 dB, quiet >= 30 dB,
# burst >= 0.7, steady tone <= 0.05), measured with the committed restatement; the twin gives the same figures to every digit
# shown.   sr     level   SNR in -> out (dB)   noise only (dB)   quiet (dB)   burst   steady tone
#          8000   1.0008  25.01 -> 33.30       18.75             38.08        0.815   0.0085
#          48000  0.9996  24.94 -> 38.41       16.45             36.35        0.798   0.0080
# A steady tone falls to 0.008 of its level in the adaptive mode: it becomes the floor.  That is the documented property of
# the mode (rvcx.h), and the last condition states it.
@pytest.mark.parametrize("sr", (8000, 48000))
@pytest.mark.parametrize("side", ("restatement", "twin"))
def test_behaviour(sr, side):
    fn = _twin if side == "twin" else (lambda x, sr, noise=None, **kw: R.denoise(x, sr, noise=noise, **kw)["y"])
    f = R.behaviour(fn, sr)
    print(f"{side} at {sr} Hz: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    R.check_behaviour(f)
