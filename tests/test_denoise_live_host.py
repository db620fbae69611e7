"""CPU: live noise reduction (include/rvcx.h stage 16) on the host -- the twin rvcx_fx_denoise_live_host against the all-float64
restatement tests/denoise_live_reference.py, the delay rule, causality, the degenerate widths, strength 0, every refusal and
the behaviour on stage 15's test signal.

Bars.  Twin against float64: 3 x the relative RMS measured at the first run (LABNOTES 24) under the condition <= 1e-3.
Measured: y 2.8e-8 .. 7.95e-8, S 5.5e-8 .. 7.27e-8, f 2.6e-8 .. 4.06e-8, m 1.5e-7 .. 2.00e-7 over 8 and 48 kHz and both modes
(the twin rounds A2, F, S and m to float32 as defined, the restatement only D and A2).  Behaviour at 16 kHz with the defaults
(strength 0.9), after the first second: the pauses between the bursts 18.49 dB down, the bursts at 0.99853 of their level;
bars at the measured attenuation less 3 dB and at +-0.5 dB around the measured level.  With stage 15's strength of 0.7 the
pauses come out 10.07 dB down -- less than the 12 dB the issue asks of the defaults, hence 0.9."""
import ctypes as C

import numpy as np
import pytest

import denoise_live_reference as R

BARS = dict(y=3 * 7.95e-8, S=3 * 7.27e-8, f=3 * 4.06e-8, m=3 * 2.00e-7)
assert all(v <= 1e-3 for v in BARS.values())
PAUSE_DB, BURST_LEVEL = 18.49, 0.99853
RATES = {4800: 512, 8000: 512, 16000: 512, 44100: 1024, 48000: 1024, 96000: 2048, 192000: 4096}


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def _signal(n, sr, seed):
    """a gliding tone in bursts with pauses of noise alone and a stretch of exact zeros"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    tone = 0.3 * np.sin(2 * np.pi * (220.0 + 60.0 * t) * t) * ((t % 0.4) < 0.22)
    x = tone + 0.01 * g.standard_normal(n)
    x[n // 2:n // 2 + n // 10] = 0.0
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def clip():
    return (0.01 * np.random.default_rng(77).standard_normal(6000)).astype(np.float32)


@pytest.mark.parametrize("sr,n", [(8000, 9600), (48000, 12000)])
@pytest.mark.parametrize("mode", (1, 0))
def test_twin_against_float64(sr, n, mode, clip):
    L = _L()
    x = _signal(n, sr, 3)
    kw = dict(mode=mode, noise=clip) if mode == 0 else dict(mode=1)
    y, t = L.fx_denoise_live_host(x, sr, dict(kw), taps=True)
    r = R.denoise_live(x, sr, **kw)
    T, N, nf, nt = L.stream_denoise_frames(n, sr)
    assert (T, N) == (R.frames(n, sr), R.geometry(sr)[0]) and (nf, nt) == R.half_widths(sr)
    assert t["S"].shape == (T, N // 2 + 1) and y.shape == (n,) and R.rms(y) > 0.02
    assert np.array_equal(t["D"][..., 0] + 1j * t["D"][..., 1], r["D"])           # rounded once from a double transform
    err = dict(y=R.rel(y, r["y"]), S=R.rel(t["S"], r["S"]), m=R.rel(t["m"], r["m"]))
    if mode == 1:
        err["f"] = R.rel(t["f"], r["f"])
    print(f"twin vs float64 at {sr} Hz mode {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= BARS[k], (k, v)


def test_delay_rule():
    L = _L()
    for sr, N in RATES.items():
        assert L.stream_denoise_delay(sr) == N == R.geometry(sr)[0], sr
    for sr in (0, 3100, 22050, 192100, -8000):
        assert L.lib().rvcx_stream_denoise_delay(sr) == -1, sr
        with pytest.raises(L.RvcxError):
            L.stream_denoise_delay(sr)
    # a click leaves N samples later, and nothing leaves in front of sample N
    sr, n = 16000, 4000
    N = L.stream_denoise_delay(sr)
    x = np.zeros(n, np.float32)
    x[1000] = 0.5
    y = L.fx_denoise_live_host(x, sr, dict(strength=0.5))
    assert not y[:N].any() and int(np.argmax(np.abs(y))) == 1000 + N
    assert L.stream_denoise_frames(N // 2 - 1, sr)[0] == 0 and L.stream_denoise_frames(N // 2, sr)[0] == 1
    assert L.stream_denoise_frames(N // 2 + N // 4 - 1, sr)[0] == 1 and L.stream_denoise_frames(N // 2 + N // 4, sr)[0] == 2


def test_the_stage_is_causal():
    """what has left after m samples does not change when more arrive: the twin on a prefix is the prefix of the twin"""
    L = _L()
    sr, n = 8000, 6000
    x = _signal(n, sr, 5)
    y, t = L.fx_denoise_live_host(x, sr, taps=True)
    for m in (1, 255, 256, 700, 3001):
        ym, tm = L.fx_denoise_live_host(x[:m], sr, taps=True)
        assert np.array_equal(ym, y[:m]), m
        Tm = R.frames(m, sr)
        assert tm["S"].shape[0] == Tm and np.array_equal(tm["f"], t["f"][:Tm]) and np.array_equal(tm["m"], t["m"][:Tm]), m


@pytest.mark.parametrize("widths", [dict(freq_smooth_hz=0.0), dict(time_smooth_ms=0.0), dict(freq_smooth_hz=0.0, time_smooth_ms=0.0)])
def test_zero_widths_leave_their_axis_alone(widths):
    L = _L()
    sr, n = 8000, 4800
    x = _signal(n, sr, 9)
    y, t = L.fx_denoise_live_host(x, sr, dict(widths), taps=True)
    r = R.denoise_live(x, sr, **widths)
    nf, nt = L.stream_denoise_frames(n, sr, widths.get("freq_smooth_hz", 500.0), widths.get("time_smooth_ms", 50.0))[2:]
    assert (nf == 0) == ("freq_smooth_hz" in widths) and (nt == 0) == ("time_smooth_ms" in widths)
    if nf == 0 and nt == 0:
        assert np.array_equal(t["S"], R.a2_of(r["D"]).astype(np.float32))       # S is A2 itself
    err = dict(S=R.rel(t["S"], r["S"]), y=R.rel(y, r["y"]), m=R.rel(t["m"], r["m"]))
    print(f"nf {nf} nt {nt}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= BARS[k], (k, v)


def test_strength_zero_is_the_delayed_input(clip):
    L = _L()
    sr, n = 8000, 4800
    x = _signal(n, sr, 11)
    N = L.stream_denoise_delay(sr)
    for kw in (dict(), dict(mode=0, noise=clip)):
        y, t = L.fx_denoise_live_host(x, sr, dict(strength=0.0, **kw), taps=True)
        assert not y[:N].any() and y[N:].tobytes() == x[:n - N].tobytes()
        on = L.fx_denoise_live_host(x, sr, dict(kw), taps=True)[1]
        assert np.array_equal(t["m"], on["m"]) and np.array_equal(t["S"], on["S"])          # analysis and floor keep running
        if not kw:
            assert np.array_equal(t["f"], on["f"]) and np.ptp(t["f"], axis=0).min() > 0.0


def test_refusals_write_nothing(clip):
    L = _L()
    lib = L.lib()
    sr, n = 8000, 2400
    x = _signal(n, sr, 13)
    mark = np.full(n, 123.25, np.float32)

    def call(sr_=sr, noise=None, n_noise=None, sr_field=0, channels=1, n_=n, **over):
        out = mark.copy()
        p = L.LiveDenoiseParams.make(sr_field, **over)
        p.channels = channels
        zn = (0 if noise is None else noise.shape[0]) if n_noise is None else n_noise
        rc = lib.rvcx_fx_denoise_live_host(x.ctypes.data, n_, sr_, None if noise is None else noise.ctypes.data, zn, C.byref(p),
                                           out.ctypes.data, None, None, None, None)
        return rc, out

    nan, inf = float("nan"), float("inf")
    cases = [dict(sr_=22050), dict(sr_=3100), dict(sr_=192100), dict(sr_field=16000), dict(channels=2), dict(mode=2), dict(mode=-1),
             dict(strength=1.5), dict(strength=-0.1), dict(strength=nan), dict(n_std=10.5), dict(knee_db=0.05), dict(knee_db=inf),
             dict(thresh_mult=-1.0), dict(thresh_mult=21.0), dict(slope=0.05), dict(slope=101.0), dict(time_constant_s=0.04),
             dict(time_constant_s=31.0), dict(fall_time_s=0.005), dict(fall_time_s=2.5), dict(fall_time_s=nan),
             dict(time_constant_s=0.1, fall_time_s=0.2), dict(freq_smooth_hz=-1.0), dict(time_smooth_ms=-1.0),
             dict(freq_smooth_hz=65 * 2 * sr / 512.0), dict(time_smooth_ms=33 * 1000.0 * 128 / sr + 1.0), dict(time_smooth_ms=inf),
             dict(mode=0), dict(mode=1, noise=clip), dict(mode=0, noise=clip, n_noise=255), dict(mode=0, noise=clip, n_noise=(1 << 22) + 1),
             dict(n_=0)]
    for k, case in enumerate(cases):
        rc, out = call(**case)
        assert rc == -1 and out.tobytes() == mark.tobytes(), (k, case)
        assert (lib.rvcx_last_error(None) or b"").decode(), k
    # the edges of the ranges run: nf = 64, nt = 32, a clip of one frame, fall_time_s == time_constant_s
    for ok in (dict(freq_smooth_hz=64 * 2 * sr / 512.0), dict(time_smooth_ms=32 * 1000.0 * 128 / sr + 0.5),
               dict(mode=0, noise=clip, n_noise=256), dict(fall_time_s=2.0), dict(sr_field=sr)):
        rc, out = call(**ok)
        assert rc == 0 and np.isfinite(out).all() and out.tobytes() != mark.tobytes(), ok
    with pytest.raises(L.RvcxError, match="needs a noise clip"):
        L.fx_denoise_live_host(x, sr, dict(mode=0))
    with pytest.raises(L.RvcxError, match="unknown value"):
        L.fx_denoise_live_host(x, sr, dict(fall_time=0.1))
    with pytest.raises(L.RvcxError, match="32 frames"):
        L.fx_denoise_live_host(x, sr, dict(time_smooth_ms=1000.0))


def test_behaviour_with_the_defaults():
    """0.25 sin 440 Hz bursts + 0.01 noise at 16 kHz: the pauses go down, the bursts stay"""
    L = _L()
    assert L.LiveDenoiseParams.DEFAULTS == R.DEFAULTS
    twin = R.behaviour(lambda x, sr: L.fx_denoise_live_host(x, sr), 16000)
    ref = R.behaviour(lambda x, sr: R.denoise_live(x, sr)["y"], 16000)
    print(f"pauses {twin[0]:.2f} dB down (restatement {ref[0]:.2f}), bursts at {twin[1]:.5f} ({ref[1]:.5f})")
    for pause_db, level in (twin, ref):
        assert pause_db >= 12.0                                              # the condition on the defaults
        assert pause_db >= PAUSE_DB - 3.0
        assert abs(R.db(level / BURST_LEVEL)) <= 0.5
