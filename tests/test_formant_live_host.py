"""CPU: include/rvcx.h stage 19 -- the host twin of the live formant shift against the float64 restatement
(tests/formant_live_reference.py) link by link and end to end at 8, 16 and 48 kHz, the behaviour conditions of stage 17 on the
restatement and on the twin at the live geometry, the off rule and the refusals.

Shapes: 8 and 16 kHz (N = 512, H = 128) and 48 kHz (N = 1024): 0.25 s of stretch_reference.signal for the links (60 / 28 / 43
frames), plus n of N / 2 - 1 (no frame), N / 2 (one), N + 3 at 8 kHz; the corners of every parameter on 1500 samples at 8 kHz."""
import ctypes as C

import numpy as np
import pytest

import formant_live_reference as R
import formant_reference as F
from stretch_reference import signal

RATES = (8000, 16000, 48000)
# Bars: 3x the worst case measured on the host twin (LABNOTES 27), the project's rule for stage 17 (tests/test_formant_host.py);
# the conditions are what a wrong link would exceed.  No link lands above stage 17's own bar: the arithmetic is stage 17's at a
# transform no longer than its own.
# 1. |D - float64 rfft| over the frame's largest magnitude: measured 5.54e-8 (the twin transforms in double and rounds once).
BAR_D, CONDITION_D = 1.67e-7, 1e-5
# 2. E against the restatement on the twin's D, absolute (nepers): measured 4.93e-7 (E is rounded to float32 after every lift).
BAR_E, CONDITION_E = 1.48e-6, 1e-3
# 3. g against the restatement on the twin's E, relative: measured 2.82e-7 (W and d rounded to float32, expf; stage 17's twin
#    shows 1.07e-6 on its source rows, which this stage does not have).
BAR_G, CONDITION_G = 8.5e-7, 1e-3
# 4. s from the twin's D and g: equal bit for bit (the sums are double in a defined order).
# 5. y against the float64 synthesis from the twin's D, g and s, over the item's peak: measured 5.93e-8.
BAR_Y, CONDITION_Y = 1.78e-7, 1e-4
# 6. the stage whole against the all-float64 restatement, relative RMS: measured 5.66e-8 (stage 17's twin: 9.2e-8, bar 2.8e-7).
BAR_E2E, CONDITION_E2E = 1.7e-7, 1e-3
assert BAR_D <= CONDITION_D and BAR_E <= CONDITION_E and BAR_G <= CONDITION_G and BAR_Y <= CONDITION_Y and BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def host_links(x, sr, worst, **kw):
    y, t = _L().fx_formant_live_host(x, sr, kw, taps=True)
    return R.check_links(y, t, x, sr, worst, **kw)


def check_bars(worst, what):
    print(f"{what}: D {worst['D']:.3e} of the frame's top, E {worst['E']:.3e}, g {worst['g']:.3e} relative, "
          f"y {worst['y']:.3e} of the peak")
    assert worst["D"] <= BAR_D and worst["E"] <= BAR_E and worst["g"] <= BAR_G and worst["y"] <= BAR_Y, worst


@pytest.mark.parametrize("sr", RATES)
def test_links_and_end_to_end(sr):
    L = _L()
    N = R.geometry(sr)[0]
    assert L.stream_formant_delay(sr) == N == (1024 if sr == 48000 else 512)
    worst = F.new_worst()
    x = signal(sr // 4, 20, sr)
    y = host_links(x, sr, worst, semitones=4.0)
    host_links(signal(sr // 4, 21, sr), sr, worst, semitones=-4.0)
    if sr == 8000:
        for i, n in enumerate((N // 2 - 1, N // 2, N + 3)):
            host_links(signal(n, 22 + i, sr), sr, worst, semitones=4.0)
    check_bars(worst, f"live host twin at {sr} Hz")
    ref = R.formant_live(x, sr, semitones=4.0)
    e2e = R.rel(y, ref["y"])
    print(f"live host twin at {sr} Hz, whole against float64: {e2e:.3e}")
    assert not y[:N].any() and R.rms(y[N:]) > 0.05 and e2e <= BAR_E2E


def test_links_at_the_corners():
    sr = 8000
    assert R.quefrency_bins(sr, 0.125) == (1, True) and R.quefrency_bins(sr, 8.0) == (64, True)
    worst = F.new_worst()
    for i, kw in enumerate(F.CORNERS):
        host_links(signal(1500, 50 + i), sr, worst, **dict(dict(ratio=F.ratio_of(-3.0)), **kw))
    host_links(signal(1500, 60), sr, worst, ratio=1.3, max_gain_db=0.0)
    check_bars(worst, "live host twin at the corners")


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
def _shift_rows(f):
    return {k: v for k, v in f.items() if k.startswith("share") or k.startswith("shift")}


@pytest.fixture(scope="module")
def reference_behaviour():
    fn = lambda x, sr, st: R.formant_live(x, sr, semitones=st)["y"]                        # noqa: E731
    return F.behaviour(dict(shift=R.realigned(fn, lambda sr: R.geometry(sr)[0])))


def test_behaviour_of_the_definition(reference_behaviour):
    """stage 17's bands on the float64 chain at the live geometry: the formants move, F0 and level stay"""
    f = reference_behaviour
    print("float64, live geometry: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    assert len(f) == 3 * 2 * 3 and f == _shift_rows(f)
    F.check_behaviour(f)


def test_behaviour_of_the_host_twin(reference_behaviour):
    L = _L()
    fn = lambda x, sr, st: L.fx_formant_live_host(x, sr, dict(semitones=st))               # noqa: E731
    f = F.behaviour(dict(shift=R.realigned(fn, L.stream_formant_delay)))
    print("live host twin: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    F.check_behaviour(f)
    for k, v in f.items():                                  # and it is the definition's behaviour, not merely inside the bands
        assert abs(v - reference_behaviour[k]) <= 1e-3, (k, v, reference_behaviour[k])


# ---- off, refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (dict(amount=0.0, ratio=1.5), dict(ratio=1.0), dict(semitones=0.0)))
def test_off_is_the_delayed_input(kw):
    L = _L()
    for sr in (8000, 48000):
        N = R.geometry(sr)[0]
        x = signal(3 * N + 17, 80, sr)
        y, t = L.fx_formant_live_host(x, sr, kw, taps=True)
        assert not y[:N].any() and y[N:].tobytes() == x[:x.shape[0] - N].tobytes()
        assert np.abs(t["g"] - 1.0).max() <= 1e-6 and np.ptp(t["E"]) > 1.0                 # the frames still ran
    short = signal(100, 81)
    assert not L.fx_formant_live_host(short, 8000, kw).any()


def test_refusals_write_nothing_and_the_frame_count():
    L = _L()
    lib = L.lib()
    assert C.sizeof(L.LiveFormantParams) == 32
    x = signal(600, 6)
    y = np.full(600, 7.0, np.float32)

    def refused(what, n=600, sr=8000, rate=0, ch=1, **kw):
        p = L.LiveFormantParams.make(rate, **dict(dict(ratio=1.5), **kw))
        p.channels = ch
        rc = lib.rvcx_fx_formant_live_host(x.ctypes.data, n, sr, C.byref(p), y.ctypes.data, None, None, None, None)
        msg = (lib.rvcx_last_error(None) or b"").decode()
        assert rc == -1 and what in msg, (rc, msg, kw)
        assert (y == 7.0).all()

    for name, bad in (("ratio", (0.49, 2.01)), ("amount", (-0.01, 1.01)), ("max_gain_db", (-1.0, 48.5))):
        for v in bad + (float("nan"), float("inf")):
            refused(name if np.isfinite(v) else "finite", **{name: v})
    refused("iterations", iterations=-1)
    refused("iterations", iterations=17)
    refused("keep_energy", keep_energy=2)
    refused("positive", quefrency_ms=0.0)
    refused("finite", quefrency_ms=float("nan"))
    refused("N / 8", quefrency_ms=0.1)                     # nc = 0
    refused("N / 8", quefrency_ms=8.2)                     # nc = 65 > 512 / 8
    refused("N / 8", sr=16000, quefrency_ms=4.1)           # nc = 65 at the live N = 512 (stage 17 takes it at its N = 1024)
    refused("sample rate", sr=22050)
    refused("sample rate", sr=3100)
    refused("sample_rate must be 0 or", rate=16000)        # a rate that is not the side's
    refused("channels", ch=2)
    refused("samples", n=0)
    assert lib.rvcx_fx_formant_live_host(x.ctypes.data, 600, 8000, None, y.ctypes.data, None, None, None, None) == -1
    assert (y == 7.0).all()
    with pytest.raises(L.RvcxError):
        L.LiveFormantParams.make(0, semitones=12.5)
    with pytest.raises(L.RvcxError):
        L.LiveFormantParams.make(0, semitones=1.0, ratio=1.1)
    with pytest.raises(L.RvcxError, match="unknown value"):
        L.LiveFormantParams.make(0, strength=1.0)
    assert L.LiveFormantParams.make(0, semitones=12.0).ratio == 2.0
    assert L.LiveFormantParams.make(0, semitones=4.0).ratio == np.float32(F.ratio_of(4.0)) == L.formant_ratio(4.0)
    # the default quefrency fits at every admitted rate; the frame count is the restatement's
    for sr in (3200, 8000, 16000, 24000, 24100, 44100, 48000, 96000, 192000):
        N, H, _ = R.geometry(sr)
        assert L.stream_formant_delay(sr) == N
        for n in (0, N // 2 - 1, N // 2, N // 2 + H - 1, N // 2 + H):
            T, N_, nc = L.stream_formant_frames(n, sr)
            assert (T, N_) == (R.frames(n, sr), N) and (nc, True) == R.quefrency_bins(sr, 1.5), (sr, n)
    assert [R.frames(n, 8000) for n in (0, 255, 256, 383, 384)] == [0, 0, 1, 1, 2]
    with pytest.raises(L.RvcxError, match="N / 8"):
        L.stream_formant_frames(1000, 16000, 4.1)
    with pytest.raises(L.RvcxError, match="multiple of 100 Hz"):
        L.stream_formant_delay(22050)
