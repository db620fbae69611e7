"""GPU: include/rvcx.h stages 17 and 18 -- the envelope transfer on the device, checked in links so that every link is judged on
the device's own input (the interface takes no spectra, so D comes from the taps): D against float64 rfft, E and Es against
the restatement on the device's D, g against the restatement on the device's E and Es, s bit for bit from the device's D and
g, y against the float64 synthesis from the device's D, g and s; then the stage whole against the all-float64 restatement and
the host twin, batch and grouping in every bit with and without sources, the skip rule, the errors, the behaviour
conditions and the mirror modules.

Shapes: sr = 8000 (N = 512, H = 128, nb = 257) with n of 1, H - 1, H, 5 H + 3 and 4000; one item of 3 N samples each at 44100,
48000 (N = 2048) and 192000 Hz (N = 8192, all 64 KiB of LDS); nc 1 and N / 8; iterations 0 and 16; ratio 0.5 and 2; amount
0.5; max_gain_db 0; keep_energy 0; an all-zero item; stereo; sources."""
import ctypes as C
import os

import numpy as np
import pytest

import formant_reference as R
from stretch_reference import rms, signal

pytestmark = pytest.mark.gpu

SR = 8000
# Bars: 3x the worst case measured on the MI355X (LABNOTES 25); the conditions are what a wrong link would exceed.
# 1. |D - float64 rfft| over the frame's largest magnitude: measured 2.0e-7, as stages 13 and 15.
BAR_D, CONDITION_D = 6e-7, 1e-5
# 2. E and Es against the restatement on the device's D, absolute (nepers): measured 1.1e-5 at N = 512, 1.3e-5 at N = 2048,
#    3.2e-5 at N = 8192 (the 2 (iterations + 1) float32 transforms of values up to 23, one float32 ulp of which is 1.9e-6; logf).
#    This is the link that carries the stage's error: the host twin, which lifts in double, shows 6.0e-7.
BAR_E, CONDITION_E = 9.6e-5, 1e-3
# 3. g against the restatement on the device's E and Es, relative: measured 1.05e-6 (W and d rounded to float32, expf).
BAR_G, CONDITION_G = 3.2e-6, 1e-3
# 4. s from the device's D and g: equal bit for bit (the sums are double in a defined order).
# 5. y against the float64 synthesis from the device's D, g and s, over the item's peak: measured 6.3e-7 (float32 transform
#    and numerator).
BAR_Y, CONDITION_Y = 1.9e-6, 1e-4
# 6. the stage whole, relative RMS difference: the device measured 6.65e-6 to the all-float64 restatement and to the host twin
#    (it is E's error, a gain error of about 1e-5 per bin); the host twin 9.2e-8 to the restatement.
BAR_E2E, BAR_E2E_TWIN, CONDITION_E2E = 2.0e-5, 2.8e-7, 1e-3
assert BAR_D <= CONDITION_D and BAR_E <= CONDITION_E and BAR_G <= CONDITION_G and BAR_Y <= CONDITION_Y
assert BAR_E2E_TWIN <= BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def device_run(ctx):
    def run(x, sr, source, **kw):
        return ctx.fx_formant_taps(x, sr, _L().FxFormantParams.make(sr, 1, **kw), source=source)
    return run


def check_bars(worst, what):
    print(f"{what}: D {worst['D']:.3e} of the frame's top, E {worst['E']:.3e}, g {worst['g']:.3e} relative, "
          f"y {worst['y']:.3e} of the peak")
    assert worst["D"] <= BAR_D and worst["E"] <= BAR_E and worst["g"] <= BAR_G and worst["y"] <= BAR_Y, worst


def test_links_at_8k(ctx):
    worst = R.new_worst()
    for i, n in enumerate((1, 127, 128, 5 * 128 + 3, 4000)):
        R.check_links(device_run(ctx), signal(n, 20 + i), SR, worst, ratio=R.ratio_of(4.0))
        R.check_links(device_run(ctx), signal(n, 30 + i), SR, worst, source=signal(n, 40 + i))
    check_bars(worst, "device at 8 kHz")


def test_links_at_the_corners(ctx):
    assert R.quefrency_bins(SR, 0.125) == 1 and R.quefrency_bins(SR, 8.0) == 512 // 8
    worst = R.new_worst()
    for i, kw in enumerate(R.CORNERS):
        kw = dict(dict(ratio=R.ratio_of(-3.0)), **kw)
        R.check_links(device_run(ctx), signal(1500, 50 + i), SR, worst, **kw)
    R.check_links(device_run(ctx), signal(1500, 60), SR, worst, source=signal(1500, 61), amount=0.5, keep_energy=0)
    check_bars(worst, "device at the corners")


@pytest.mark.parametrize("sr", (44100, 48000, 192000))
def test_links_at_other_rates(ctx, sr):
    worst = R.new_worst()
    N = R.geometry(sr)[0]
    R.check_links(device_run(ctx), signal(3 * N, 70, sr), sr, worst, ratio=R.ratio_of(-4.0))
    R.check_links(device_run(ctx), signal(3 * N, 71, sr), sr, worst, source=signal(3 * N, 72, sr))
    ms = 1000.0 * (N // 8 + 0.01) / sr                                       # nc = N / 8: every kept quefrency a lane can hold
    assert R.quefrency_bins(sr, ms) == N // 8
    R.check_links(device_run(ctx), signal(3 * N, 73, sr), sr, worst, ratio=2.0, quefrency_ms=ms)
    check_bars(worst, f"device at {sr} Hz")


def test_gain_limit_zeros_and_the_warps_clamp(ctx):
    L = _L()
    x = signal(3000, 5)
    # max_gain_db 0 leaves only s_t, which is then 1: the output is the resynthesis of the input
    # (links 1 and 5 then hold y to the float64 resynthesis of the input's own spectra)
    y, t = ctx.fx_formant_taps(x, SR, L.FxFormantParams.make(SR, 1, ratio=1.5, max_gain_db=0.0))
    assert (t["g"] == 1.0).all() and (t["s"] == 1.0).all()
    worst = R.new_worst()
    assert np.array_equal(R.check_links(device_run(ctx), x, SR, worst, ratio=1.5, max_gain_db=0.0), y)
    check_bars(worst, "device at max_gain_db 0")
    # the gain never leaves the limit
    lim = 6.0 * np.log(10.0) / 20.0
    _, t = ctx.fx_formant_taps(x, SR, L.FxFormantParams.make(SR, 1, ratio=2.0, max_gain_db=6.0))
    assert np.abs(np.log(t["g"].astype(np.float64))).max() <= lim * (1 + 1e-6) and (np.abs(np.log(t["g"])) > 0.99 * lim).any()
    # ratio 0.5: every bin from nb / 2 on takes the last bin's envelope
    _, t = ctx.fx_formant_taps(x, SR, L.FxFormantParams.make(SR, 1, ratio=0.5, max_gain_db=48.0, keep_energy=0))
    nb = t["E"].shape[1]
    lim = 48 * np.log(10) / 20
    want = np.exp(np.clip(t["Es"][:, nb - 1:nb].astype(np.float64) - t["E"][:, nb // 2:], -lim, lim))
    assert np.abs(t["g"][:, nb // 2:] / want - 1.0).max() <= BAR_G and (t["s"] == 1.0).all()
    # all-zero input: all-zero output with g = 1
    z = np.zeros(1000, np.float32)
    for src in (None, z):
        y, t = ctx.fx_formant_taps(z, SR, L.FxFormantParams.make(SR, 1, ratio=1.25), source=src)
        assert not y.any() and not t["D"].any() and (t["g"] == 1.0).all() and (t["s"] == 1.0).all()


def test_stereo_and_sources(ctx):
    L = _L()
    a, b, sa, sb = (signal(2000, 80 + i) for i in range(4))
    st = np.ascontiguousarray(np.stack([a, b], axis=1))
    p1, p2 = L.FxFormantParams.make(SR, 1, semitones=3.0), L.FxFormantParams.make(SR, 2, semitones=3.0)
    one = lambda x, z=None: ctx.fx_formant([x], SR, p1, source=None if z is None else [z])[0]      # noqa: E731
    y2 = ctx.fx_formant([st], SR, p2)[0]
    assert np.array_equal(y2[:, 0], one(a)) and np.array_equal(y2[:, 1], one(b)) and not np.array_equal(y2[:, 0], y2[:, 1])
    y2 = ctx.fx_formant([st], SR, p2, source=[np.stack([sa, sb], axis=1)])[0]
    assert np.array_equal(y2[:, 0], one(a, sa)) and np.array_equal(y2[:, 1], one(b, sb))
    assert not np.array_equal(one(a, sa), one(a)) and not np.array_equal(one(a, sa), one(a, sb))
    assert np.array_equal(one(a), ctx.fx_formant_taps(a, SR, p1)[0])                # the taps change no bit
    with pytest.raises(L.RvcxError, match="same length"):
        ctx.fx_formant([a], SR, p1, source=[sa[:-1]])
    with pytest.raises(L.RvcxError, match="one source entry"):
        ctx.fx_formant([a, b], SR, p1, source=[sa])


def _with_max_batch(value, fn):
    old = os.environ.get("RVCX_MAX_BATCH")
    os.environ["RVCX_MAX_BATCH"] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["RVCX_MAX_BATCH"]
        else:
            os.environ["RVCX_MAX_BATCH"] = old


def test_batch_and_grouping_change_no_bit(ctx):
    """mixed lengths in one call against single calls, RVCX_MAX_BATCH 1 and 3, an item next to a much longer one; sources for
    some items and none for others within one call; at ratio 1 the items without a source are not run"""
    L = _L()
    for ch in (1, 2):
        def sig(n, seed):
            x = signal(n, seed) if ch == 1 else np.stack([signal(n, seed), signal(n, seed + 40)], axis=1)
            return np.ascontiguousarray(x)
        lens = (1, 127, 513, 4000, 40000, 128, 2049)
        xs = [sig(n, 50 + i) for i, n in enumerate(lens)]
        with_src = (True, False, True, True, False, False, True)
        srcs = [sig(n, 70 + i) if w else None for i, (n, w) in enumerate(zip(lens, with_src))]
        for ratio, run in ((R.ratio_of(4.0), 7), (1.0, 4)):
            p = L.FxFormantParams.make(SR, ch, ratio=ratio)
            single = [ctx.fx_formant([x], SR, p, source=[z])[0].tobytes() for x, z in zip(xs, srcs)]
            assert [y.tobytes() for y in ctx.fx_formant(xs, SR, p, source=srcs)] == single
            for cap in (1, 3):
                got = _with_max_batch(cap, lambda: ([y.tobytes() for y in ctx.fx_formant(xs, SR, p, source=srcs)],
                                                    ctx.fx_last_passes()[1]))
                assert got[0] == single and got[1] == -(-run // cap), (ch, ratio, cap, got[1])
            if ratio == 1.0:
                assert all(s == x.tobytes() for s, x, z in zip(single, xs, srcs) if z is None)
                assert all(s != x.tobytes() for s, x, z in zip(single, xs, srcs) if z is not None and x.shape[0] > 1)
            else:                                           # without sources in the same batch: the same bits for those items
                plain = [y.tobytes() for y in ctx.fx_formant(xs, SR, p)]
                assert all(a == b for a, b, z in zip(plain, single, srcs) if z is None)
                # (a one-sample item has a flat spectrum and a flat envelope: no source can shape it)
                assert all(a != b for a, b, z, n in zip(plain, single, srcs, lens) if z is not None and n > 1)


@pytest.fixture(scope="module")
def whole():
    """the end-to-end cases with their all-float64 restatement and their host twin (computed once)"""
    L = _L()
    x8, s8, xv = signal(16000, 90), signal(16000, 91), R.vowel(48000, 110.0, 150.0)
    cases = [(x8, SR, None, dict(ratio=R.ratio_of(4.0))), (x8, SR, s8, dict()), (xv, 48000, None, dict(ratio=R.ratio_of(-4.0)))]
    return [(x, sr, src, kw, R.stage(x, sr, src=src, **kw)["y"],
             L.fx_formant_host(x, sr, L.FxFormantParams.make(sr, 1, **kw), source=src)) for x, sr, src, kw in cases]


def test_stage_whole_against_float64_and_host_twin(ctx, whole):
    L = _L()
    worst = dict(ref=0.0, host=0.0, twin=0.0)
    for x, sr, src, kw, ref, host in whole:
        y = ctx.fx_formant([x], sr, L.FxFormantParams.make(sr, 1, **kw), source=None if src is None else [src])[0]
        assert y.shape == x.shape
        worst["ref"] = max(worst["ref"], rms(y - ref) / rms(ref))
        worst["host"] = max(worst["host"], rms(y - host) / rms(host))
        worst["twin"] = max(worst["twin"], rms(host - ref) / rms(ref))
    print(f"device vs float64 {worst['ref']:.3e}, vs host twin {worst['host']:.3e}, host twin vs float64 {worst['twin']:.3e} "
          f"relative RMS")
    assert worst["ref"] <= BAR_E2E and worst["host"] <= BAR_E2E and worst["twin"] <= BAR_E2E_TWIN, worst


def test_stage_18_is_stage_14_then_the_transfer(ctx):
    L = _L()
    x = signal(6000, 95)
    st = np.ascontiguousarray(np.stack([x, signal(6000, 96)], axis=1))
    items = [st, st[:700].copy()]
    shifted = ctx.fx_pitch_shift(items, SR, 5.0)
    want = ctx.fx_formant(shifted, SR, L.FxFormantParams.make(SR, 2), source=items)
    got = ctx.fx_pitch_shift(items, SR, 5.0, preserve_formants=True)
    t = ctx.fx_formant_timing()
    assert t["pitch_shift"] > 0.0 and t["frames"] > 0.0 and t["total"] > 0.99 * (t["pitch_shift"] + t["frames"])
    assert all(np.array_equal(a, b) and not np.array_equal(a, c) for a, b, c in zip(got, want, shifted))
    # its ratio is not read; amount 0 leaves stage 14; P == sr returns the input and launches nothing
    got = ctx.fx_pitch_shift(items, SR, 5.0, preserve_formants=True, formant_params=L.FxFormantParams.make(SR, 2, ratio=1.7))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    got = ctx.fx_pitch_shift(items, SR, 5.0, preserve_formants=True, formant_params=L.FxFormantParams.make(SR, 2, amount=0.0))
    assert all(np.array_equal(a, b) for a, b in zip(got, shifted))
    got = ctx.fx_pitch_shift(items, SR, 0.0, preserve_formants=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, items))
    assert ctx.fx_formant_timing()["total"] == 0.0 and ctx.fx_last_passes()[1] == 0
    assert all(np.array_equal(a, b) for a, b in zip(ctx.fx_pitch_shift(items, SR, 5.0), shifted))      # the plain call is what it was


@pytest.mark.parametrize("case", R.VOWELS, ids=lambda c: str(c[0]))
def test_behaviour_on_the_device(ctx, case):
    """the conditions of tests/test_formant_host.py, on the device"""
    L = _L()
    f = R.behaviour(dict(shift=lambda x, sr, st: ctx.fx_formant([x], sr, L.FxFormantParams.make(sr, 1, semitones=st))[0],
                         pitch=lambda x, sr, st: ctx.fx_pitch_shift([x], sr, st)[0],
                         preserved=lambda x, sr, st: ctx.fx_pitch_shift([x], sr, st, preserve_formants=True)[0]), cases=(case,))
    print(f"device at {case[0]} Hz: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    assert len(f) == 2 * 3 + 2 * 4
    R.check_behaviour(f)


def test_skip(ctx):
    L = _L()
    x = signal(4000, 5)
    x[7] = np.float32(-0.0)
    ctx.fx_formant([x], SR, L.FxFormantParams.make(SR, 1, ratio=1.5))
    assert ctx.fx_formant_timing()["total"] > 0.0 and ctx.fx_last_passes()[1] == 1
    st = np.ascontiguousarray(np.stack([x, signal(4000, 6)], axis=1))
    for kw, src in ((dict(ratio=1.0), None), (dict(ratio=1.5, amount=0.0), None), (dict(amount=0.0), [st[::-1].copy(), None])):
        y = ctx.fx_formant([st, st[:100]], SR, L.FxFormantParams.make(SR, 2, **kw), source=src)     # bit for bit, nothing launched
        assert np.array_equal(y[0].view(np.uint32), st.view(np.uint32)) and np.array_equal(y[1], st[:100])
        assert ctx.fx_formant_timing()["total"] == 0.0 and ctx.fx_last_passes()[1] == 0
    y = ctx.fx_formant([st], SR, L.FxFormantParams.make(SR, 2), source=[st[::-1].copy()])             # ratio 1 with a source runs
    assert not np.array_equal(y[0], st) and ctx.fx_last_passes()[1] == 1
    with pytest.raises(L.RvcxError, match="skipped"):
        ctx.fx_formant_taps(x, SR, L.FxFormantParams.make(SR, 1))


def test_errors_write_nothing(ctx):
    L = _L()
    lib = L.lib()
    x = signal(600, 6)
    y = np.full(600, 7.0, np.float32)
    xp, yp = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(y.ctypes.data)

    def refused(what, n=600, sr=SR, ch=1, B=1, **kw):
        p = L.FxFormantParams.make(sr, ch, **dict(dict(ratio=1.5), **kw))
        rc = lib.rvcx_fx_formant(ctx._h, B, xp, (C.c_int64 * 1)(n), None, C.byref(p), yp)
        msg = (lib.rvcx_last_error(ctx._h) or b"").decode()
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
    refused("sample rate", sr=7000)
    refused("channels", ch=3)
    refused("frames", n=0)
    refused("B < 1", B=0)

    def refused18(what, s=5.0, out=yp, **kw):
        p = L.FxFormantParams.make(SR, 1, **kw)
        rc = lib.rvcx_fx_pitch_shift_formant(ctx._h, 1, xp, (C.c_int64 * 1)(600), 1, SR, s, C.byref(p), out)
        msg = (lib.rvcx_last_error(ctx._h) or b"").decode()
        assert rc == -1 and what in msg, (rc, msg, kw)
        assert (y == 7.0).all()

    refused18("semitones", s=12.5)
    refused18("finite", s=float("nan"))
    refused18("amount", amount=2.0)
    before = x.copy()
    refused18("must not lie over", out=xp)
    assert np.array_equal(x, before)
    # a partial overlap, and an output over ANOTHER item's input, are refused too
    buf = np.concatenate([x, x, x])
    snap = buf.copy()
    for off_x, off_y in ((0, 300), (300, 0), (600, 1)):
        p = L.FxFormantParams.make(SR, 1)
        rc = lib.rvcx_fx_pitch_shift_formant(ctx._h, 1, (C.c_void_p * 1)(buf[off_x:].ctypes.data), (C.c_int64 * 1)(600), 1, SR, 5.0,
                                             C.byref(p), (C.c_void_p * 1)(buf[off_y:].ctypes.data))
        assert rc == -1 and "must not lie over" in (lib.rvcx_last_error(ctx._h) or b"").decode() and np.array_equal(buf, snap)
    p = L.FxFormantParams.make(SR, 1)
    two_x = (C.c_void_p * 2)(buf[0:].ctypes.data, buf[600:].ctypes.data)
    two_y = (C.c_void_p * 2)(y.ctypes.data, buf[0:].ctypes.data)              # output 1 over input 0
    rc = lib.rvcx_fx_pitch_shift_formant(ctx._h, 2, two_x, (C.c_int64 * 2)(600, 600), 1, SR, 5.0, C.byref(p), two_y)
    assert rc == -1 and np.array_equal(buf, snap) and (y == 7.0).all()
    rc = lib.rvcx_fx_pitch_shift_formant(ctx._h, 1, (C.c_void_p * 1)(buf[0:].ctypes.data), (C.c_int64 * 1)(600), 1, SR, 5.0,
                                         C.byref(p), (C.c_void_p * 1)(buf[600:].ctypes.data))    # adjacent is no overlap
    assert rc == 0 and np.array_equal(buf[:600], snap[:600]) and not np.array_equal(buf[600:1200], snap[600:1200])
    old = os.environ.get("RVCX_ARENA_GB")               # an item that does not fit the arena budget on its own
    os.environ["RVCX_ARENA_GB"] = "0"
    try:
        refused("600 frames needs")
        refused18("600 frames needs")
    finally:
        if old is None:
            del os.environ["RVCX_ARENA_GB"]
        else:
            os.environ["RVCX_ARENA_GB"] = old
    assert ctx.fx_formant([x], SR, L.FxFormantParams.make(SR, 1, ratio=1.5))[0].shape == (600,)      # the context works on


# ---- the mirror modules ----------------------------------------------------------------------------------------------------------
def _pcm(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _f32(a):
    return (a.astype(np.float64) / 32768.0).astype(np.float32)         # what read_audio hands over


def test_shift_formants_through_files(ctx, tmp_path):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    L = _L()
    sr = 16000
    x = R.vowel(sr, 220.0, 250.0, seconds=0.5)
    mono, stereo = _pcm(x), np.stack([_pcm(x), _pcm(x[::-1])], axis=1)
    wavfile.write(str(tmp_path / "m.wav"), sr, mono)
    wavfile.write(str(tmp_path / "s.wav"), sr, stereo)
    M.shift_formants(str(tmp_path / "m.wav"), str(tmp_path / "m_out.wav"), 3.0)
    sr2, got = wavfile.read(str(tmp_path / "m_out.wav"))
    want = ctx.fx_formant([_f32(mono)], sr, L.FxFormantParams.make(sr, 1, semitones=3.0))[0]
    assert sr2 == sr and got.dtype == np.int16 and got.shape == mono.shape
    assert np.array_equal(got, _pcm(want)) and not np.array_equal(got, mono)
    M.shift_formants(str(tmp_path / "m.wav"), str(tmp_path / "m_q.wav"), -2.0, quefrency_ms=1.0, amount=0.5)
    want = ctx.fx_formant([_f32(mono)], sr, L.FxFormantParams.make(sr, 1, semitones=-2.0, quefrency_ms=1.0, amount=0.5))[0]
    assert np.array_equal(wavfile.read(str(tmp_path / "m_q.wav"))[1], _pcm(want))
    M.shift_formants(str(tmp_path / "s.wav"), str(tmp_path / "s0.wav"), 0.0)                # 0 copies the samples
    assert np.array_equal(wavfile.read(str(tmp_path / "s0.wav"))[1], stereo)
    outs = M.shift_formants_many([(str(tmp_path / "m.wav"), str(tmp_path / "a.wav")), (str(tmp_path / "s.wav"), str(tmp_path / "b.wav")),
                                  (str(tmp_path / "m.wav"), str(tmp_path / "c.flac"))], 3.0)
    assert outs == [str(tmp_path / n) for n in ("a.wav", "b.wav", "c.flac")]
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "m_out.wav").read_bytes()
    want = ctx.fx_formant([_f32(stereo)], sr, L.FxFormantParams.make(sr, 2, semitones=3.0))[0]
    got = wavfile.read(str(tmp_path / "b.wav"))[1]
    assert got.shape == stereo.shape and np.array_equal(got, _pcm(want))
    # shift_pitch(preserve_formants=True): the library call's samples, not those of the plain shift
    M.shift_pitch(str(tmp_path / "s.wav"), str(tmp_path / "p.wav"), 4.0, preserve_formants=True)
    M.shift_pitch(str(tmp_path / "s.wav"), str(tmp_path / "p_plain.wav"), 4.0)
    sr2, got = wavfile.read(str(tmp_path / "p.wav"))
    want = ctx.fx_pitch_shift([_f32(stereo)], sr, 4.0, preserve_formants=True)[0]
    assert sr2 == sr and got.shape == stereo.shape and np.array_equal(got, _pcm(want))
    assert np.array_equal(wavfile.read(str(tmp_path / "p_plain.wav"))[1], _pcm(ctx.fx_pitch_shift([_f32(stereo)], sr, 4.0)[0]))
    assert not np.array_equal(got, wavfile.read(str(tmp_path / "p_plain.wav"))[1])
    M.shift_pitch(str(tmp_path / "s.wav"), str(tmp_path / "p0.wav"), 0.0, preserve_formants=True)
    assert np.array_equal(wavfile.read(str(tmp_path / "p0.wav"))[1], stereo)


def test_process_audio_shifts_the_vocals_formants(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    L = _L()
    monkeypatch.setattr(M, "OUTPUT_DIR", str(tmp_path / "output"))
    sr = 16000
    x = R.vowel(sr, 220.0, 250.0, seconds=0.5)
    wavfile.write(str(tmp_path / "v.wav"), sr, _pcm(x))
    wavfile.write(str(tmp_path / "i.wav"), sr, np.zeros((sr // 2, 2), np.int16))
    fx = list(L.FX_UI_DEFAULTS.values())
    for use_effects in (False, True):
        args = (str(tmp_path / "v.wav"), str(tmp_path / "i.wav"), *fx, "wav", 0, 0, use_effects)
        plain = open(M.process_audio(*args), "rb").read()
        assert open(M.process_audio(*args, vocal_formant=0.0), "rb").read() == plain          # byte for byte at 0.0
        moved = open(M.process_audio(*args, vocal_formant=3.0), "rb").read()
        assert moved != plain and len(moved) == len(plain)
        many = M.process_audio_many([args + (str(tmp_path / "m1.wav"),), args + (str(tmp_path / "m2.wav"),)], vocal_formant=3.0)
        assert [open(p, "rb").read() for p in many] == [moved, moved]
        many = M.process_audio_many([args + (str(tmp_path / "m3.wav"),)], vocal_formant=0.0)
        assert open(many[0], "rb").read() == plain
    # without the board the cover is the shifted vocal (the instrumental is silent): the Context call on the same samples
    args = (str(tmp_path / "v.wav"), str(tmp_path / "i.wav"), *fx, "wav", 0, 0, False)
    _, cover = wavfile.read(M.process_audio(*args, vocal_formant=3.0))
    v = _f32(_pcm(x))
    from polgen_rvc_amd.infer import _state
    want = _state.context().fx_formant([np.stack([v, v], axis=1)], sr, L.FxFormantParams.make(sr, 2, semitones=3.0))[0]
    assert np.array_equal(cover, _pcm(want))


class _StubVC:
    """VC.pipeline's place in rvc_infer: returns a fixed int16 signal and keeps what it was given"""

    def __init__(self, out):
        self.out, self.seen = out, []

    def pipeline(self, model, net_g, sid, audio, *a, **kw):
        self.seen.append(np.array(audio))
        return self.out

    def pipeline_stream(self, model, net_g, sid, clips, *a, **kw):
        for c in clips:
            self.seen.append(np.array(c))
            yield self.out


class _StubHubert:
    def __init__(self, ctx):
        self.ctx = ctx


def test_rvc_infer_formant_shift(ctx, tmp_path):
    from polgen_rvc_amd.infer import infer as I
    from polgen_rvc_amd.infer.audio import write_output
    L = _L()
    tgt_sr = 48000
    x = R.vowel(16000, 220.0, 250.0, seconds=0.5)
    out = _pcm(R.vowel(tgt_sr, 220.0, 250.0, seconds=0.5))
    write_output(str(tmp_path / "in.wav"), _pcm(x), 16000)
    hub = _StubHubert(ctx)

    def run(fn, name, **kw):
        vc = _StubVC(out)
        fn(None, 0, str(tmp_path / "in.wav"), str(tmp_path / name), 0.0, "rmvpe+", {"f0": 1}, "v2", None, 3, tgt_sr, 1.0, 0.33, 128,
           vc, hub, **kw)
        return (tmp_path / name).read_bytes(), vc.seen[0]

    plain, fed = run(I.rvc_infer, "plain.wav")
    same, fed_0 = run(I.rvc_infer_clean, "zero.wav", clean_audio=None, formant_shift=0.0)
    assert same == plain and np.array_equal(fed, fed_0)                                    # 0.0: nothing changes
    want = ctx.fx_formant([fed.astype(np.float32)], 16000, L.FxFormantParams.make(16000, 1, semitones=3.0))[0].astype(np.float64)
    got, fed_in = run(I.rvc_infer_clean, "moved.wav", clean_audio=None, formant_shift=3.0)
    assert got == plain and np.array_equal(fed_in, want) and not np.array_equal(fed_in, fed)
    want_q = ctx.fx_formant([fed.astype(np.float32)], 16000,
                            L.FxFormantParams.make(16000, 1, semitones=3.0, quefrency_ms=1.0))[0].astype(np.float64)
    _, fed_q = run(I.rvc_infer_clean, "moved_q.wav", clean_audio=None, formant_shift=3.0, formant_quefrency_ms=1.0)
    assert np.array_equal(fed_q, want_q) and not np.array_equal(fed_q, want)
    # behind the cleaning
    cleaned = ctx.fx_denoise([fed.astype(np.float32)], 16000, L.FxDenoiseParams.make(16000, 1, mode=1, strength=0.6))[0]
    want_c = ctx.fx_formant([cleaned], 16000, L.FxFormantParams.make(16000, 1, semitones=3.0))[0].astype(np.float64)
    _, fed_c = run(I.rvc_infer_clean, "both.wav", clean_audio="input", clean_strength=0.6, formant_shift=3.0)
    assert np.array_equal(fed_c, want_c)
    vc = _StubVC(out)
    I.rvc_infer_many(None, 0, [str(tmp_path / "in.wav")] * 2, [str(tmp_path / "m0.wav"), str(tmp_path / "m1.wav")], 0.0, "rmvpe+",
                     {"f0": 1}, "v2", None, 3, tgt_sr, 1.0, 0.33, 128, vc, hub, formant_shift=3.0)
    assert (tmp_path / "m0.wav").read_bytes() == plain == (tmp_path / "m1.wav").read_bytes()
    assert np.array_equal(vc.seen[0], want) and np.array_equal(vc.seen[1], want)
    vc = _StubVC(out)
    I.rvc_infer_many(None, 0, [str(tmp_path / "in.wav")], [str(tmp_path / "m2.wav")], 0.0, "rmvpe+", {"f0": 1}, "v2", None, 3,
                     tgt_sr, 1.0, 0.33, 128, vc, hub)
    assert (tmp_path / "m2.wav").read_bytes() == plain and np.array_equal(vc.seen[0], fed)
    for bad in (dict(formant_shift=13.0), dict(formant_shift=2.0, formant_quefrency_ms=0.0)):
        with pytest.raises(ValueError):
            run(I.rvc_infer_clean, "bad.wav", clean_audio=None, **bad)
    assert not (tmp_path / "bad.wav").exists()


def test_rvc_infer_formant_shift_changes_the_conversion(ctx, tmp_path):
    """through the real VC.pipeline / pipeline_stream on the reduced models: the converted file differs with formant_shift and
    is byte for byte the default-keyword file at 0.0; what the models are fed is the library call's output"""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.infer import infer as I
    from polgen_rvc_amd.infer.audio import write_output
    L = _L()
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    I._CTX[0] = ctx
    hub = I.load_hubert("cuda:0", False, None, state=S.hubert_state(hcfg, 11), cfg=hcfg)
    I.load_rmvpe("cuda:0", state=S.rmvpe_state(rcfg, 11), cfg=rcfg)
    cpt = S.synth_checkpoint(scfg, 11)
    cpt["weight"] = S.synth_state(scfg, 11, input_dim=hcfg["embed_dim"])
    cfg = I.Config()
    cfg.x_pad, cfg.x_query, cfg.x_center, cfg.x_max = 1, 1, 2, 3
    cpt, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, cfg, None, cpt=cpt)
    vc.seed = 21
    ins = []
    for i, (f0, secs) in enumerate(((220.0, 1.3), (150.0, 0.9))):
        ins.append(str(tmp_path / f"in{i}.wav"))
        write_output(ins[i], _pcm(R.vowel(16000, f0, 250.0, seconds=secs)), 16000)

    def one(name, path, **kw):
        I.rvc_infer_clean(None, 0, path, str(tmp_path / name), 0.0, "rmvpe+", cpt, version, net_g, 3, tgt_sr, 1.0, 0.33, 128, vc, hub,
                          clean_audio=None, **kw)
        return (tmp_path / name).read_bytes()

    def many(tag, **kw):
        outs = [str(tmp_path / f"{tag}{i}.wav") for i in range(len(ins))]
        I.rvc_infer_many(None, 0, ins, outs, 0.0, "rmvpe+", cpt, version, net_g, 3, tgt_sr, 1.0, 0.33, 128, vc, hub, **kw)
        return [open(o, "rb").read() for o in outs]

    plain = []
    for i, path in enumerate(ins):
        I.rvc_infer(None, 0, path, str(tmp_path / f"plain{i}.wav"), 0.0, "rmvpe+", cpt, version, net_g, 3, tgt_sr, 1.0, 0.33, 128, vc, hub)
        plain.append((tmp_path / f"plain{i}.wav").read_bytes())
    assert all(len(b) > 1000 for b in plain)
    default = [one(f"default{i}.wav", p) for i, p in enumerate(ins)]            # the default keywords
    zero = [one(f"zero{i}.wav", p, formant_shift=0.0) for i, p in enumerate(ins)]
    moved = [one(f"moved{i}.wav", p, formant_shift=3.0) for i, p in enumerate(ins)]
    down = [one(f"down{i}.wav", p, formant_shift=-3.0) for i, p in enumerate(ins)]
    assert default == plain and zero == plain
    assert all(m != b and len(m) == len(b) and d != b and d != m for m, d, b in zip(moved, down, plain))
    assert many("many_default") == plain and many("many_zero", formant_shift=0.0) == plain
    assert many("many_moved", formant_shift=3.0) == moved
    # the moved file is the conversion of the library call's output: VC.pipeline on that array writes the same bytes
    for i, path in enumerate(ins):
        audio = I.load_audio(path, 16000)
        fed = ctx.fx_formant([audio.astype(np.float32)], 16000, L.FxFormantParams.make(16000, 1, semitones=3.0))[0].astype(np.float64)
        opt = vc.pipeline(hub, net_g, 0, fed, path, 0.0, "rmvpe+", None, 0, 1, 3, tgt_sr, 0, 1.0, "v2", 0.33, 128, None)
        write_output(str(tmp_path / f"direct{i}.wav"), opt, tgt_sr)
        assert (tmp_path / f"direct{i}.wav").read_bytes() == moved[i]
