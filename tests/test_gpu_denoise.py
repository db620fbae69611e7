"""GPU: include/rvcx.h stage 15 -- noise reduction on the device, checked in links so that every stage is judged on the
device's own input: D against float64 rfft, S against the restatement on the device's A2, mu and sd (mode 0) or b (mode 1)
against the restatement on the device's S, m against the restatement on the device's S and statistics or floor, y against
the float64 synthesis from the device's D and m; then the stage whole against the all-float64 restatement and the host
twin, batch and grouping in every bit, noise clips shared, per item and absent, the skip rule, the errors, the behaviour
conditions and the mirror modules.

Shapes: sr = 8000 (N = 512, H = 128, nb = 257); lengths 1, 127, 128, 511, 512, 513, 4000 and those that give T = L - 1, L, L + 1
and 3 L + 1 frames for the smoothing tile (L = 16 frames) and for the statistics chunk (L = 64 frames); mono and stereo; an
all-zero item and one with 0.2 s of exact zeros in the middle; one 1 s item each at 44100, 48000 and 192000 Hz; both modes;
the default half-widths and (0, 0) and (64, 16); knee_db 1 and 0.25."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_reference as R
from stretch_reference import rms, signal

pytestmark = pytest.mark.gpu

SR = 8000
# Bars: 3x the worst case measured on the GPU at the first run (LABNOTES 23); each condition is the issue's.
# 1. |D - float64 rfft| over the frame's largest magnitude: measured 2.2e-7 (1.6e-7 at N = 8192), as stage 13's.
BAR_D, CONDITION_D = 7e-7, 1e-5
# 2. S against the restatement on the device's A2, relative per element: measured 4.8e-7 at half-widths (64, 16), 0 at
#    (0, 0) (a wrong tap or edge weight: 1e-2).
BAR_S, CONDITION_S = 1.5e-6, 1e-5
# 3. mu and sd against the restatement on the device's S, in dB: measured 4.5e-6 (float32 log10f).
BAR_STAT, CONDITION_STAT = 1.4e-5, 1e-3
# 4. b against the restatement on the device's S, relative: measured 5.7e-8 (sqrtf is exact, the recurrences are double).
BAR_B, CONDITION_B = 1.8e-7, 1e-6
# 5. m against the restatement on the device's S and the device's mu, sd or b, absolute: measured 2.7e-6 at knee_db 0.25,
#    1.4e-6 at 1 (expf, log10f).
BAR_M, CONDITION_M = 9e-6, 1e-3
# 6. y against the float64 synthesis from the device's D and m, over the item's peak: measured 2.3e-7 (float32 transform
#    and numerator).
BAR_Y, CONDITION_Y = 7e-7, 1e-4
# 7. the stage whole: relative RMS difference to the all-float64 restatement and to the host twin: measured 1.3e-7 to both
#    (no decision in this stage can fall the other way: the gate is continuous in the spectrum).
BAR_E2E, CONDITION_E2E = 4e-7, 1e-3
assert BAR_D <= CONDITION_D and BAR_S <= CONDITION_S and BAR_STAT <= CONDITION_STAT and BAR_B <= CONDITION_B
assert BAR_M <= CONDITION_M and BAR_Y <= CONDITION_Y and BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def n_for_frames(T, H=128):
    return max((T - 1) * H, 1)


def lengths():
    tile_t, _, chunk = _L().fx_denoise_tiles()
    return [1, 127, 128, 511, 512, 513, 4000] + [n_for_frames(T) for L in (tile_t, chunk) for T in (L - 1, L, L + 1, 3 * L + 1)]


def new_worst():
    return dict(D=0.0, S=0.0, stat=0.0, b=0.0, m=0.0, y=0.0)


def rel(a, ref):
    """largest relative difference per element; where the reference is zero the value must be zero too"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert not a[ref == 0].any()
    ok = ref != 0
    return float((np.abs(a[ok] - ref[ok]) / np.abs(ref[ok])).max()) if ok.any() else 0.0


def check_links(ctx, x, sr, worst, noise=None, **kw):
    """links 1 - 6 on one channel; returns the device's y"""
    L = _L()
    v = R.values(**kw)
    n = x.shape[0]
    N, H, nb = R.geometry(sr)
    T = R.frames(n, sr)
    nf, nt = R.half_widths(sr, v["freq_smooth_hz"], v["time_smooth_ms"])
    p = L.FxDenoiseParams.make(sr, 1, **kw)
    y, t = ctx.fx_denoise_taps(x, sr, p, noise=noise)
    assert y.shape == (n,) and t["D"].shape == (T, nb, 2) and t["S"].shape == (T, nb) and t["m"].shape == (T, nb)
    D32 = R.pairs_to_complex(t["D"])
    ref_D = R.analysis(x, sr)
    top = np.abs(ref_D).max(axis=1)
    err = np.abs(ref_D - D32.astype(np.complex128)).max(axis=1)
    worst["D"] = max(worst["D"], float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0)
    assert not err[top == 0].any()
    worst["S"] = max(worst["S"], rel(t["S"], R.smooth(R.a2_of(D32), nf, nt)))
    if v["mode"] == 0:
        # the profile: the item's own S, or the S the device forms for the clip (a result depends on the signal alone)
        Sp = t["S"] if noise is None else ctx.fx_denoise_taps(noise, sr, p)[1]["S"]
        mu, sd = R.profile_stats(Sp)
        worst["stat"] = max(worst["stat"], float(np.abs(t["mu"] - mu).max()), float(np.abs(t["sd"] - sd).max()))
        m = R.mask_profile(t["S"], t["mu"], t["sd"], v["n_std"], v["knee_db"])
    else:
        worst["b"] = max(worst["b"], rel(t["b"], R.floor(t["S"], R.floor_constant(sr, v["time_constant_s"]))[1]))
        m = R.mask_adaptive(t["S"], t["b"], v["thresh_mult"], v["slope"])
    worst["m"] = max(worst["m"], float(np.abs(t["m"] - m).max()))
    ref = R.synthesis(D32, t["m"], v["strength"], n, sr)
    worst["y"] = max(worst["y"], float(np.abs(y - ref).max()) / max(float(np.abs(x).max()), 1e-30))
    return y


def check_bars(worst, what):
    print(f"{what}: D {worst['D']:.3e} of the frame's top, S {worst['S']:.3e} relative, mu/sd {worst['stat']:.3e} dB, "
          f"b {worst['b']:.3e} relative, m {worst['m']:.3e}, y {worst['y']:.3e} of the peak")
    assert worst["D"] <= BAR_D and worst["S"] <= BAR_S and worst["stat"] <= BAR_STAT and worst["b"] <= BAR_B, worst
    assert worst["m"] <= BAR_M and worst["y"] <= BAR_Y, worst


@pytest.mark.parametrize("mode", (0, 1))
def test_links_at_8k(ctx, mode):
    worst = new_worst()
    for i, n in enumerate(lengths()):
        clip = signal(n_for_frames(7 + 20 * (i % 4)), 60 + i) * np.float32(0.1) if mode == 0 and i % 2 else None
        check_links(ctx, signal(n, 20 + i), SR, worst, noise=clip, mode=mode)
    check_bars(worst, f"mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("hz,ms", ((0.0, 0.0), (64 * 2 * SR / 512.0, 16 * 2000 * 128.0 / SR)))
def test_links_at_other_widths_and_knee(ctx, mode, hz, ms):
    """half-widths (0, 0) and (64, 16), the second with items shorter than the time triangle; knee_db 0.25"""
    assert R.half_widths(SR, hz, ms) in ((0, 0), (64, 16))
    tile_t = _L().fx_denoise_tiles()[0]
    worst = new_worst()
    for i, n in enumerate((1, 513, 4000, n_for_frames(tile_t), n_for_frames(3 * tile_t + 1))):
        check_links(ctx, signal(n, 80 + i), SR, worst, mode=mode, freq_smooth_hz=hz, time_smooth_ms=ms, knee_db=0.25)
    check_bars(worst, f"mode {mode}, widths {R.half_widths(SR, hz, ms)}")


@pytest.mark.parametrize("sr", (44100, 48000, 192000))
def test_links_at_other_rates(ctx, sr):
    worst = new_worst()
    check_links(ctx, signal(sr, 40, sr), sr, worst, mode=1)
    check_links(ctx, signal(sr, 41, sr), sr, worst, noise=signal(sr // 4, 42, sr), mode=0)
    check_bars(worst, f"sr {sr}")


def test_zeros_and_stereo(ctx):
    """an all-zero item returns zeros; 0.2 s of exact zeros in the middle pass the links; a stereo item is its two channels"""
    L = _L()
    z = np.zeros(3000, np.float32)
    for mode in (0, 1):
        y, t = ctx.fx_denoise_taps(z, SR, L.FxDenoiseParams.make(SR, 1, mode=mode))
        assert not y.any() and not t["D"].any() and not t["S"].any() and np.isfinite(t["m"]).all()
    worst = new_worst()
    x = signal(8000, 31)
    x[3000:4600] = 0.0
    for mode in (0, 1):
        a = check_links(ctx, x, SR, worst, mode=mode)
        b = check_links(ctx, signal(8000, 32), SR, worst, mode=mode)
        st = np.ascontiguousarray(np.stack([x, signal(8000, 32)], axis=1))
        y2 = ctx.fx_denoise([st], SR, L.FxDenoiseParams.make(SR, 2, mode=mode))[0]
        assert np.array_equal(y2[:, 0], a) and np.array_equal(y2[:, 1], b)
    check_bars(worst, "zeros in the middle")
    # a stereo clip: channel c of the clip serves channel c of the item
    za, zb = signal(2000, 33) * np.float32(0.1), signal(2000, 34) * np.float32(0.1)
    p = L.FxDenoiseParams.make(SR, 2, mode=0)
    y2 = ctx.fx_denoise([st], SR, p, noise=np.stack([za, zb], axis=1))[0]
    assert np.array_equal(y2[:, 0], ctx.fx_denoise([x], SR, p, noise=za)[0])
    assert np.array_equal(y2[:, 1], ctx.fx_denoise([signal(8000, 32)], SR, p, noise=zb)[0])


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
    """mixed lengths in one call against single calls, RVCX_MAX_BATCH 1 and 3, an item next to a much longer one; a noise
    clip shared, per item and absent within one call"""
    L = _L()
    for ch in (1, 2):
        def sig(n, seed, scale=1.0):
            x = signal(n, seed) if ch == 1 else np.stack([signal(n, seed), signal(n, seed + 40)], axis=1)
            return np.ascontiguousarray(x * np.float32(scale))
        xs = [sig(n, 50 + i) for i, n in enumerate((1, 127, 513, 4000, 40000, 128, 2049))]
        shared, own = sig(1500, 70, 0.1), sig(900, 71, 0.1)
        for mode in (0, 1):
            p = L.FxDenoiseParams.make(SR, ch, mode=mode)
            clips = [shared, None, own, shared, None, shared, own][:len(xs)] if mode == 0 else [None] * len(xs)
            single = [ctx.fx_denoise([x], SR, p, noise=[z])[0].tobytes() for x, z in zip(xs, clips)]
            assert [y.tobytes() for y in ctx.fx_denoise(xs, SR, p, noise=clips)] == single
            for cap, groups in ((1, 7), (3, 3)):
                got = _with_max_batch(cap, lambda: ([y.tobytes() for y in ctx.fx_denoise(xs, SR, p, noise=clips)],
                                                    ctx.fx_last_passes()[1]))
                assert got[0] == single and got[1] == groups, (ch, mode, cap, got[1])
            if mode == 0:         # one array for all items is the same clip for each of them
                all_shared = [ctx.fx_denoise([x], SR, p, noise=shared)[0].tobytes() for x in xs]
                assert [y.tobytes() for y in ctx.fx_denoise(xs, SR, p, noise=shared)] == all_shared
                assert all_shared[0] == single[0] and all_shared[1] != single[1]


@pytest.fixture(scope="module")
def whole():
    """three signals and, per mode, the all-float64 restatement and the host twin (computed once)"""
    L = _L()
    xs = [signal(n, 90 + i) for i, n in enumerate((4000, 12289, 16000))]
    clip = signal(3000, 99) * np.float32(0.1)
    ref = {(i, mode): (R.denoise(x, SR, noise=clip if mode == 0 else None, mode=mode)["y"],
                       L.fx_denoise_host(x, SR, L.FxDenoiseParams.make(SR, 1, mode=mode), noise=clip if mode == 0 else None))
           for i, x in enumerate(xs) for mode in (0, 1)}
    return xs, clip, ref


def test_stage_whole_against_float64_and_host_twin(ctx, whole):
    L = _L()
    xs, clip, ref = whole
    worst = dict(ref=0.0, host=0.0)
    for mode in (0, 1):
        ys = ctx.fx_denoise(xs, SR, L.FxDenoiseParams.make(SR, 1, mode=mode), noise=clip if mode == 0 else None)
        for i, y in enumerate(ys):
            yr, yh = ref[(i, mode)]
            assert y.shape == xs[i].shape
            worst["ref"] = max(worst["ref"], rms(y - yr) / rms(yr))
            worst["host"] = max(worst["host"], rms(y - yh) / rms(yh))
    print(f"device vs float64 {worst['ref']:.3e}, vs host twin {worst['host']:.3e} relative RMS")
    assert worst["ref"] <= BAR_E2E and worst["host"] <= BAR_E2E, worst


@pytest.mark.parametrize("sr", (8000, 48000))
def test_behaviour_on_the_device(ctx, sr):
    """the conditions of tests/test_denoise_host.py, on the device"""
    L = _L()
    f = R.behaviour(lambda x, sr, noise=None, **kw: ctx.fx_denoise([x.astype(np.float32)], sr, L.FxDenoiseParams.make(sr, 1, **kw),
                                                                   noise=None if noise is None else noise.astype(np.float32))[0], sr)
    print(f"device at {sr} Hz: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    R.check_behaviour(f)


def test_skip(ctx):
    L = _L()
    x = signal(4000, 5)
    ctx.fx_denoise([x], SR)
    assert ctx.fx_denoise_timing()["total"] > 0.0 and ctx.fx_last_passes()[1] == 1
    st = np.ascontiguousarray(np.stack([x, signal(4000, 6)], axis=1))
    for mode in (0, 1):                                               # strength 0: bit for bit, nothing launched
        y = ctx.fx_denoise([st, st[:100]], SR, L.FxDenoiseParams.make(SR, 2, mode=mode, strength=0.0))
        assert np.array_equal(y[0].view(np.uint32), st.view(np.uint32)) and np.array_equal(y[1], st[:100])
        assert ctx.fx_denoise_timing()["total"] == 0.0 and ctx.fx_last_passes()[1] == 0


def test_errors_write_nothing(ctx):
    L = _L()
    lib = L.lib()
    x, z = signal(600, 6), signal(300, 7)
    y = np.full(600, 7.0, np.float32)
    xp, yp = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(y.ctypes.data)
    zp = (C.c_void_p * 1)(z.ctypes.data)

    def refused(what, n=600, noise=None, n_noise=0, sr=SR, ch=1, B=1, **kw):
        p = L.FxDenoiseParams.make(sr, ch, **kw)
        rc = lib.rvcx_fx_denoise(ctx._h, B, xp, (C.c_int64 * 1)(n), noise, (C.c_int64 * 1)(n_noise), C.byref(p), yp)
        msg = (lib.rvcx_last_error(ctx._h) or b"").decode()
        assert rc == -1 and what in msg, (rc, msg, kw)
        assert (y == 7.0).all()

    for name, bad in (("strength", (-0.01, 1.01)), ("n_std", (-1.0, 10.5)), ("knee_db", (0.05, 21.0)),
                      ("thresh_mult", (-0.1, 20.5)), ("slope", (0.05, 101.0)), ("time_constant_s", (0.01, 31.0))):
        for v in bad + (float("nan"),):
            refused(name if np.isfinite(v) else "finite", **{name: v})
    refused("negative", freq_smooth_hz=-1.0)
    refused("negative", time_smooth_ms=-1.0)
    refused("finite", time_smooth_ms=float("inf"))
    refused("64 bins", freq_smooth_hz=65 * 2 * SR / 512.0)
    refused("16 frames", time_smooth_ms=17 * 2000 * 128 / SR + 1.0)
    refused("mode", mode=2)
    refused("sample rate", sr=7000)
    refused("channels", ch=3)
    refused("frames", n=0)
    refused("B < 1", B=0)
    refused("noise clip", mode=1, noise=zp, n_noise=300)
    refused("noise clip", mode=0, noise=zp, n_noise=0)
    with pytest.raises(L.RvcxError, match="channel"):
        ctx.fx_denoise([x], SR, L.FxDenoiseParams.make(SR, 1, mode=0), noise=np.stack([z, z], axis=1))
    old = os.environ.get("RVCX_ARENA_GB")               # an item that does not fit the arena budget on its own
    os.environ["RVCX_ARENA_GB"] = "0"
    try:
        refused("600 frames needs")
    finally:
        if old is None:
            del os.environ["RVCX_ARENA_GB"]
        else:
            os.environ["RVCX_ARENA_GB"] = old
    with pytest.raises(L.RvcxError, match="skipped"):
        ctx.fx_denoise_taps(x, SR, L.FxDenoiseParams.make(SR, 1, strength=0.0))
    assert ctx.fx_denoise([x], SR)[0].shape == (600,)                       # the context works on


# ---- the mirror modules ----------------------------------------------------------------------------------------------------------
def _pcm(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def test_reduce_noise_through_files(ctx, tmp_path):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    L = _L()
    sr = 16000
    x, _, _ = R.tone_in_noise(sr, 1.0, seed=3, gate=(0.25, 0.5))
    mono, stereo = _pcm(x), np.stack([_pcm(x), _pcm(x[::-1])], axis=1)
    clip = _pcm(0.01 * np.random.default_rng(4).standard_normal(sr // 2))
    wavfile.write(str(tmp_path / "m.wav"), sr, mono)
    wavfile.write(str(tmp_path / "s.wav"), sr, stereo)
    wavfile.write(str(tmp_path / "z.wav"), sr, clip)
    f32 = lambda a: (a.astype(np.float64) / 32768.0).astype(np.float32)      # noqa: E731  (what read_audio hands over)
    M.reduce_noise(str(tmp_path / "m.wav"), str(tmp_path / "m_out.wav"), 0.8)
    sr2, got = wavfile.read(str(tmp_path / "m_out.wav"))
    want = ctx.fx_denoise([f32(mono)], sr, L.FxDenoiseParams.make(sr, 1, mode=1, strength=0.8))[0]
    assert sr2 == sr and got.dtype == np.int16 and np.array_equal(got, _pcm(want)) and not np.array_equal(got, mono)
    M.reduce_noise(str(tmp_path / "m.wav"), str(tmp_path / "m_prof.wav"), 1.0, mode="profile", noise_path=str(tmp_path / "z.wav"),
                   n_std=2.0)
    want = ctx.fx_denoise([f32(mono)], sr, L.FxDenoiseParams.make(sr, 1, mode=0, strength=1.0, n_std=2.0), noise=f32(clip))[0]
    assert np.array_equal(wavfile.read(str(tmp_path / "m_prof.wav"))[1], _pcm(want))
    M.reduce_noise(str(tmp_path / "s.wav"), str(tmp_path / "s0.wav"), 0.0)                # strength 0 copies the samples
    assert np.array_equal(wavfile.read(str(tmp_path / "s0.wav"))[1], stereo)
    outs = M.reduce_noise_many([(str(tmp_path / "m.wav"), str(tmp_path / "a.wav")), (str(tmp_path / "s.wav"), str(tmp_path / "b.wav")),
                                (str(tmp_path / "m.wav"), str(tmp_path / "c.flac"))], 0.8)
    assert outs == [str(tmp_path / n) for n in ("a.wav", "b.wav", "c.flac")]
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "m_out.wav").read_bytes()
    want = ctx.fx_denoise([f32(stereo)], sr, L.FxDenoiseParams.make(sr, 2, mode=1, strength=0.8))[0]
    assert np.array_equal(wavfile.read(str(tmp_path / "b.wav"))[1], _pcm(want))
    for bad in (dict(strength=1.5), dict(mode="spectral"), dict(noise_path=str(tmp_path / "z.wav")),
                dict(mode="profile", noise_path=str(tmp_path / "s.wav")), dict(slope=0.0)):
        kw = dict(bad)
        with pytest.raises(ValueError):
            M.reduce_noise(str(tmp_path / "m.wav"), str(tmp_path / "bad.wav"), kw.pop("strength", 0.7), **kw)
    assert not (tmp_path / "bad.wav").exists()


def test_process_audio_cleans_the_vocal(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    L = _L()
    monkeypatch.setattr(M, "OUTPUT_DIR", str(tmp_path / "output"))
    sr = 16000
    x, _, _ = R.tone_in_noise(sr, 1.0, seed=5, gate=(0.25, 0.5))
    wavfile.write(str(tmp_path / "v.wav"), sr, _pcm(x))
    wavfile.write(str(tmp_path / "i.wav"), sr, np.zeros((sr, 2), np.int16))
    fx = list(L.FX_UI_DEFAULTS.values())
    for use_effects in (False, True):
        args = (str(tmp_path / "v.wav"), str(tmp_path / "i.wav"), *fx, "wav", 0, 0, use_effects)
        plain = open(M.process_audio(*args), "rb").read()
        assert open(M.process_audio(*args, vocal_denoise=0.0), "rb").read() == plain          # byte for byte at 0.0
        cleaned = open(M.process_audio(*args, vocal_denoise=0.9), "rb").read()
        assert cleaned != plain and len(cleaned) == len(plain)
        many = M.process_audio_many([args + (str(tmp_path / "m1.wav"),), args + (str(tmp_path / "m2.wav"),)], vocal_denoise=0.9)
        assert [open(p, "rb").read() for p in many] == [cleaned, cleaned]
        many = M.process_audio_many([args + (str(tmp_path / "m3.wav"),)], vocal_denoise=0.0)
        assert open(many[0], "rb").read() == plain
    # without the board the cover is the cleaned vocal (the instrumental is silent): the Context call on the same samples
    args = (str(tmp_path / "v.wav"), str(tmp_path / "i.wav"), *fx, "wav", 0, 0, False)
    _, cover = wavfile.read(M.process_audio(*args, vocal_denoise=0.9))
    v = (_pcm(x).astype(np.float64) / 32768.0).astype(np.float32)
    from polgen_rvc_amd.infer import _state
    want = _state.context().fx_denoise([np.stack([v, v], axis=1)], sr, L.FxDenoiseParams.make(sr, 2, mode=1, strength=0.9))[0]
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


def test_rvc_infer_clean_audio(ctx, tmp_path):
    from polgen_rvc_amd.infer import infer as I
    from polgen_rvc_amd.infer.audio import write_output
    L = _L()
    tgt_sr = 48000
    x, _, _ = R.tone_in_noise(16000, 1.0, seed=6, gate=(0.25, 0.5))
    o, _, _ = R.tone_in_noise(tgt_sr, 1.0, seed=7, gate=(0.25, 0.5))
    out = _pcm(o)
    write_output(str(tmp_path / "in.wav"), _pcm(x), 16000)
    hub = _StubHubert(ctx)

    def run(fn, name, **kw):
        vc = _StubVC(out)
        fn(None, 0, str(tmp_path / "in.wav"), str(tmp_path / name), 0.0, "rmvpe+", {"f0": 1}, "v2", None, 3, tgt_sr, 1.0, 0.33, 128,
           vc, hub, **kw)
        return (tmp_path / name).read_bytes(), vc.seen[0]

    plain, fed = run(I.rvc_infer, "plain.wav")
    same, fed_none = run(I.rvc_infer_clean, "none.wav", clean_audio=None)
    assert same == plain and np.array_equal(fed, fed_none)                                 # None: the bytes are unchanged
    p16 = L.FxDenoiseParams.make(16000, 1, mode=1, strength=0.6)
    p48 = L.FxDenoiseParams.make(tgt_sr, 1, mode=1, strength=0.6)
    want_in = ctx.fx_denoise([fed.astype(np.float32)], 16000, p16)[0].astype(np.float64)
    want_out = _pcm(ctx.fx_denoise([out.astype(np.float32) / np.float32(32768.0)], tgt_sr, p48)[0])
    write_output(str(tmp_path / "want.wav"), want_out, tgt_sr)
    cleaned_bytes = (tmp_path / "want.wav").read_bytes()
    got, fed_in = run(I.rvc_infer_clean, "input.wav", clean_audio="input", clean_strength=0.6)
    assert got == plain and np.array_equal(fed_in, want_in) and not np.array_equal(fed_in, fed)
    got, fed_out = run(I.rvc_infer_clean, "output.wav", clean_audio="output", clean_strength=0.6)
    assert got == cleaned_bytes and got != plain and np.array_equal(fed_out, fed)
    got, fed_both = run(I.rvc_infer_clean, "both.wav", clean_audio="both", clean_strength=0.6)
    assert got == cleaned_bytes and np.array_equal(fed_both, want_in)
    # rvc_infer_many: the same bytes per file
    vc = _StubVC(out)
    I.rvc_infer_many(None, 0, [str(tmp_path / "in.wav")] * 2, [str(tmp_path / "m0.wav"), str(tmp_path / "m1.wav")], 0.0, "rmvpe+",
                     {"f0": 1}, "v2", None, 3, tgt_sr, 1.0, 0.33, 128, vc, hub, clean_audio="both", clean_strength=0.6)
    assert (tmp_path / "m0.wav").read_bytes() == cleaned_bytes == (tmp_path / "m1.wav").read_bytes()
    assert np.array_equal(vc.seen[0], want_in) and np.array_equal(vc.seen[1], want_in)
    vc = _StubVC(out)
    I.rvc_infer_many(None, 0, [str(tmp_path / "in.wav")], [str(tmp_path / "m2.wav")], 0.0, "rmvpe+", {"f0": 1}, "v2", None, 3,
                     tgt_sr, 1.0, 0.33, 128, vc, hub)
    assert (tmp_path / "m2.wav").read_bytes() == plain
    for bad in (dict(clean_audio="loud"), dict(clean_audio="input", clean_strength=1.5)):
        with pytest.raises(ValueError):
            run(I.rvc_infer_clean, "bad.wav", **bad)
