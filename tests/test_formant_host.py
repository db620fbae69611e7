"""CPU: include/rvcx.h stages 17 and 18 -- the host twin of the envelope transfer against the float64 restatement
(tests/formant_reference.py) link by link and whole, the corners of every parameter, the skip rule, the refusals, the
behaviour conditions on the float64 restatement itself and on the twin, and the refusals of the mirror modules before any file
exists.

Shapes: sr = 8000 (N = 512, H = 128, nb = 257) with n of 1, H - 1, H, 5 H + 3 and 4000; one item of 3 N samples each at 44100,
48000 and 192000 Hz; nc 1 and N / 8; iterations 0 and 16; ratio 0.5 and 2; amount 0.5; max_gain_db 0; keep_energy 0."""
import ctypes as C

import numpy as np
import pytest

import formant_reference as R
from stretch_reference import rms, signal

SR = 8000
# Bars: 3x the worst case measured on the host twin (LABNOTES 25); the conditions are what a wrong link would exceed.
# 1. |D - float64 rfft| over the frame's largest magnitude: measured 5.5e-8 (the twin transforms in double and rounds once:
#    half a float32 ulp of the top).
BAR_D, CONDITION_D = 1.7e-7, 1e-5
# 2. E against the restatement on the twin's D, absolute (nepers): measured 6.0e-7 (E is rounded to float32 after every lift,
#    values up to 23; a wrong lifter or a missing iteration: 1e-2).
BAR_E, CONDITION_E = 1.8e-6, 1e-3
# 3. g against the restatement on the twin's E and Es, relative: measured 1.07e-6 (W and d rounded to float32, expf).
BAR_G, CONDITION_G = 3.2e-6, 1e-3
# 4. s from the twin's D and g: equal bit for bit (the sums are double in a defined order).
# 5. y against the float64 synthesis from the twin's D, g and s, over the item's peak: measured 1.14e-7 (fl(g s) and y
#    rounded once each).
BAR_Y, CONDITION_Y = 3.4e-7, 1e-4
# 6. the stage whole against the all-float64 restatement, relative RMS: measured 9.2e-8.
BAR_E2E, CONDITION_E2E = 2.8e-7, 1e-3
assert BAR_D <= CONDITION_D and BAR_E <= CONDITION_E and BAR_G <= CONDITION_G and BAR_Y <= CONDITION_Y and BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def host_run(x, sr, source, **kw):
    L = _L()
    return L.fx_formant_host(x, sr, L.FxFormantParams.make(sr, 1, **kw), source=source, taps=True)


new_worst, check_links, CORNERS = R.new_worst, R.check_links, R.CORNERS


def check_bars(worst, what):
    print(f"{what}: D {worst['D']:.3e} of the frame's top, E {worst['E']:.3e}, g {worst['g']:.3e} relative, "
          f"y {worst['y']:.3e} of the peak")
    assert worst["D"] <= BAR_D and worst["E"] <= BAR_E and worst["g"] <= BAR_G and worst["y"] <= BAR_Y, worst


def test_links_at_8k():
    worst = new_worst()
    for i, n in enumerate((1, 127, 128, 5 * 128 + 3, 4000)):
        check_links(host_run, signal(n, 20 + i), SR, worst, ratio=R.ratio_of(4.0))
        check_links(host_run, signal(n, 30 + i), SR, worst, source=signal(n, 40 + i))
    check_bars(worst, "host twin at 8 kHz")


def test_links_at_the_corners():
    assert R.quefrency_bins(SR, 0.125) == 1 and R.quefrency_bins(SR, 8.0) == 512 // 8
    worst = new_worst()
    for i, kw in enumerate(CORNERS):
        kw = dict(dict(ratio=R.ratio_of(-3.0)), **kw)
        check_links(host_run, signal(1500, 50 + i), SR, worst, **kw)
    check_links(host_run, signal(1500, 60), SR, worst, source=signal(1500, 61), amount=0.5, keep_energy=0)
    check_bars(worst, "host twin at the corners")


@pytest.mark.parametrize("sr", (44100, 48000, 192000))
def test_links_at_other_rates(sr):
    worst = new_worst()
    n = 3 * R.geometry(sr)[0]
    check_links(host_run, signal(n, 70, sr), sr, worst, ratio=R.ratio_of(-4.0))
    check_links(host_run, signal(n, 71, sr), sr, worst, source=signal(n, 72, sr))
    check_bars(worst, f"host twin at {sr} Hz")


def test_envelope_alone():
    """rvcx_fx_formant_envelope_host on a log spectrum of its own: the lifter's corners at every N"""
    L = _L()
    rng = np.random.default_rng(3)
    worst = 0.0
    for N, cases in ((512, ((1, 0), (1, 16), (64, 0), (64, 16), (12, 8))), (2048, ((72, 8),)), (8192, ((1024, 8), (288, 8)))):
        for nc, it in cases:
            Lx = (rng.standard_normal(N // 2 + 1) * 3.0 - 5.0).astype(np.float32)
            E = L.fx_formant_envelope_host(Lx, N, nc, it)
            ref = R.envelope(Lx, N, nc, it)
            worst = max(worst, float(np.abs(E - ref).max()))
            if it == 16:                                   # the iteration lifts the envelope onto the peaks
                assert (ref >= R.envelope(Lx, N, nc, 0) - 1e-9).all()
    print(f"envelope alone: {worst:.3e}")
    assert worst <= BAR_E
    for bad in ((500, 8, 8), (512, 0, 8), (512, 65, 8), (512, 8, 17), (512, 8, -1), (16384, 8, 8)):
        with pytest.raises(L.RvcxError):
            L.fx_formant_envelope_host(np.zeros(bad[0] // 2 + 1, np.float32), *bad)


def test_gain_limit_zeros_and_the_warps_clamp():
    L = _L()
    x = signal(3000, 5)
    # max_gain_db 0 leaves only s_t, which is then 1: the output is the resynthesis of the input
    # (links 1 and 5 then hold y to the float64 resynthesis of the input's own spectra)
    y, t = L.fx_formant_host(x, SR, L.FxFormantParams.make(SR, 1, ratio=1.5, max_gain_db=0.0), taps=True)
    assert (t["g"] == 1.0).all() and (t["s"] == 1.0).all()
    worst = new_worst()
    assert np.array_equal(check_links(host_run, x, SR, worst, ratio=1.5, max_gain_db=0.0), y)
    check_bars(worst, "host twin at max_gain_db 0")
    # the gain never leaves the limit
    lim = 6.0 * np.log(10.0) / 20.0
    _, t = L.fx_formant_host(x, SR, L.FxFormantParams.make(SR, 1, ratio=2.0, max_gain_db=6.0), taps=True)
    assert np.abs(np.log(t["g"].astype(np.float64))).max() <= lim * (1 + 1e-6) and (np.abs(np.log(t["g"])) > 0.99 * lim).any()
    # ratio 0.5: every bin from nb / 2 on takes the last bin's envelope
    _, t = L.fx_formant_host(x, SR, L.FxFormantParams.make(SR, 1, ratio=0.5, max_gain_db=48.0, keep_energy=0), taps=True)
    nb = t["E"].shape[1]
    want = np.exp(np.clip(t["Es"][:, nb - 1:nb].astype(np.float64) - t["E"][:, nb // 2:], -48 * np.log(10) / 20, 48 * np.log(10) / 20))
    assert np.abs(t["g"][:, nb // 2:] / want - 1.0).max() <= BAR_G and (t["s"] == 1.0).all()
    # all-zero input: all-zero output with g = 1
    z = np.zeros(1000, np.float32)
    for src in (None, z):
        y, t = L.fx_formant_host(z, SR, L.FxFormantParams.make(SR, 1, ratio=1.25), source=src, taps=True)
        assert not y.any() and not t["D"].any() and (t["g"] == 1.0).all() and (t["s"] == 1.0).all()


def test_stereo_and_sources():
    L = _L()
    a, b, sa, sb = (signal(2000, 80 + i) for i in range(4))
    st = np.ascontiguousarray(np.stack([a, b], axis=1))
    p1, p2 = L.FxFormantParams.make(SR, 1, semitones=3.0), L.FxFormantParams.make(SR, 2, semitones=3.0)
    y2 = L.fx_formant_host(st, SR, p2)
    assert np.array_equal(y2[:, 0], L.fx_formant_host(a, SR, p1)) and np.array_equal(y2[:, 1], L.fx_formant_host(b, SR, p1))
    y2 = L.fx_formant_host(st, SR, p2, source=np.stack([sa, sb], axis=1))
    ya = L.fx_formant_host(a, SR, p1, source=sa)
    assert np.array_equal(y2[:, 0], ya) and np.array_equal(y2[:, 1], L.fx_formant_host(b, SR, p1, source=sb))
    assert not np.array_equal(ya, L.fx_formant_host(a, SR, p1)) and not np.array_equal(ya, L.fx_formant_host(a, SR, p1, source=sb))
    with pytest.raises(L.RvcxError, match="same length"):
        L.fx_formant_host(a, SR, p1, source=sa[:-1])
    with pytest.raises(L.RvcxError, match="same length"):
        L.fx_formant_host(a, SR, p1, source=np.stack([sa, sb], axis=1))


@pytest.fixture(scope="module")
def whole():
    """the end-to-end cases and their all-float64 restatement (computed once)"""
    x8, s8, xv = signal(16000, 90), signal(16000, 91), R.vowel(48000, 110.0, 150.0)
    cases = [(x8, SR, None, dict(ratio=R.ratio_of(4.0))), (x8, SR, s8, dict()), (xv, 48000, None, dict(ratio=R.ratio_of(-4.0)))]
    return [(x, sr, src, kw, R.stage(x, sr, src=src, **kw)["y"]) for x, sr, src, kw in cases]


def test_stage_whole_against_float64(whole):
    L = _L()
    worst = 0.0
    for x, sr, src, kw, ref in whole:
        y = L.fx_formant_host(x, sr, L.FxFormantParams.make(sr, 1, **kw), source=src)
        worst = max(worst, rms(y - ref) / rms(ref))
    print(f"host twin vs float64: {worst:.3e} relative RMS")
    assert worst <= BAR_E2E


def test_stage_18_is_stage_14_then_the_transfer():
    L = _L()
    x = signal(6000, 95)
    st = np.ascontiguousarray(np.stack([x, signal(6000, 96)], axis=1))
    for item in (x, st):
        ch = 1 if item.ndim == 1 else 2
        shifted = L.fx_pitch_shift_host(item, SR, 5.0)
        want = L.fx_formant_host(shifted, SR, L.FxFormantParams.make(SR, ch), source=item)
        assert np.array_equal(L.fx_pitch_shift_formant_host(item, SR, 5.0), want) and not np.array_equal(want, shifted)
        # its ratio is not read; amount 0 leaves stage 14; P == sr returns the input
        assert np.array_equal(L.fx_pitch_shift_formant_host(item, SR, 5.0, L.FxFormantParams.make(SR, ch, ratio=1.7)), want)
        assert np.array_equal(L.fx_pitch_shift_formant_host(item, SR, 5.0, L.FxFormantParams.make(SR, ch, amount=0.0)), shifted)
        assert np.array_equal(L.fx_pitch_shift_formant_host(item, SR, 0.0).view(np.uint32), item.view(np.uint32))
    ref = R.pitch_shift_preserved(x, SR, 5.0)
    got = L.fx_pitch_shift_formant_host(x, SR, 5.0)
    print(f"stage 18, host twin vs float64: {rms(got - ref) / rms(ref):.3e} relative RMS (unpinned: stage 13 decides per bin)")


def test_skip():
    L = _L()
    x = signal(4000, 5)
    x[7] = np.float32(-0.0)
    st = np.ascontiguousarray(np.stack([x, signal(4000, 6)], axis=1))
    for item in (x, st):
        ch = 1 if item.ndim == 1 else 2
        for kw in (dict(ratio=1.0), dict(ratio=1.5, amount=0.0)):
            y = L.fx_formant_host(item, SR, L.FxFormantParams.make(SR, ch, **kw))
            assert np.array_equal(y.view(np.uint32), item.view(np.uint32))
        y = L.fx_formant_host(item, SR, L.FxFormantParams.make(SR, ch, amount=0.0), source=item[::-1].copy())
        assert np.array_equal(y.view(np.uint32), item.view(np.uint32))
        y = L.fx_formant_host(item, SR, L.FxFormantParams.make(SR, ch), source=item[::-1].copy())     # ratio 1 with a source runs
        assert not np.array_equal(y, item)
    with pytest.raises(L.RvcxError, match="skipped"):
        L.fx_formant_host(x, SR, L.FxFormantParams.make(SR, 1), taps=True)


def test_errors_write_nothing():
    L = _L()
    lib = L.lib()
    assert C.sizeof(L.FxFormantParams) == 32
    x = signal(600, 6)
    y = np.full(600, 7.0, np.float32)

    def refused(what, n=600, sr=SR, ch=1, **kw):
        p = L.FxFormantParams.make(sr, ch, **dict(dict(ratio=1.5), **kw))
        rc = lib.rvcx_fx_formant_host(x.ctypes.data, n, None, C.byref(p), y.ctypes.data, None, None, None, None, None)
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
    refused("positive", quefrency_ms=-1.0)
    refused("finite", quefrency_ms=float("nan"))
    refused("N / 8", quefrency_ms=0.1)                     # nc = 0
    refused("N / 8", quefrency_ms=8.2)                     # nc = 65 > 512 / 8
    refused("sample rate", sr=7000)
    refused("channels", ch=3)
    refused("frames", n=0)
    for s in (12.5, float("nan")):
        rc = lib.rvcx_fx_pitch_shift_formant_host(x.ctypes.data, 600, 1, SR, s, None, y.ctypes.data)
        assert rc == -1 and (y == 7.0).all()
    with pytest.raises(L.RvcxError):
        L.FxFormantParams.make(SR, 1, semitones=12.5)
    with pytest.raises(L.RvcxError):
        L.FxFormantParams.make(SR, 1, semitones=1.0, ratio=1.1)
    with pytest.raises(L.RvcxError):
        L.FxFormantParams.make(SR, 1, strength=1.0)
    assert L.FxFormantParams.make(SR, 1, semitones=12.0).ratio == 2.0 and L.FxFormantParams.make(SR, 1, semitones=-12.0).ratio == 0.5
    assert L.fx_formant_frames(4000, SR) == (32, 512, 12) and L.fx_formant_frames(1, 192000, 2.0) == (1, 8192, 384)


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_behaviour():
    return R.behaviour(dict(shift=R.shift, pitch=R.pitch_shift, preserved=R.pitch_shift_preserved))


def test_behaviour_of_the_definition(reference_behaviour):
    """the table of the issue on the float64 restatement: the formants move and F0 and level stay; through a key change the
    formants stay where stage 14 alone moves them"""
    f = reference_behaviour
    print("float64: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    assert len(f) == 3 * (2 * 3 + 2 * 4)
    R.check_behaviour(f)


def test_behaviour_of_the_host_twin(reference_behaviour):
    L = _L()
    f = R.behaviour(dict(shift=lambda x, sr, st: L.fx_formant_host(x, sr, L.FxFormantParams.make(sr, 1, semitones=st)),
                         preserved=lambda x, sr, st: L.fx_pitch_shift_formant_host(x, sr, st)))
    print("host twin: " + ", ".join(f"{k} {v:.4f}" for k, v in f.items()))
    R.check_behaviour(f)
    for k, v in f.items():                                  # and it is the definition's behaviour, not merely inside the bands
        if k.startswith("share") or k.startswith("shift"):
            assert abs(v - reference_behaviour[k]) <= 1e-3, (k, v, reference_behaviour[k])


# ---- the mirror modules: every refusal before a file exists ---------------------------------------------------------------------
def test_mirror_modules_refuse_before_writing(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.infer import infer as I
    from polgen_rvc_amd.scripts import audio_processing as M
    pcm = np.clip(np.rint(signal(4000, 7, 16000).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "m.wav"), 16000, pcm)
    out = tmp_path / "bad.wav"
    for bad in (dict(semitones=12.5), dict(semitones=float("nan")), dict(semitones=2.0, amount=1.5),
                dict(semitones=2.0, quefrency_ms=0.0), dict(semitones=2.0, quefrency_ms=50.0)):
        kw = dict(bad)
        with pytest.raises(ValueError):
            M.shift_formants(str(tmp_path / "m.wav"), str(out), kw.pop("semitones"), **kw)
        with pytest.raises(ValueError):
            M.shift_formants_many([(str(tmp_path / "m.wav"), str(tmp_path / "ok.wav")), (str(tmp_path / "m.wav"), str(out))],
                                  bad["semitones"], **kw)
    with pytest.raises(ValueError):
        M.shift_pitch(str(tmp_path / "m.wav"), str(out), 12.5, preserve_formants=True)
    assert not out.exists() and not (tmp_path / "ok.wav").exists()
    # process_audio(_many): vocal_formant is refused beside the paths and the format, before Voice_Stereo.wav is written
    monkeypatch.setattr(M, "OUTPUT_DIR", str(tmp_path / "output"))
    args = (str(tmp_path / "m.wav"), str(tmp_path / "m.wav"), *_L().FX_UI_DEFAULTS.values(), "wav", 0, 0, False)
    for bad in (12.5, float("nan")):
        with pytest.raises(ValueError):
            M.process_audio(*args, vocal_denoise=0.5, vocal_formant=bad)
        with pytest.raises(ValueError):
            M.process_audio_many([args + (str(out),)], vocal_denoise=0.5, vocal_formant=bad)
    assert not (tmp_path / "output").exists() and not out.exists()
    # 0 semitones copies the samples without a device
    M.shift_formants(str(tmp_path / "m.wav"), str(tmp_path / "same.wav"), 0.0)
    assert np.array_equal(wavfile.read(str(tmp_path / "same.wav"))[1], pcm)
    for bad in (dict(formant_shift=12.5), dict(formant_shift=float("nan")), dict(formant_shift=2.0, formant_quefrency_ms=0.0),
                dict(formant_shift=2.0, formant_quefrency_ms=40.0)):
        with pytest.raises(ValueError):
            I._formant_check(bad["formant_shift"], bad.get("formant_quefrency_ms", 1.5))
    assert I._formant_check(0.0, 1.5) is None and I._formant_check(3.0, 1.0).quefrency_ms == 1.0
