"""GPU: include/rvcx.h stages 13 and 14 -- the time stretch and the pitch shift on the device, checked in links so that a
near-tie in a peak decision cannot decide a test: D against float64 rfft, own against the restatement applied to the device's
D, TH against float64 atan2 of the device's D, R against the integer scan of the restatement on the device's own and TH (and
against itself under other chunk and segment lengths), y against the float64 synthesis from the device's D, own, TH and R;
then batch and grouping in every bit, the stage whole against the all-float64 restatement and the host twin, the identity,
the skip rule, the errors and the mirror module.

Shapes: sr = 8000 (N = 512, H = 128, nb = 257); lengths 1, 127, 128, 511, 512, 513, 4000 and those that give J = 1, Lc - 1, Lc,
Lc + 1 and 3 Lc + 1 output frames for the scan chunk Lc; P / 8000 in {8000, 4000, 16000, 9514, 7551}; mono and stereo; an
all-zero item and one with 0.2 s of exact zeros in the middle; one 1 s item each at 44100, 48000 and 192000 Hz."""
import os

import numpy as np
import pytest

import stretch_reference as R
from stretch_reference import rms, signal, sine_peak_hz, tones, unit_diff

pytestmark = pytest.mark.gpu

SR = 8000
RATIOS = (8000, 4000, 16000, 9514, 7551)
# Bars: 3x the worst case measured on the GPU at the first run (LABNOTES 22); each condition is the issue's.
# 1. |D - float64 rfft| over the frame's largest magnitude: measured 1.9e-7 (1.6e-7 at N = 8192).  fp32 radix-2 theory: about
#    1e-6; a wrong twiddle gives order 1.
BAR_D, CONDITION_D = 6e-7, 1e-5
# 3. TH against float64 atan2 of the device's D, in units of 2^-32 turn: measured 202 (one float32 step of an angle near pi
#    is 163 units; the host's atan2f measures 166).
BAR_TH, CONDITION_TH = 610, 1 << 12
# 5. y against the float64 synthesis from the device's own D, own, TH and R, over the item's peak: measured 2.2e-7 (float32
#    transform, angle and numerator).
BAR_Y, CONDITION_Y = 7e-7, 1e-4
# 7. the stage whole: relative RMS difference to the all-float64 restatement and to the host twin: measured 9.1e-5 to both
#    (the twin against the restatement: 7.6e-7).  The device's float32 D differs from the rounded float64 D in its last bits,
#    so a near-tie between two bins may fall the other way and hand a few bins to the neighbouring peak; links 1 - 5 show
#    that every stage is right given its input.
BAR_E2E, CONDITION_E2E = 3e-4, 1e-3
assert BAR_D <= CONDITION_D and BAR_TH <= CONDITION_TH and BAR_Y <= CONDITION_Y and BAR_E2E <= CONDITION_E2E


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def n_for_frames(J, P, Q=SR, H=128):
    """a length whose stretch has exactly J output frames (J = ceil(T P / Q), T = floor(n / H) + 1)"""
    for T in range(1, 4 * J + 4):
        if -(-T * P // Q) == J:
            return max((T - 1) * H, 1)
    return None


def lengths(P):
    Lc = _L().fx_stretch_chunk()
    js = [n_for_frames(J, P) for J in (1, Lc - 1, Lc, Lc + 1, 3 * Lc + 1)]
    return [1, 127, 128, 511, 512, 513, 4000] + [n for n in js if n]


def check_links(ctx, x, sr, P, Q, worst):
    """links 1 - 5 on one channel; returns the device's y"""
    n = x.shape[0]
    N, H, nb = R.geometry(sr)
    T, J = R.frames(n, sr, P, Q)
    y, t = ctx.fx_stretch_taps(x, sr, P, Q)
    assert y.shape == (R.stretch_len(n, P, Q),) and t["D"].shape == (T + 2, nb, 2) and t["R"].shape == (J, nb)
    D32 = R.pairs_to_complex(t["D"])
    assert not D32[T:].any() and not t["TH"][T:].any()
    ref_D = R.analysis(x, sr)
    top = np.abs(ref_D).max(axis=1)
    err = np.abs(ref_D - D32.astype(np.complex128)).max(axis=1)
    worst["D"] = max(worst["D"], float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0)
    assert not err[top == 0].any()
    assert np.array_equal(t["own"], R.owners(D32)), (n, P)
    worst["TH"] = max(worst["TH"], unit_diff(t["TH"], R.th_of(D32, as_float32=False)))
    assert np.array_equal(t["R"], R.scan(t["own"], t["TH"], J, P, Q)), (n, P)
    ref = R.stretch(x, sr, P, Q, D32=D32, own=t["own"], TH=t["TH"], R=t["R"])["y"]
    worst["y"] = max(worst["y"], float(np.abs(y - ref).max()) / max(float(np.abs(x).max()), 1e-30))
    return y


def check_bars(worst, what):
    print(f"{what}: D {worst['D']:.3e} of the frame's top, TH {worst['TH']} units, y {worst['y']:.3e} of the peak")
    assert worst["D"] <= BAR_D and worst["TH"] <= BAR_TH and worst["y"] <= BAR_Y, worst


@pytest.mark.parametrize("P", RATIOS)
def test_links_at_8k(ctx, P):
    worst = dict(D=0.0, TH=0, y=0.0)
    for i, n in enumerate(lengths(P)):
        check_links(ctx, signal(n, 20 + i), SR, P, SR, worst)
    check_bars(worst, f"P {P}")


@pytest.mark.parametrize("sr", (44100, 48000, 192000))
def test_links_at_other_rates(ctx, sr):
    worst = dict(D=0.0, TH=0, y=0.0)
    check_links(ctx, signal(sr, 40, sr), sr, R.pitch_ratio(sr, 3), sr, worst)
    check_bars(worst, f"sr {sr}")


def test_zeros_and_stereo(ctx):
    """an all-zero item returns zeros; 0.2 s of exact zeros in the middle pass the links; a stereo item is its two channels"""
    worst = dict(D=0.0, TH=0, y=0.0)
    z = np.zeros(3000, np.float32)
    y, t = ctx.fx_stretch_taps(z, SR, 9514, SR)
    assert not y.any() and not t["R"].any() and np.array_equal(t["own"], np.tile(np.arange(257), (t["own"].shape[0], 1)))
    assert not ctx.fx_pitch_shift([z], SR, 3.0)[0].any()
    x = signal(8000, 31)
    x[3000:4600] = 0.0
    a = check_links(ctx, x, SR, 9514, SR, worst)
    b = check_links(ctx, signal(8000, 32), SR, 9514, SR, worst)
    check_bars(worst, "zeros in the middle")
    st = np.ascontiguousarray(np.stack([x, signal(8000, 32)], axis=1))
    y2 = ctx.fx_stretch([st], SR, 9514, SR)[0]
    assert np.array_equal(y2[:, 0], a) and np.array_equal(y2[:, 1], b)
    p2 = ctx.fx_pitch_shift([st], SR, -5.0)[0]
    for c in range(2):
        assert np.array_equal(p2[:, c], ctx.fx_pitch_shift([np.ascontiguousarray(st[:, c])], SR, -5.0)[0])


def test_chunk_and_segment_lengths_change_no_bit(ctx):
    L = _L()
    Lc = L.fx_stretch_chunk()
    x = signal(n_for_frames(3 * Lc + 1, 9514), 33)
    # stereo items of two and three output frames: with one-frame segments a segment's first sample lies in front of the
    # row (clamped to 0), and the rows of an item end in the same launches
    short = [np.ascontiguousarray(np.stack([signal(n, 90 + n), signal(n, 91 + n)], axis=1)) for n in (129, 200, 255, 256)]
    want = {}
    try:
        for chunk, seg in ((0, 0), (1, 0), (2, 0), (0, Lc), (0, 3 * Lc), (1, 1), (2, 3), (5, 2 * Lc + 3)):
            L.fx_stretch_override(chunk, seg)
            for P in (9514, 4000, 16000):
                y, t = ctx.fx_stretch_taps(x, SR, P, SR)
                got = (y.tobytes(), t["R"].tobytes(), t["own"].tobytes(), t["TH"].tobytes())
                assert want.setdefault(P, got) == got, (chunk, seg, P)
            st = ctx.fx_pitch_shift([np.stack([x, x[::-1]], axis=1)], SR, 7.0)[0].tobytes()
            assert want.setdefault("shift", st) == st, (chunk, seg)
            for P in (8000, 9514, 16000):
                got = [y.tobytes() for y in ctx.fx_stretch(short, SR, P, SR)]
                assert want.setdefault(("short", P), got) == got, (chunk, seg, P)
                one = [ctx.fx_stretch([s], SR, P, SR)[0].tobytes() for s in short]
                assert one == got, (chunk, seg, P)
    finally:
        L.fx_stretch_override(0, 0)
    assert L.fx_stretch_chunk() == Lc


def test_batch_and_grouping_change_no_bit(ctx):
    for C in (1, 2):
        xs = []
        for i, n in enumerate((1, 127, 513, 4000, 12289, 128)):
            x = signal(n, 50 + i) if C == 1 else np.stack([signal(n, 50 + i), signal(n, 70 + i)], axis=1)
            xs.append(np.ascontiguousarray(x))
        for P in (9514, 7551):
            single = [ctx.fx_stretch([x], SR, P, SR)[0].tobytes() for x in xs]
            shifted = [ctx.fx_pitch_shift([x], SR, 3.0)[0].tobytes() for x in xs]
            assert [y.tobytes() for y in ctx.fx_stretch(xs, SR, P, SR)] == single
            assert [y.tobytes() for y in ctx.fx_pitch_shift(xs, SR, 3.0)] == shifted
            old = os.environ.get("RVCX_MAX_BATCH")
            os.environ["RVCX_MAX_BATCH"] = "2"
            try:
                grouped = [y.tobytes() for y in ctx.fx_stretch(xs, SR, P, SR)]
                groups = ctx.fx_last_passes()[1]
                grouped_shift = [y.tobytes() for y in ctx.fx_pitch_shift(xs, SR, 3.0)]
            finally:
                if old is None:
                    del os.environ["RVCX_MAX_BATCH"]
                else:
                    os.environ["RVCX_MAX_BATCH"] = old
            assert groups == 3 and grouped == single and grouped_shift == shifted


@pytest.fixture(scope="module")
def whole():
    """the three signals of 16000 samples and, per shift, the all-float64 restatement and the host twin (computed once)"""
    L = _L()
    xs = {k: v.astype(np.float32) for k, v in tones().items()}
    ref = {(k, s): (R.pitch_shift(x, SR, s), L.fx_pitch_shift_host(x, SR, s)) for k, x in xs.items()
           for s in (-12, -5, 0.37, 3, 7, 12)}
    return xs, ref


def test_stage_whole_against_float64_and_host_twin(ctx, whole):
    xs, ref = whole
    worst = dict(ref=0.0, host=0.0, lo=9.0, hi=0.0, hz=0.0)
    names = list(xs)
    for s in (-12, -5, 0.37, 3, 7, 12):
        ys = ctx.fx_pitch_shift([xs[k] for k in names], SR, s)
        for k, y in zip(names, ys):
            x, n = xs[k], xs[k].shape[0]
            yr, yh = ref[(k, s)]
            assert y.shape == x.shape
            worst["ref"] = max(worst["ref"], rms(y - yr) / rms(yr))
            worst["host"] = max(worst["host"], rms(y - yh) / rms(yh))
            ratio = rms(y[2000:n - 2000]) / rms(x[2000:n - 2000])
            worst["lo"], worst["hi"] = min(worst["lo"], ratio), max(worst["hi"], ratio)
            if k == "sine":
                worst["hz"] = max(worst["hz"], abs(sine_peak_hz(y, SR) - 440.0 * R.pitch_ratio(SR, s) / SR))
    print(f"device vs float64 {worst['ref']:.3e}, vs host twin {worst['host']:.3e} relative RMS; level {worst['lo']:.4f} .. "
          f"{worst['hi']:.4f}; sine peak off by {worst['hz']:.4f} Hz")
    assert worst["ref"] <= BAR_E2E and worst["host"] <= BAR_E2E, worst
    assert 0.98 <= worst["lo"] and worst["hi"] <= 1.02 and worst["hz"] <= 0.5, worst


def test_identity_and_skip(ctx, whole):
    xs, _ = whole
    for k, x in xs.items():
        y = ctx.fx_stretch([x], SR, SR, SR)[0]
        assert np.abs(y - x).max() <= 1e-5 * np.abs(x).max(), k          # P = Q through the kernels
    ctx.fx_stretch([xs["sine"]], SR, 9514, SR)
    assert ctx.fx_stretch_timing()["total"] > 0.0
    st = np.ascontiguousarray(np.stack([xs["sine"], xs["glide"]], axis=1))
    for s in (0.0, 1e-4):                                                 # P == sr: bit for bit, nothing launched
        y = ctx.fx_pitch_shift([st, xs["chord"].reshape(-1, 1).repeat(2, axis=1)], SR, s)
        assert np.array_equal(y[0].view(np.uint32), st.view(np.uint32))
        assert ctx.fx_stretch_timing()["total"] == 0.0 and ctx.fx_last_passes()[1] == 0


def test_errors_write_nothing(ctx):
    import ctypes as C
    L = _L()
    lib = L.lib()
    x = signal(600, 6)
    y = np.full(2400, 7.0, np.float32)
    xp, yp, n = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(y.ctypes.data), (C.c_int64 * 1)(600)

    def refused(rc, what):
        assert rc == -1 and what in (lib.rvcx_last_error(ctx._h) or b"").decode(), (rc, lib.rvcx_last_error(ctx._h))
        assert (y == 7.0).all()

    refused(lib.rvcx_fx_pitch_shift(ctx._h, 1, xp, n, 1, SR, C.c_double(12.5), yp), "semitones")
    refused(lib.rvcx_fx_pitch_shift(ctx._h, 1, xp, n, 1, SR, C.c_double(float("nan")), yp), "finite")
    refused(lib.rvcx_fx_pitch_shift(ctx._h, 1, xp, n, 1, 7000, C.c_double(3.0), yp), "sample rate")
    refused(lib.rvcx_fx_pitch_shift(ctx._h, 1, xp, n, 3, SR, C.c_double(3.0), yp), "channels")
    refused(lib.rvcx_fx_stretch(ctx._h, 1, xp, n, 1, SR, 3999, 8000, yp), "Q / 2 <= P")
    refused(lib.rvcx_fx_stretch(ctx._h, 1, xp, n, 1, SR, 16001, 8000, yp), "Q / 2 <= P")
    refused(lib.rvcx_fx_stretch(ctx._h, 1, xp, n, 1, SR, 1 << 20, (1 << 20) + 1, yp), "Q")
    refused(lib.rvcx_fx_stretch(ctx._h, 0, xp, n, 1, SR, 8000, 8000, yp), "B < 1")
    with pytest.raises(L.RvcxError):
        ctx.fx_pitch_shift([x], SR, -12.01)
    assert ctx.fx_stretch([x], SR, 9514, SR)[0].shape == (714,)             # the context works on


# ---- the mirror module ---------------------------------------------------------------------------------------------------------
def test_process_audio_shifts_the_instrumental(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    L = _L()
    monkeypatch.setattr(M, "OUTPUT_DIR", str(tmp_path / "output"))
    sr = 16000
    t = np.arange(2 * sr) / sr
    voc = np.zeros(2 * sr, np.int16)
    inst = np.round(0.5 * np.sin(2 * np.pi * 440.0 * t) * 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "v.wav"), sr, voc)
    wavfile.write(str(tmp_path / "i.wav"), sr, np.stack([inst, inst], axis=1))
    fx = list(L.FX_UI_DEFAULTS.values())
    args = (str(tmp_path / "v.wav"), str(tmp_path / "i.wav"), *fx, "wav", 0, 0, False)
    plain = open(M.process_audio(*args), "rb").read()
    assert open(M.process_audio(*args, instrumental_pitch=0.0), "rb").read() == plain     # byte for byte at 0.0
    shifted = open(M.process_audio(*args, instrumental_pitch=3.0), "rb").read()
    assert shifted != plain and len(shifted) == len(plain)
    _, cover = wavfile.read(M.process_audio(*args, instrumental_pitch=3.0))
    want = 440.0 * R.pitch_ratio(sr, 3.0) / sr
    got = sine_peak_hz(cover[:, 0].astype(np.float64), sr)
    print(f"cover peak {got:.3f} Hz, 440 P / sr = {want:.3f} Hz")
    assert abs(got - want) <= 0.5 and abs(sine_peak_hz(wavfile.read(str(tmp_path / 'i.wav'))[1][:, 0], sr) - 440.0) <= 0.5
    mastered = M.process_audio(*args, target_lufs=-16.0, instrumental_pitch=3.0)
    assert abs(sine_peak_hz(wavfile.read(mastered)[1][:, 0].astype(np.float64), sr) - want) <= 0.5
    many = M.process_audio_many([args + (str(tmp_path / "second.wav"),), args + (str(tmp_path / "third.wav"),)],
                                instrumental_pitch=3.0)       # both instrumentals in one rvcx_fx_pitch_shift call
    assert [open(p, "rb").read() for p in many] == [shifted, shifted]
    many = M.process_audio_many([args + (str(tmp_path / "m2.wav"),), args + (str(tmp_path / "m3.wav"),)], target_lufs=-16.0,
                                instrumental_pitch=3.0)
    assert [open(p, "rb").read() for p in many] == [open(mastered, "rb").read()] * 2
    M.shift_pitch(str(tmp_path / "i.wav"), str(tmp_path / "up.wav"), 3.0)
    sr2, up = wavfile.read(str(tmp_path / "up.wav"))
    assert sr2 == sr and up.shape == (2 * sr, 2) and up.dtype == np.int16
    assert abs(sine_peak_hz(up[:, 1].astype(np.float64), sr) - want) <= 0.5
    with pytest.raises(ValueError):
        M.shift_pitch(str(tmp_path / "i.wav"), str(tmp_path / "bad.wav"), 13.0)
