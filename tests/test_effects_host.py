"""CPU: post-production without a GPU (include/rvcx.h "post-production").  The float64 restatement (tests/effects_reference.py)
is pinned on scipy.signal.lfilter; the sequential float32 host twins of the library are compared with the restatement on the
same float32 coefficients; the follower logic, the mix arithmetic, the refusals and the mirror module's signatures are checked
exactly."""
import ast
import os

import numpy as np
import pytest
from scipy.signal import lfilter

import effects_reference as R

# 3 x the worst relative RMS error of a float32 host twin against the float64 restatement on the same float32 coefficients,
# measured on the CPU over every case of test_host_twins_vs_restatement (worst: 3.36e-6, the 48 kHz -6 dB high shelf; the
# shelves' poles sit closest to the unit circle at that rate; everything else is below 3.1e-7; LABNOTES 17).  The project's
# budget is 1e-3.
HOST_TWIN_BAR = 1.0e-5
assert HOST_TWIN_BAR <= 1e-3

REFERENCE = "/root/reference/rvc/scripts/audio_processing.py"


def _lib():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def _clip(n, sr, seed=3):
    """the GPU tests' signal shape: a synthetic voice at +-0.5 with exact zeros in the middle"""
    L = _lib()
    from polgen_rvc_amd import synthetic as S
    x = S.make_clip(seed, n / sr + 0.01, sr)[:n].astype(np.float64)
    x *= 0.5 / np.abs(x).max()
    x[n // 2:n // 2 + sr // 5] = 0.0
    return x.astype(np.float32)


def _peak_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


# ---- the restatement on lfilter ---------------------------------------------------------------------------------------------
def test_restatement_highpass_and_shelves_vs_lfilter():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(6000)
    for sr in (8000, 48000):
        cases = [R.highpass_coeffs(sr)] + [R.shelf_coeffs(sr, g, high) for g in (6.0, -6.0) for high in (False, True)]
        for c in cases:
            want = lfilter(c[:3], [1.0, c[3], c[4]], x)
            assert _peak_err(R.biquad(x, c), want) < 1e-12
    # the high-pass is the stated first-order recurrence
    c = R.highpass_coeffs(48000)
    y, xp, yp = np.empty(64), 0.0, 0.0
    for i in range(64):
        yp = c[0] * x[i] + c[1] * xp - c[3] * yp
        xp = x[i]
        y[i] = yp
    assert _peak_err(R.biquad(x[:64], c), y) < 1e-12


def test_restatement_comb_and_allpass_vs_lfilter():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(500)
    D, fb, d = 7, 0.84, 0.2
    b = np.zeros(D + 2)
    b[D], b[D + 1] = 1.0, -d                      # z^-D (1 - d z^-1)
    a = np.zeros(D + 1)
    a[0], a[1] = 1.0, -d
    a[D] -= fb * (1.0 - d)                        # (1 - d z^-1) - fb (1 - d) z^-D
    assert _peak_err(R.comb(x, D, fb, d), lfilter(b, a, x)) < 1e-12
    D = 5
    b, a = np.zeros(D + 1), np.zeros(D + 1)
    b[0], b[D], a[0], a[D] = -1.0, 1.5, 1.0, -0.5
    assert _peak_err(R.allpass(x, D), lfilter(b, a, x)) < 1e-12


def test_coefficients_are_the_definition_rounded_once():
    L = _lib()
    for sr in (8000, 44100, 48000, 192000):
        assert np.array_equal(L.fx_coeffs(0, sr, 50.0), R.highpass_coeffs(sr).astype(np.float32))
        for g in (6.0, -6.0, 3.5):
            for high in (False, True):
                got = L.fx_coeffs(2 if high else 1, sr, 440.0, 2.0 ** -0.5, g)
                want = R.shelf_coeffs(sr, g, high)
                assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()     # libm's last bit, then one rounding
        for ms in (0.0, 1.0, 10.0, 50.0, 100.0, 5000.0):
            assert abs(float(L.fx_cte(ms, sr)) - R.cte(ms, sr)) <= 2.0 ** -24
        for D in R.COMB + R.ALLPASS:
            assert L.fx_delay(sr, D + 23) == R.delay(sr, D + 23)
    assert L.fx_cte(0.0, 48000) == 0.0 and L.fx_cte(9e-4, 48000) == 0.0
    assert [L.fx_delay(8000, D) for D in (1116, 1617 + 23)] == [202, 297]


# ---- the host twins ------------------------------------------------------------------------------------------------------------
def test_host_twins_vs_restatement():
    L = _lib()
    worst = {}
    for sr, n in ((8000, 16000), (48000, 24000)):
        x = _clip(n, sr)
        c = L.fx_coeffs(0, sr, 50.0)
        worst[f"highpass {sr}"] = R.rel_rms(L.fx_highpass_host(x, sr), R.biquad(x, c.astype(np.float64)))
        for g in (6.0, -6.0):
            for high in (False, True):
                c = L.fx_coeffs(2 if high else 1, sr, 440.0, 2.0 ** -0.5, g)
                worst[f"shelf {sr} {g} {high}"] = R.rel_rms(L.fx_biquad_host(x, c), R.biquad(x, c.astype(np.float64)))
        ca, cr = float(L.fx_cte(1.0, sr)), float(L.fx_cte(100.0, sr))
        worst[f"follower {sr}"] = R.rel_rms(L.fx_follower_host(x, ca, cr), R.follower(x, ca, cr))
        c0, c50 = float(L.fx_cte(0.0, sr)), float(L.fx_cte(50.0, sr))
        worst[f"follower sq {sr}"] = R.rel_rms(L.fx_follower_host(x, c0, c50, square=True, sqrt_out=True),
                                               R.follower(x, c0, c50, square=True, sqrt_out=True))
        y, _ = L.fx_compressor_host(x, sr, 4.0, -12.0)
        worst[f"compressor {sr}"] = R.rel_rms(y, R.compressor(x, sr, 4.0, -12.0, c=(ca, cr))[0])
        c10 = float(L.fx_cte(10.0, sr))
        y, _ = L.fx_gate_host(x, sr, -40.0, 8.0, 10.0, 100.0)
        worst[f"gate {sr}"] = R.rel_rms(y, R.gate(x, sr, -40.0, 8.0, 10.0, 100.0, c=(c0, c50, c10, cr))[0])
        fb, d = R.f32v(0.28 * 0.1 + 0.7), R.f32v(0.4 * 0.9)
        D = L.fx_delay(sr, 1116)
        worst[f"comb {sr}"] = R.rel_rms(L.fx_comb_host(0.03 * x, D, fb, d), R.comb(0.03 * x.astype(np.float64), D, fb, d))
        D = L.fx_delay(sr, 225)
        worst[f"allpass {sr}"] = R.rel_rms(L.fx_allpass_host(x, D), R.allpass(x, D))
        for fbk in (0.0, 0.5):
            worst[f"chorus {sr} {fbk}"] = R.rel_rms(L.fx_chorus_host(x, sr, 1.5, R.f32v(0.25), 7.0, fbk, 0.5),
                                                    R.chorus(x, sr, 1.5, R.f32v(0.25), 7.0, fbk, 0.5))
    for k, v in worst.items():
        print(f"host twin {k}: {v:.3e}")
    bad = {k: v for k, v in worst.items() if not v <= HOST_TWIN_BAR}
    assert not bad, bad


# ---- follower logic, exactly ---------------------------------------------------------------------------------------------------
def test_follower_attack_release_exact():
    L = _lib()
    ca, cr = np.float32(0.25), np.float32(0.75)
    up = L.fx_follower_host(np.array([0, 0, 1, 1], np.float32), ca, cr)
    e1 = np.float32(1) - ca                               # 1 + ca (0 - 1): the attack constant
    e2 = np.float32(1) + ca * (e1 - np.float32(1))
    assert up.tolist() == [0.0, 0.0, float(e1), float(e2)]
    down = L.fx_follower_host(np.array([1, 0, 0], np.float32), np.float32(0), cr)
    assert down.tolist() == [1.0, float(cr), float(cr * cr)]           # attack 0 jumps, then e = cr e: the release constant
    sq = L.fx_follower_host(np.array([0.5, 0], np.float32), np.float32(0), cr, square=True, sqrt_out=True)
    assert sq.tolist() == [0.5, float(np.sqrt(np.float32(0.25) * cr))]


def test_ratio_one_is_the_identity_and_silence_stays_silent():
    L = _lib()
    x = _clip(4000, 8000)
    for y, _ in (L.fx_compressor_host(x, 8000, 1.0, -12.0), L.fx_gate_host(x, 8000, -40.0, 1.0, 10.0, 100.0)):
        assert y.tobytes() == x.tobytes()
    z = np.zeros(3000, np.float32)
    y, e = L.fx_gate_host(z, 8000, -40.0, 8.0, 10.0, 100.0)
    assert y.tobytes() == z.tobytes() and not np.isnan(e).any() and not np.any(e)
    tail = np.concatenate([0.5 * np.ones(100, np.float32), z])           # a closing gate ends in exact, finite zeros
    y, e = L.fx_gate_host(tail, 8000, -40.0, 8.0, 0.0, 1.0)
    assert np.isfinite(y).all() and np.isfinite(e).all() and not np.any(y[2000:])
    y, e = L.fx_compressor_host(z, 8000, 4.0, -12.0)
    assert y.tobytes() == z.tobytes() and not np.any(e)


# ---- mix -----------------------------------------------------------------------------------------------------------------------
def test_mix_arithmetic():
    L = _lib()
    st = lambda *v: np.array([[a, a] for a in v], np.int16)          # noqa: E731
    assert L.fx_mix_host(st(20000), st(0), 6.0, 0.0).tolist() == [[32767, 32767]]          # 39905 saturates
    assert L.fx_mix_host(st(-20000), st(0), 6.0, 0.0).tolist() == [[-32768, -32768]]
    assert L.fx_mix_host(st(-3, 3), st(0, 0), -6.0, 0.0)[:, 0].tolist() == [-2, 1]         # floor, not truncation
    assert L.fx_mix_host(st(30000, -30000), st(30000, -30000), 0.0, 0.0)[:, 0].tolist() == [32767, -32768]
    v = st(1, 2, 3, 4)
    assert L.fx_mix_host(v, st(10, 20, 30, 40, 50, 60), 0.0, 0.0)[:, 1].tolist() == [11, 22, 33, 44]    # longer: cut
    assert L.fx_mix_host(v, st(10), 0.0, 0.0)[:, 0].tolist() == [11, 2, 3, 4]                            # shorter: zeros
    assert L.fx_mix_host(v, np.zeros((0, 2), np.int16), 0.0, 0.0).tolist() == v.tolist()
    rng = np.random.default_rng(5)
    a, b = (rng.integers(-32768, 32768, (777, 2)).astype(np.int16) for _ in range(2))
    for gv, gi in ((0.0, 0.0), (3.0, -4.0), (-10.0, 10.0)):
        assert np.array_equal(L.fx_mix_host(a, b[:500], gv, gi), R.mix(a, b[:500], gv, gi))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_parameters_change_nothing():
    L = _lib()
    x = _clip(512, 8000)
    mark = np.full(512, 123.25, np.float32)
    calls = [
        lambda o: L.fx_compressor_host(x, 8000, 0.5, -12.0, out=o),                 # ratio < 1
        lambda o: L.fx_gate_host(x, 8000, -40.0, 0.99, 10.0, 100.0, out=o),
        lambda o: L.fx_compressor_host(x, 22050, 4.0, -12.0, out=o),                # not a multiple of 100 Hz
        lambda o: L.fx_highpass_host(x, 7900, out=o),                               # below 8000
        lambda o: L.fx_highpass_host(x, 192100, out=o),
        lambda o: L.fx_chorus_host(x, 8000, 1.0, 0.25, 7.0, 1.0, 0.5, out=o),       # |feedback| >= 1
        lambda o: L.fx_chorus_host(x, 8000, 1.0, 0.25, 7.0, -1.5, 0.5, out=o),
        lambda o: L.fx_gate_host(x, 8000, float("nan"), 8.0, 10.0, 100.0, out=o),
        lambda o: L.fx_follower_host(x, 1.0, 0.5, out=o),                           # a constant outside [0, 1)
    ]
    for k, call in enumerate(calls):
        out = mark.copy()
        with pytest.raises(L.RvcxError):
            call(out)
        assert out.tobytes() == mark.tobytes(), k
    with pytest.raises(L.RvcxError):
        L.fx_coeffs(1, 44150, 440.0)
    with pytest.raises(L.RvcxError):
        L.FxParams.make([0.0] * 17, 48000)
    assert L.fx_chunk() >= 64 and L.fx_chunk() % 4 == 0


# ---- the mirror module ---------------------------------------------------------------------------------------------------------
def _positional(fn_node):
    return [a.arg for a in fn_node.args.posonlyargs + fn_node.args.args]


def test_mirror_signatures_match_the_reference():
    if not os.path.exists(REFERENCE):
        pytest.skip("the reference tree is not on this machine")
    import inspect
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    tree = ast.parse(open(REFERENCE, encoding="utf-8").read())
    ref = {n.name: _positional(n) for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name in ("convert_to_stereo", "add_effects", "combine_audio", "process_audio"):
        got = [p.name for p in inspect.signature(getattr(M, name)).parameters.values()
               if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        assert got == ref[name], name
    assert inspect.signature(M.process_audio).parameters["progress"].default is None
    assert list(_lib().FX_FIELDS) == ref["add_effects"][2:]
    assert hasattr(M, "process_audio_many")


def test_mirror_refuses_before_any_work(tmp_path):
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.scripts import audio_processing as M
    args = ["v.wav", "i.wav"] + [0.0] * 18 + ["wav", 0, 0, False]
    for k, word in ((0, "вокалом"), (1, "инструменталом")):
        bad = list(args)
        bad[k] = ""
        with pytest.raises(ValueError, match=word):
            M.process_audio(*bad)
        with pytest.raises(ValueError, match=word):
            M.process_audio_many([bad])
    bad = list(args)
    bad[20] = "mp3"
    with pytest.raises(ValueError, match="no encoder"):
        M.process_audio(*bad)
    with pytest.raises(ValueError, match="no encoder"):
        M.combine_audio("v.wav", "i.wav", str(tmp_path / "o.mp3"), 0, 0, "mp3")
