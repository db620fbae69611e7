"""CPU: the refusals that the post-production ABI files share (csrc/api_fx_common.h) -- null pointer, sample rate, channel
count, frame count and a value that is not finite -- on one host twin of each file, message for message.  The texts are what
rvcx_last_error has always shown for these calls; a caller may match on them, so they are compared whole."""
import ctypes as C

import numpy as np

SR, N = 8000, 600
NAN = float("nan")


def _cases(L):
    lib = L.lib()
    x, y = np.zeros(2 * N, np.float32), np.zeros(2 * N, np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data

    def chorus(x=xp, sr=SR, rate=1.0):                                                        # api_fx.hip (one channel, n >= 0)
        return lib.rvcx_fx_chorus_host(x, N, sr, rate, 0.25, 7.0, 0.0, 0.5, yp)

    def limit(x=xp, n=N, ch=1, sr=SR, ceiling=-1.0):                                          # api_loudness.hip (n >= 0)
        return lib.rvcx_fx_limit_host(x, n, ch, sr, ceiling, 2.0, 100.0, yp, None)

    def pitch(x=xp, n=N, ch=1, sr=SR, semitones=2.0):                                         # api_pitch.hip
        return lib.rvcx_fx_pitch_shift_host(x, n, ch, sr, semitones, yp, None, None, None, None)

    def denoise(x=xp, n=N, ch=1, sr=SR, **kw):                                                # api_denoise.hip
        p = L.FxDenoiseParams.make(sr, ch, **dict(dict(mode=1), **kw))
        return lib.rvcx_fx_denoise_host(x, n, None, 0, C.byref(p), yp, None, None, None, None, None, None)

    def formant(x=xp, n=N, ch=1, sr=SR, **kw):                                                # api_formant.hip
        p = L.FxFormantParams.make(sr, ch, **dict(dict(ratio=1.5), **kw))
        return lib.rvcx_fx_formant_host(x, n, None, C.byref(p), yp, None, None, None, None, None)

    def live(n=N, sr=SR, **kw):                                                               # api_stream_denoise.hip (mono)
        p = L.LiveDenoiseParams.make(0, **dict(dict(mode=1), **kw))
        return lib.rvcx_fx_denoise_live_host(xp, n, sr, None, 0, C.byref(p), yp, None, None, None, None)

    rate = "the sample rate must be a multiple of 100 Hz within 8000 .. 192000"
    return [
        (lambda: chorus(x=None), "fx_chorus_host: null pointer"),
        (lambda: chorus(sr=7000), "fx_chorus_host: " + rate),
        (lambda: chorus(rate=NAN), "fx_chorus_host: rate_hz is not finite"),
        (lambda: limit(x=None), "fx_limit_host: null pointer"),
        (lambda: limit(sr=192100), "fx_limit_host: " + rate),
        (lambda: limit(ch=3), "fx_limit_host: channels must be 1 or 2"),
        (lambda: limit(ceiling=NAN), "fx_limit_host: a value is not finite"),
        (lambda: pitch(x=None), "fx_pitch_shift_host: null pointer"),
        (lambda: pitch(sr=8050), "fx_pitch_shift_host: " + rate),
        (lambda: pitch(ch=3), "fx_pitch_shift_host: channels must be 1 or 2"),
        (lambda: pitch(n=0), "fx_pitch_shift_host: 1 .. 2^30 frames are required"),
        (lambda: pitch(semitones=NAN), "fx_pitch_shift_host: a value is not finite"),
        (lambda: denoise(x=None), "fx_denoise_host: null pointer"),
        (lambda: denoise(sr=7900), "fx_denoise_host: " + rate),
        (lambda: denoise(ch=3), "fx_denoise_host: channels must be 1 or 2"),
        (lambda: denoise(n=0), "fx_denoise_host: every item needs 1 .. 2^30 frames"),
        (lambda: denoise(knee_db=NAN), "fx_denoise_host: a value is not finite"),
        (lambda: denoise(strength=1.5), "fx_denoise_host: strength must lie in 0.000000 .. 1.000000"),
        (lambda: formant(x=None), "fx_formant_host: null pointer"),
        (lambda: formant(sr=7000), "fx_formant_host: " + rate),
        (lambda: formant(ch=3), "fx_formant_host: channels must be 1 or 2"),
        (lambda: formant(n=0), "fx_formant_host: every item needs 1 .. 2^30 frames"),
        (lambda: formant(amount=NAN), "fx_formant_host: a value is not finite"),
        (lambda: live(sr=3100), "fx_denoise_live_host: the sample rate must be a multiple of 100 Hz within 3200 .. 192000"),
        (lambda: live(n=0), "fx_denoise_live_host: 1 .. 2^30 samples are required"),
    ]


def test_refusals_name_their_caller():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib as L
    cases = _cases(L)
    for call, text in cases:
        assert call() == -1, text
        assert (L.lib().rvcx_last_error(None) or b"").decode() == text
    assert len(cases) == 25
