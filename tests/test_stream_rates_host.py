"""CPU: the host side of live streams at the sound card's rate -- the delay of a session's resampler as the library defines it
(rvcx_stream_resample_delay, no GPU), the proof on the numpy oracle alone that this delay is the right one (every sample a step
emits has all its taps inside the input received so far; one sample less and it has not), and the rate checks of
VC.stream_open that need no device."""
import math

import numpy as np
import pytest

DELAYS = [((48000, 16000), 96), ((44100, 16000), 96), ((8000, 16000), 192), ((40000, 48000), 116), ((32000, 48000), 144),
          ((48000, 44100), 96), ((40000, 44100), 106), ((4800, 6000), 120), ((4800, 3200), 96)]


def _delay(sr_in, sr_out):
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib.stream_resample_delay(sr_in, sr_out)


def test_resample_delay_is_the_definition():
    for (a, b), want in DELAYS:
        assert _delay(a, b) == want, (a, b)
        assert want == math.ceil(96 * max(1.0, b / a) - 1e-9)
    for r in (16000, 44100, 48000, 4800, 8000, 192000):
        assert _delay(r, r) == 0
    for bad in (22050, 7900, 11025, 0, -16000, 192100, 48050):
        for other in (16000, 48000):
            assert _delay(bad, other) == -1 and _delay(other, bad) == -1, (bad, other)


def _steps_hold(x, sr_in, sr_out, Fb, K, d):
    """for every step k: the samples it emits, computed from the input received so far, are those of the whole signal (x is
    longer than K blocks, so the last step is no exception)"""
    from oracle.audio import resample_kaiser_hq
    b_in, b_out = Fb * sr_in // 100, Fb * sr_out // 100
    assert x.shape[0] > K * b_in
    whole = resample_kaiser_hq(x, sr_in, sr_out)
    ok = []
    for k in range(K):
        part = resample_kaiser_hq(x[:(k + 1) * b_in], sr_in, sr_out)
        lo, hi = max(k * b_out - d, 0), (k + 1) * b_out - d
        if hi <= lo:
            ok.append(True)
            continue
        assert hi <= part.shape[0]
        ok.append(bool(np.array_equal(part[lo:hi], whole[lo:hi])))
    return ok


def test_the_delay_is_right_and_one_less_is_not():
    """44100 -> 16000, blocks of 3 frames.  With d = 96 every step holds.  In exact arithmetic the last tap of the right wing
    of sample (k + 1) B - 96 sits AT the window's end (264.6 input samples = 96 crossings) and d = 95 would do; in double its
    table position lands below the end for some t, the tap is taken (with the table's zero-end weight, 1e-12) and reaches one
    sample past the input received.  That happens first at step 13 of these blocks (measured: steps 0 .. 12 hold with 95), so
    the negative control runs 21 steps; the first 7 are the case the definition was checked on."""
    g = np.random.default_rng(5)
    x = g.standard_normal(3 * 441 * 21 + 3000)
    d = _delay(44100, 16000)
    assert d == 96
    assert all(_steps_hold(x, 44100, 16000, 3, 7, d))
    assert all(_steps_hold(x, 44100, 16000, 3, 21, d))
    less = _steps_hold(x, 44100, 16000, 3, 21, d - 1)
    print("steps that fail with d - 1:", [k for k, ok in enumerate(less) if not ok])
    assert not all(less)


@pytest.mark.parametrize("rates,Fb,K", [((48000, 16000), 3, 7), ((4800, 6000), 1, 9), ((4800, 3200), 1, 9), ((4800, 6000), 6, 4)])
def test_the_delay_holds_for_other_pairs(rates, Fb, K):
    g = np.random.default_rng(6)
    x = g.standard_normal(Fb * rates[0] // 100 * K + 500)
    assert all(_steps_hold(x, rates[0], rates[1], Fb, K, _delay(*rates)))


def test_stream_open_refuses_rates_before_the_library_is_called():
    from polgen_rvc_amd.infer import infer as I, pipeline as P

    class Net:
        input_dim, ctx, model_id = 768, object(), 0

    class Hub:
        ctx = object()
    vc = P.VC(48000, I.Config())
    geo = dict(block_ms=100, context_ms=2500, crossfade_ms=50, search_ms=10)
    args = (Hub(), Net(), [0], [0.0], "rmvpe", "", 0.0, "v2", 0.33)
    for bad in (dict(input_sr=22050), dict(input_sr=11025), dict(output_sr=44150), dict(output_sr=0), dict(input_sr=16000.5)):
        with pytest.raises(ValueError, match="multiple of 100 Hz"):
            vc.stream_open(*args, **geo, **bad)
    with pytest.raises(ValueError, match="input_channels"):
        vc.stream_open(*args, **geo, input_channels=0)
    # valid rates get as far as the next check (the two stand-in models live on different contexts)
    with pytest.raises(ValueError, match="different rvcx contexts"):
        vc.stream_open(*args, **geo, input_sr=44100, input_channels=2, output_sr=48000)
