"""CPU: the host side of live post-production (include/rvcx.h "live post-production").  rvcx_fx_reverb_host -- the sequential
float32 reverb a live session's reverb equals bit for bit -- against the float64 restatement (tests/effects_reference.py), its
refusals, and the mirror's `effects=` argument.

Bar: tests/test_effects_host.py's bar for host twins, 1.0e-5 relative RMS.  Measured on the CPU (LABNOTES 18): 8 kHz defaults
3.69e-8, 8 kHz second setting 1.75e-7, 48 kHz defaults 3.60e-8, 48 kHz second setting 1.48e-7."""
import numpy as np
import pytest

import effects_reference as R

HOST_TWIN_BAR = 1.0e-5                     # tests/test_effects_host.py
assert HOST_TWIN_BAR <= 1e-3

REVERBS = {"defaults": (0.1, 0.9, 0.1, 0.8, 1.0), "second": (0.8, 0.3, 0.33, 0.0, 0.5)}    # room, damping, wet, dry, width


def _lib():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def _signal(n, sr, seed):
    """the shape of tests/test_gpu_effects.py::_signal: synthetic.make_clip at +-0.5, exact zeros in the middle"""
    from polgen_rvc_amd import synthetic as S
    ch = []
    for k in range(2):
        x = S.make_clip(seed + 7 * k, n / sr + 0.01, sr)[:n].astype(np.float64)
        x *= 0.5 / max(np.abs(x).max(), 1e-9)
        x[n // 2:n // 2 + sr // 5] = 0.0
        ch.append(x)
    return np.ascontiguousarray(np.stack(ch, axis=1), dtype=np.float32)


@pytest.mark.parametrize("sr,n", [(8000, 8000), (48000, 24000)])
@pytest.mark.parametrize("name", sorted(REVERBS))
def test_reverb_host_vs_float64(sr, n, name):
    L = _lib()
    x = _signal(n, sr, 31)
    args = [R.f32v(v) for v in REVERBS[name]]
    got = L.fx_reverb_host(x, sr, *args)
    assert got.shape == x.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = R.rel_rms(got, R.reverb(x, sr, *args))
    print(f"reverb host twin {sr} {name}: rel rms {err:.3e}")
    assert err <= HOST_TWIN_BAR


def test_reverb_host_is_its_pieces():
    """the twin is fx_comb_host / fx_allpass_host and the mix FMAs: the wet part alone at width 1 (w2 = 0) is w1 times the
    all-passed comb sum of a side"""
    L = _lib()
    sr = 8000
    x = _signal(2000, sr, 5)
    room, damping, wet = R.f32v(0.1), R.f32v(0.9), R.f32v(0.1)
    got = L.fx_reverb_host(x, sr, room, damping, wet, 0.0, 1.0)
    inp = (np.float32(0.015) * (x[:, 0] + x[:, 1])).astype(np.float32)
    fb, d = np.float32(0.28 * room + 0.7), np.float32(0.4 * damping)
    w1 = np.float32(1.5 * wet * 2.0)
    for side in range(2):
        acc = L.fx_comb_host(inp, L.fx_delay(sr, R.COMB[0] + 23 * side), fb, d)
        for D in R.COMB[1:]:
            acc = acc + L.fx_comb_host(inp, L.fx_delay(sr, D + 23 * side), fb, d)
        for D in R.ALLPASS:
            acc = L.fx_allpass_host(acc, L.fx_delay(sr, D + 23 * side))
        assert np.array_equal(got[:, side], acc * w1)


def test_reverb_host_refusals_write_nothing():
    L = _lib()
    x = _signal(4000, 8000, 2)[:512]
    mark = np.full((512, 2), 123.25, np.float32)
    nan = float("nan")
    lib = L.lib()

    def call(n, sr, *args):
        out = mark.copy()
        rc = lib.rvcx_fx_reverb_host(x.ctypes.data, n, sr, *args, out.ctypes.data)
        return rc, out

    for k, (n, sr, args) in enumerate([(512, 8000, (nan, 0.9, 0.1, 0.8, 1.0)), (512, 8000, (0.1, nan, 0.1, 0.8, 1.0)),
                                       (512, 8000, (0.1, 0.9, float("inf"), 0.8, 1.0)), (512, 8000, (0.1, 0.9, 0.1, nan, 1.0)),
                                       (512, 8000, (0.1, 0.9, 0.1, 0.8, nan)), (-1, 8000, (0.1, 0.9, 0.1, 0.8, 1.0)),
                                       (512, 22050, (0.1, 0.9, 0.1, 0.8, 1.0))]):
        rc, out = call(n, sr, *args)
        assert rc == -1 and out.tobytes() == mark.tobytes(), k
        assert lib.rvcx_last_error(None)
    rc, out = call(512, 8000, 0.1, 0.9, 0.1, 0.8, 1.0)
    assert rc == 0 and out.tobytes() != mark.tobytes()
    rc, out = call(0, 8000, 0.1, 0.9, 0.1, 0.8, 1.0)             # nothing to do is no error
    assert rc == 0 and out.tobytes() == mark.tobytes()
    with pytest.raises(L.RvcxError, match="stereo"):
        L.fx_reverb_host(x[:, 0], 8000, 0.1, 0.9, 0.1, 0.8, 1.0)


def test_effect_values_are_laid_over_the_ui_defaults():
    L = _lib()
    v = L.fx_values(dict(chorus_mix=0.5, low_shelf_gain=6))
    assert list(v) == list(L.FX_UI_DEFAULTS) and set(v) == set(L.FX_FIELDS)
    assert v["chorus_mix"] == 0.5 and v["low_shelf_gain"] == 6.0 and v["compressor_ratio"] == 4.0
    assert L.fx_values(dict(reverb_wet=0.3), base=v)["chorus_mix"] == 0.5
    p = L.FxParams.make(v, 48000, 2)
    assert L.fx_values(p) == {k: float(np.float32(x)) for k, x in v.items()}
    with pytest.raises(L.RvcxError, match="unknown name"):
        L.fx_values(dict(reverb_size=0.3))


def test_mirror_stream_open_takes_effects_and_refuses_unknown_names_first():
    import inspect
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    from polgen_rvc_amd.infer.pipeline import VC
    for fn in (VC.stream_open, _lib.Context.stream_open):
        assert inspect.signature(fn).parameters["effects"].default is None
    vc = VC.__new__(VC)                    # no model, no context: the refusal comes before any of them is touched
    with pytest.raises(ValueError, match="unknown name"):
        vc.stream_open(None, None, [0], [0.0], "nonsense-method", "", 0.0, "v2", 0.33, block_ms=60, context_ms=200,
                       crossfade_ms=20, search_ms=10, effects=dict(reverb_room=0.5))
    # a known name passes that check and reaches the next one
    with pytest.raises(Exception) as e:
        vc.stream_open(None, None, [0], [0.0], "nonsense-method", "", 0.0, "v2", 0.33, block_ms=60, context_ms=200,
                       crossfade_ms=20, search_ms=10, effects=dict(reverb_rm_size=0.5))
    assert "unknown name" not in str(e.value)
