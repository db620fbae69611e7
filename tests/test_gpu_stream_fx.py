"""GPU: the effects board inside live sessions (include/rvcx.h "live post-production").  Op level (rvcx_op_stream_fx, no model):
partition independence, every stage against its anchor on the whole signal in every bit, composition, the float64 restatement,
what a caller could do before (the one-shot board block by block), identities and refusals.  Session level (the reduced models
and geometry of tests/test_gpu_stream_rates.py): a session with effects is the board on a plain session's output, in groups,
after a reset, through a repeated step and under set_effects.

Shapes: sr = 8000, 60 frames = 4800 samples (four multiples of rvcx_fx_chunk(), many comb / all-pass / chorus blocks), S = 3
rows, blocks of 1 (80 samples: shorter than every comb delay), 3, 12 and 60 frames; one run at 48 kHz, 9600 samples in blocks of
5 frames.  The signal is synthetic.make_clip at +-0.5 with exact zeros in the middle.

Bars.  Anchors, partitions, composition, sessions: bit for bit.  Against float64 (check 4): 3 x the relative RMS measured on
the GPU at the first run (LABNOTES 18) -- 8 kHz: 2.16e-6, 48 kHz: 4.29e-5 -- under the condition <= 1e-3, the project's budget.
Negative control (check 5): the one-shot board block by block (12 frames) misses the float64 chain by 3.5e+5 x the live
result's distance (measured: 0.756 against 2.16e-6; the bar of 100 x stands).

The high-pass has no identity setting (stage 1 is never skipped), so "the identity setting" of checks 6 and 11 leaves the
high-pass alone standing: with stage 1 masked out the board returns the stereo duplicate of its input, and with it the board
returns what stage 1 alone returns -- both bit for bit."""
import ctypes as C

import numpy as np
import pytest

import effects_reference as R
import test_gpu_stream_rates as T

pytestmark = pytest.mark.gpu

SR, FRAMES, S = 8000, 60, 3
N = FRAMES * SR // 100
BARS = {8000: 3 * 2.161e-6, 48000: 3 * 4.285e-5}
assert all(v <= 1e-3 for v in BARS.values())
NEGATIVE_FACTOR = 100.0

CHORUS = dict(chorus_rate_hz=1.5, chorus_depth=0.25, chorus_centre_delay_ms=7.0, chorus_feedback=0.5, chorus_mix=0.5)
FULL = dict(low_shelf_gain=6.0, high_shelf_gain=-6.0, **CHORUS)
REVERBS = [dict(), dict(reverb_rm_size=0.8, reverb_damping=0.3, reverb_wet=0.33, reverb_dry=0.0, reverb_width=0.5)]
IDENTITY = dict(compressor_ratio=1.0, noise_gate_ratio=1.0, low_shelf_gain=0.0, high_shelf_gain=0.0, chorus_mix=0.0,
                reverb_wet=0.0, reverb_dry=0.5)
FC, FX, FS, FB = T.FC, T.FX, T.FS, T.FB


def _L():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    return _lib


def _signal(n, sr, seed):
    """(n, 2) float32, L != R: the shape of tests/test_gpu_effects.py::_signal, the zeros at every length"""
    from polgen_rvc_amd import synthetic as Sy
    ch = []
    for k in range(2):
        x = Sy.make_clip(seed + 7 * k, n / sr + 0.01, sr)[:n].astype(np.float64)
        x *= 0.5 / max(np.abs(x).max(), 1e-9)
        x[n // 2:n // 2 + min(sr // 5, n // 4)] = 0.0
        ch.append(x)
    return np.ascontiguousarray(np.stack(ch, axis=1), dtype=np.float32)


@pytest.fixture(scope="module")
def stereo():
    return np.ascontiguousarray(np.stack([_signal(N, SR, 40 + 3 * s) for s in range(S)]))      # (S, N, 2)


@pytest.fixture(scope="module")
def mono(stereo):
    return np.ascontiguousarray(stereo[:, :, 0])                                               # (S, N)


def _dup(x):
    return np.ascontiguousarray(np.stack([x, x], axis=-1))


def _f64(values):
    return {k: R.f32v(v) for k, v in _L().fx_values(values).items()}


@pytest.fixture(scope="module")
def live_full(ctx, mono):
    """the whole board on the base case in blocks of 3 frames: computed once, shared, never written"""
    y = ctx.stream_fx(mono, SR, 3, FULL)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------------------------------------------------ op level
def test_partition_independence(ctx, mono, live_full):
    assert live_full.shape == (S, N, 2) and np.isfinite(live_full).all() and np.abs(live_full).max() > 0.05
    assert not np.array_equal(live_full[..., 0], live_full[..., 1])            # the reverb's sides differ
    for fb in (1, 12, 60):
        assert np.array_equal(ctx.stream_fx(mono, SR, fb, FULL), live_full), fb
    for s in range(S):
        assert np.array_equal(ctx.stream_fx(mono[s:s + 1], SR, 12, FULL)[0], live_full[s]), s
    assert np.array_equal(ctx.stream_fx(_dup(mono), SR, 3, FULL), live_full)
    assert not np.array_equal(live_full[0], live_full[1])


def test_each_stage_alone_equals_its_anchor(ctx, mono, stereo):
    L = _L()
    q = 2.0 ** -0.5
    # per-channel stages: mono rows (L = R leaves) and one stereo run with L != R
    def rows(y, x, anchor, what):
        for s in range(x.shape[0]):
            for c in range(2):
                v = x[s] if x.ndim == 2 else x[s, :, c]
                assert np.array_equal(y[s, :, c], anchor(np.ascontiguousarray(v))), (what, s, c)

    y = ctx.stream_fx(mono, SR, 3, {}, stages=[1])
    rows(y, mono, lambda v: L.fx_highpass_host(v, SR), "highpass")
    lo, hi = L.fx_coeffs(1, SR, 440.0, q, 6.0), L.fx_coeffs(2, SR, 440.0, q, -6.0)
    rows(ctx.stream_fx(mono, SR, 3, FULL, stages=[5]), mono, lambda v: L.fx_biquad_host(v, lo), "low shelf")
    rows(ctx.stream_fx(mono, SR, 3, FULL, stages=[6]), mono, lambda v: L.fx_biquad_host(v, hi), "high shelf")
    rows(ctx.stream_fx(stereo, SR, 3, FULL, stages=[6]), stereo, lambda v: L.fx_biquad_host(v, hi), "high shelf stereo")
    rows(ctx.stream_fx(mono, SR, 3, {}, stages=[2]), mono, lambda v: ctx.fx_compressor(v, SR, 4.0, -12.0), "compressor")
    rows(ctx.stream_fx(mono, SR, 3, {}, stages=[3]), mono, lambda v: ctx.fx_gate(v, SR, -40.0, 8.0, 10.0, 100.0), "gate")
    rows(ctx.stream_fx(stereo, SR, 3, {}, stages=[3]), stereo, lambda v: ctx.fx_gate(v, SR, -40.0, 8.0, 10.0, 100.0),
         "gate stereo")
    for fbk in (0.5, 0.0):
        p = dict(CHORUS, chorus_feedback=fbk)
        anchor = lambda v: ctx.fx_chorus(v, SR, 1.5, 0.25, 7.0, fbk, 0.5)     # noqa: E731
        rows(ctx.stream_fx(mono, SR, 3, p, stages=[7]), mono, anchor, f"chorus {fbk}")
        rows(ctx.stream_fx(stereo[:1], SR, 3, p, stages=[7]), stereo[:1], anchor, f"chorus {fbk} stereo")
    # the reverb: stereo in, stereo out, at both settings, from L = R and from L != R
    for k, rv in enumerate(REVERBS):
        v = L.fx_values(rv)
        args = [v[n] for n in ("reverb_rm_size", "reverb_damping", "reverb_wet", "reverb_dry", "reverb_width")]
        for x in (_dup(mono), stereo):
            y = ctx.stream_fx(x, SR, 3, rv, stages=[4])
            for s in range(S):
                assert np.array_equal(y[s], L.fx_reverb_host(x[s], SR, *args)), (k, s)
    assert np.array_equal(ctx.stream_fx(mono, SR, 3, {}, stages=[4]), ctx.stream_fx(_dup(mono), SR, 3, {}, stages=[4]))


def test_the_board_is_its_stages_composed(ctx, mono, live_full):
    y = mono
    for k in range(1, 8):
        y = ctx.stream_fx(y, SR, 3, FULL, stages=[k])
    assert np.array_equal(y, live_full)


@pytest.mark.parametrize("sr,frames,fb", [(8000, FRAMES, 3), (48000, 20, 5)])
def test_against_float64(ctx, sr, frames, fb, mono, live_full):
    if sr == SR:
        x, got = mono[:1], live_full[:1]
    else:
        x = np.ascontiguousarray(_signal(frames * sr // 100, sr, 51)[None, :, 0])
        got = ctx.stream_fx(x, sr, fb, FULL)
    err = R.rel_rms(got[0], R.chain(_dup(x[0]), sr, _f64(FULL)))
    print(f"live board vs float64 at {sr} Hz: rel rms {err:.3e} (bar {BARS[sr]:.3e})")
    assert err <= BARS[sr]


def test_negative_control_the_one_shot_board_block_by_block(ctx, mono, live_full):
    """what a caller can do today: rvcx_fx_chain per block of 12 frames restarts every filter, envelope and delay line"""
    L = _L()
    x = _dup(mono[0])
    p = L.FxParams.make(L.fx_values(FULL), SR, 2)
    blk = 12 * SR // 100
    cut = np.concatenate(ctx.fx_chain([x[j:j + blk] for j in range(0, N, blk)], p))
    want = R.chain(x, SR, _f64(FULL))
    far, near = R.rel_rms(cut, want), R.rel_rms(live_full[0], want)
    print(f"one-shot board block by block vs float64: {far:.3e}; the live board: {near:.3e}; ratio {far / near:.3g}")
    assert not np.array_equal(cut, live_full[0])
    assert far >= NEGATIVE_FACTOR * near


def test_identity(ctx, mono, stereo):
    L = _L()
    assert np.float32(2.0) * np.float32(L.fx_values(IDENTITY)["reverb_dry"]) == np.float32(1.0)
    assert np.array_equal(ctx.stream_fx(mono, SR, 3, IDENTITY, stages=range(2, 8)), _dup(mono))
    assert np.array_equal(ctx.stream_fx(stereo, SR, 3, IDENTITY, stages=range(2, 8)), stereo)
    assert np.array_equal(ctx.stream_fx(mono, SR, 3, IDENTITY), ctx.stream_fx(mono, SR, 3, {}, stages=[1]))


def test_op_refusals_write_nothing(ctx, mono):
    L = _L()
    lib = L.lib()
    x = np.ascontiguousarray(mono[:1])
    mark = np.full((1, N, 2), 123.25, np.float32)

    def call(sr, fb, frames=N, **over):
        out = mark.copy()
        p = L.FxParams.make(L.fx_values(over), 0, 0)
        rc = lib.rvcx_op_stream_fx(ctx._h, x.ctypes.data, 1, C.c_int64(frames), 1, sr, fb, C.byref(p), 0x7F, out.ctypes.data)
        return rc, out

    cases = [dict(sr=22050, fb=3), dict(sr=3100, fb=3), dict(sr=SR, fb=7), dict(sr=SR, fb=3, compressor_ratio=0.5),
             dict(sr=SR, fb=3, noise_gate_ratio=0.99), dict(sr=SR, fb=3, chorus_feedback=1.0),
             dict(sr=SR, fb=3, chorus_feedback=-1.5), dict(sr=SR, fb=3, reverb_wet=float("nan")),
             dict(sr=SR, fb=3, low_shelf_gain=float("inf"))]
    for k, case in enumerate(cases):
        rc, out = call(**case)
        assert rc == -1 and out.tobytes() == mark.tobytes(), k
        assert (lib.rvcx_last_error(ctx._h) or b"").decode()
    with pytest.raises(L.RvcxError, match="multiple of 100 Hz"):
        ctx.stream_fx(x, 22050, 3, {})
    with pytest.raises(L.RvcxError, match="multiple of the block"):
        ctx.stream_fx(x, SR, 7, {})
    rc, out = call(SR, 3)
    assert rc == 0 and np.isfinite(out).all() and out.tobytes() != mark.tobytes()
    # 3200 .. 7900 Hz are open to the op: the reduced voice models' rates
    assert np.isfinite(ctx.stream_fx(np.ascontiguousarray(x[:, :4800]), 4800, 5, FULL)).all()


# ------------------------------------------------------------------------------------------------------------ sessions
@pytest.fixture(scope="module")
def voice(ctx):
    from polgen_rvc_amd import synthetic as Sy
    E = T._load_front(ctx, 6)
    mid = T._load_synth(ctx, Sy.SYNTH_CFG_TINY, 6, input_dim=E)
    yield mid
    ctx.unload_synth(mid)


def _blocks(seed, steps, n_streams):
    return T._mic(seed, steps, n_streams, rate=16000, channels=1)[..., 0]              # (steps, S, FB * 160)


def _run(ctx, mid, mic, seed=5, sids=(2,), pitches=(3.0,), taps=False, inject_at=None, **kw):
    """-> (list of step results, the session's last taps per step when asked)"""
    outs, native = [], []
    with ctx.stream_open(mid, T._params(seed=seed), list(sids), list(pitches), FB, FC, FX, FS, **kw) as se:
        for k in range(len(mic)):
            if k == inject_at:
                n0 = ctx.gru_fallbacks()
                ctx.debug_inject(1)            # the software flag: the step's body runs twice (BiGRU fallback)
            outs.append(se.step(mic[k], taps=taps))
            if k == inject_at:
                assert ctx.gru_fallbacks() == n0 + 1
            if se.out_resampled:
                native.append(se.last_taps()[1])
        shape = (se.out_channels, se.block_out, se.out_rate)
    return outs, native, shape


@pytest.mark.parametrize("out_rate", [0, 6000])
def test_a_session_with_effects_is_the_board_on_a_plain_session(ctx, voice, out_rate):
    mic = _blocks(61, 8, 1)
    sr = out_rate or 4800
    fx, _, shape = _run(ctx, voice, mic, taps=True, out_rate=out_rate, effects=FULL)
    plain, _, pshape = _run(ctx, voice, mic, taps=True, out_rate=out_rate)
    assert shape == (2, FB * sr // 100, sr) and pshape == (1, FB * sr // 100, sr)
    assert fx[0][0].shape == (1, FB * sr // 100, 2) and plain[0][0].shape == (1, FB * sr // 100)
    for k in range(8):
        assert np.array_equal(fx[k][1], plain[k][1]) and np.array_equal(fx[k][2], plain[k][2]), k     # pre_sola, offsets
    whole = T._whole([o[0] for o in plain])
    got = T._whole([o[0] for o in fx])
    assert np.abs(whole).max() > 1e-3 and np.isfinite(got).all()
    if out_rate:
        assert not whole[:, :120].any() and not got[:, :120].any()            # the delay's zeros enter the board
    assert np.array_equal(got, ctx.stream_fx(whole, sr, FB, FULL))
    assert not np.array_equal(got[..., 0], whole)


def test_group_alone_and_reset(ctx, voice):
    sids, pitches, seed, steps = [0, 3, 1], [0.0, 3.5, -2.0], 21, 8
    mic = _blocks(62, steps, 3)
    with ctx.stream_open(voice, T._params(seed=seed), sids, pitches, FB, FC, FX, FS, out_rate=6000, effects=FULL) as grp:
        first = [grp.step(mic[k]) for k in range(steps)]
        grp.reset()
        again = [grp.step(mic[k]) for k in range(steps)]
    assert all(o.shape == (3, FB * 60, 2) and np.isfinite(o).all() for o in first) and np.abs(first[-1]).max() > 1e-3
    for k in range(steps):
        assert np.array_equal(first[k], again[k]), k
    for s in range(3):
        one, _, _ = _run(ctx, voice, mic[:, s:s + 1], seed=seed + s, sids=sids[s:s + 1], pitches=pitches[s:s + 1],
                         out_rate=6000, effects=FULL)
        for k in range(steps):
            assert np.array_equal(one[k][0], first[k][s]), (s, k)
    assert not np.array_equal(first[-1][0], first[-1][1])


def test_a_repeated_step_leaves_the_board_where_it_was(ctx, voice):
    """step 2 of 8 runs twice (rvcx_debug_inject 1, as tests/test_gpu_stream_rates.py does): the board read the state set the
    first attempt did not write, so the session is still the board on its own output in front of the board -- here the output
    resampler's, rebuilt from the native taps"""
    mic = _blocks(63, 8, 1)
    fx, native, _ = _run(ctx, voice, mic, out_rate=6000, effects=FULL, inject_at=2)
    before = ctx.stream_resample(T._whole(native), 4800, 6000, FB)
    assert np.abs(before).max() > 1e-3
    assert np.array_equal(T._whole(fx), ctx.stream_fx(before, 6000, FB, FULL))


def test_set_effects(ctx, voice):
    L = _L()
    mic = _blocks(64, 8, 1)
    base, _, _ = _run(ctx, voice, mic, effects=FULL)
    plain, _, _ = _run(ctx, voice, mic)
    whole = T._whole(plain)
    k_switch = 4
    got = []
    with ctx.stream_open(voice, T._params(), [2], [3.0], FB, FC, FX, FS, effects=FULL) as se:
        assert se.effects["chorus_mix"] == 0.5 and se.effects["compressor_ratio"] == 4.0
        for k in range(8):
            if k == 2:
                se.set_effects(**FULL)                                   # unchanged values change no bit
                se.set_effects()
            if k == 3:
                for bad in (dict(compressor_ratio=0.5), dict(chorus_feedback=1.0), dict(reverb_wet=float("nan"))):
                    with pytest.raises(L.RvcxError):
                        se.set_effects(reverb_dry=0.1, **bad)            # refused: nothing changes, reverb_dry included
                with pytest.raises(L.RvcxError, match="unknown name"):
                    se.set_effects(reverb_size=1.0)
                assert se.effects["reverb_dry"] == 0.8
            if k == k_switch:
                se.set_effects(**IDENTITY)
            got.append(se.step(mic[k]))
        ms = se.last_fx_ms()
    assert list(ms) == ["highpass", "compressor", "gate", "reverb", "low_shelf", "high_shelf", "chorus", "total"]
    assert ms["total"] > 0.0 and ms["reverb"] > 0.0 and ms["compressor"] >= 0.0
    for k in range(k_switch):
        assert np.array_equal(got[k], base[k]), k
    # from the switch on only the high-pass still acts, from the state it has carried since sample 0 (see the header)
    B = FB * 48
    hp = ctx.stream_fx(whole, 4800, FB, {}, stages=[1])
    for k in range(k_switch, 8):
        assert np.array_equal(got[k], hp[:, k * B:(k + 1) * B]), k
        assert not np.array_equal(got[k], base[k]), k
    with ctx.stream_open(voice, T._params(), [2], [3.0], FB, FC, FX, FS) as se:
        with pytest.raises(L.RvcxError, match="without effects"):
            se.set_effects(reverb_wet=0.2)
        with pytest.raises(L.RvcxError):
            se.last_fx_ms()
        assert se.out_channels == 1


def test_a_session_opened_without_effects_is_todays(ctx, voice):
    """rvcx_stream_open_fx with fx == NULL against rvcx_stream_open_io: (S, block_out), the same bits"""
    L = _L()
    mic = _blocks(65, 8, 1)
    want, _, shape = _run(ctx, voice, mic, taps=True, effects=None)
    assert shape[0] == 1 and want[0][0].shape == (1, FB * 48)
    sid, pit = np.asarray([2], np.int32), np.asarray([3.0], np.float32)
    cfg, io, p, h = L.StreamCfg(1, FB, FC, FX, FS), L.StreamIO(0, 1, 0, 0), T._params(), C.c_int(0)
    ctx._ck(L.lib().rvcx_stream_open_fx(ctx._h, int(voice), C.byref(cfg), C.byref(io), None, C.byref(p), sid.ctypes.data,
                                        pit.ctypes.data, C.byref(h)), "stream_open_fx")
    with L.StreamSession(ctx, int(h.value), cfg, io, ctx.synth_upp(voice)) as se:
        assert se.out_channels == 1
        for k in range(8):
            for a, b in zip(se.step(mic[k], taps=True), want[k]):
                assert np.array_equal(a, b), k
    # a refused board opens nothing
    bad = L.FxParams.make(L.fx_values(dict(compressor_ratio=0.5)), 0, 0)
    assert L.lib().rvcx_stream_open_fx(ctx._h, int(voice), C.byref(cfg), C.byref(io), C.byref(bad), C.byref(p),
                                       sid.ctypes.data, pit.ctypes.data, C.byref(h)) == -1
    for sr_field, ch_field in ((44100, 0), (0, 1)):
        bad = L.FxParams.make(L.fx_values({}), sr_field, ch_field)
        assert L.lib().rvcx_stream_open_fx(ctx._h, int(voice), C.byref(cfg), C.byref(io), C.byref(bad), C.byref(p),
                                           sid.ctypes.data, pit.ctypes.data, C.byref(h)) == -1
