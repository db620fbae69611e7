"""Live streams at the sound card's rate on the GPU: the session's stateful resampler without a session
(rvcx_op_stream_resample) against the one-shot filter, and rate sessions (rvcx_stream_open_io) against the composition of
their parts, in groups, after a reset, under live controls and through a repeated step.

Bars.  Partition independence, composition, groups, reset, controls: bit for bit.  Against the float64 numpy oracle:
2^-23 |ref| + 1e-9 (one float32 rounding of a double sum that is exact to 1e-12).  Against the one-shot device kernel
rounded to float32: one float32 ulp (the tap loop is shared, the sum is double); the count of samples that differ at all is
printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FC, FX, FS = 20, 2, 1
FB = 6


def _load_synth(ctx, cfg, seed, input_dim=768):
    from polgen_rvc_amd import synthetic as S, weights as W
    return ctx.load_synth(W.synth_cfg_struct(cfg, input_dim), S.synth_state(cfg, seed, input_dim=input_dim))


def _load_front(ctx, seed):
    from polgen_rvc_amd import synthetic as S, weights as W
    hcfg, rcfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, seed))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, seed))
    return hcfg["embed_dim"]


def _params(index_rate=0.0, protect=0.33, seed=5, pitch=0.0):
    from polgen_rvc_amd import _lib
    p = _lib.Params(pitch, 50.0, 1100.0, index_rate, protect, 1.0, 0, 1, 1, 2, 3, seed)
    p.f0_method = 0
    return p


def _mic(seed, steps, S, fb=FB, rate=44100, channels=2):
    """(steps, S, fb * rate / 100, channels) float32: a voiced tone plus noise, different per stream and channel"""
    g = np.random.default_rng(seed)
    n = steps * fb * rate // 100
    t = np.arange(n) / rate
    x = np.empty((S, n, channels), np.float32)
    for s in range(S):
        tone = 0.3 * np.sin(2 * np.pi * (140.0 + 35.0 * s) * t * (1.0 + 0.1 * np.sin(2 * np.pi * 1.5 * t)))
        for c in range(channels):
            x[s, :, c] = tone * (1.0 - 0.2 * c) + 0.05 * g.standard_normal(n)
    return np.ascontiguousarray(x.reshape(S, steps, -1, channels).transpose(1, 0, 2, 3))


def _whole(blocks):
    """(steps, S, n[, c]) -> (S, steps * n[, c])"""
    return np.ascontiguousarray(np.concatenate(list(blocks), axis=1))


# ---------------------------------------------------------------------------------------------- op level
OP_CASES = [(44100, 16000, 2, 3, (1, 3, 10)), (4800, 6000, 1, 3, (1, 6)), (4800, 3200, 1, 3, (1, 6))]


@pytest.mark.parametrize("sr_in,sr_out,ch,S,fbs", OP_CASES)
def test_partition_independence(ctx, sr_in, sr_out, ch, S, fbs):
    """0.30 s of noise: the result does not depend on the block (a block of 60 / 32 output samples is shorter than the delay
    and than a wing), and row s of a group is that row alone"""
    g = np.random.default_rng(sr_in + sr_out)
    frames = 30 * sr_in // 100
    x = g.standard_normal((S, frames, ch) if ch > 1 else (S, frames)).astype(np.float32)
    ys = [ctx.stream_resample(x, sr_in, sr_out, fb) for fb in fbs]
    assert ys[0].shape == (S, 30 * sr_out // 100) and np.isfinite(ys[0]).all() and ys[0].any()
    for fb, y in zip(fbs[1:], ys[1:]):
        assert np.array_equal(y, ys[0]), fb
    for s in range(S):
        for fb in fbs:
            assert np.array_equal(ctx.stream_resample(x[s:s + 1], sr_in, sr_out, fb)[0], ys[0][s]), (s, fb)


@pytest.mark.parametrize("sr_in,sr_out,ch", [(44100, 16000, 2), (48000, 16000, 1), (4800, 6000, 1), (4800, 3200, 1)])
def test_it_is_the_one_shot_filter_delayed(ctx, sr_in, sr_out, ch):
    from polgen_rvc_amd import _lib
    from oracle.audio import resample_kaiser_hq, to_mono
    g = np.random.default_rng(sr_in + 7 * sr_out)
    S, fb = 2, 3
    frames = 30 * sr_in // 100
    x = g.standard_normal((S, frames, ch) if ch > 1 else (S, frames)).astype(np.float32)
    d = _lib.stream_resample_delay(sr_in, sr_out)
    y = ctx.stream_resample(x, sr_in, sr_out, fb)
    n_out = y.shape[1]
    assert n_out == 30 * sr_out // 100 and d < n_out
    assert not y[:, :d].any()
    blk_in, blk_out = 10 * sr_in // 100, 10 * sr_out // 100
    for s in range(S):
        x64 = x[s].astype(np.float64)
        got = y[s, d:]
        # (a) the float64 numpy oracle on the double of the input
        ref = resample_kaiser_hq(to_mono(x64), sr_in, sr_out)[:n_out - d]
        err = np.abs(got.astype(np.float64) - ref)
        bar = 2.0 ** -23 * np.abs(ref) + 1e-9
        print(f"{sr_in}->{sr_out} x{ch} row {s}: vs float64 oracle max err / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
        # (b) the one-shot device kernel on the same input as float64, rounded to float32
        one = ctx.resample(x64, sr_in, sr_out, kind=0)
        one32 = one.astype(np.float32)[:n_out - d]
        ulp = np.spacing(np.abs(one32))
        diff = np.abs(got.astype(np.float64) - one32.astype(np.float64))
        print(f"{sr_in}->{sr_out} x{ch} row {s}: {int((got != one32).sum())} of {got.size} samples differ from the one-shot "
              f"kernel, worst {float((diff / ulp).max()):.2f} ulp")
        assert (diff <= ulp).all()
        # (c) negative control: what a caller can do today, the one-shot resampler block by block (100 ms)
        cut = np.concatenate([ctx.resample(x64[k * blk_in:(k + 1) * blk_in], sr_in, sr_out, kind=0) for k in range(3)])
        assert cut.shape[0] == 3 * blk_out
        miss = np.abs(cut - one[:3 * blk_out]) / np.spacing(np.abs(one[:3 * blk_out]).astype(np.float32))
        edge = float(max(miss[blk_out - 4:blk_out + 4].max(), miss[2 * blk_out - 4:2 * blk_out + 4].max()))
        print(f"{sr_in}->{sr_out} x{ch} row {s}: block-by-block one-shot misses by {edge:.3g} float32 ulp at the block edges")
        assert edge > 100.0


def test_op_refusals(ctx):
    from polgen_rvc_amd._lib import RvcxError
    x = np.zeros((1, 441 * 6), np.float32)
    for a, b in ((22050, 16000), (44100, 11025), (44150, 16000), (7900, 16000)):
        with pytest.raises(RvcxError, match="multiple of 100 Hz"):
            ctx.stream_resample(np.zeros((1, a * 6 // 100), np.float32), a, b, 2)
    with pytest.raises(RvcxError, match="channels >= 1"):
        ctx.stream_resample(np.zeros((1, 441 * 6, 0), np.float32), 44100, 16000, 2)
    with pytest.raises(RvcxError, match="multiple of the block"):
        ctx.stream_resample(x, 44100, 16000, 4)
    assert ctx.stream_resample(x, 44100, 16000, 3).shape == (1, 960)


# ---------------------------------------------------------------------------------------------- sessions
def _open_the_old_way(ctx, mid, params, sids, pitches, *frames):
    """rvcx_stream_open itself (Context.stream_open goes through rvcx_stream_open_io)"""
    import ctypes as C
    from polgen_rvc_amd import _lib
    sid, pit = np.asarray(sids, np.int32), np.asarray(pitches, np.float32)
    cfg = _lib.StreamCfg(len(sid), *frames)
    h = C.c_int(0)
    ctx._ck(_lib.lib().rvcx_stream_open(ctx._h, int(mid), C.byref(cfg), C.byref(params), sid.ctypes.data_as(C.c_void_p),
                                        pit.ctypes.data_as(C.c_void_p), C.byref(h)), "stream_open")
    return _lib.StreamSession(ctx, int(h.value), cfg, _lib.StreamIO(0, 1, 0, 0), ctx.synth_upp(mid))


def test_todays_path_is_untouched(ctx):
    """io {0, 1, 0} and {16000, 1, the model's rate} are rvcx_stream_open bit for bit: 5 steps, parity noise, every tap"""
    from polgen_rvc_amd import synthetic as S
    E = _load_front(ctx, 6)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 6, input_dim=E)
    upp = ctx.synth_upp(mid)
    blocks = _mic(3, 5, 1, rate=16000, channels=1)[..., 0]
    try:
        runs = []
        for io in (None, dict(in_rate=0, in_channels=1, out_rate=0), dict(in_rate=16000, in_channels=1, out_rate=100 * upp)):
            with (_open_the_old_way(ctx, mid, _params(), [2], [3.0], FB, FC, FX, FS) if io is None else
                  ctx.stream_open(mid, _params(), [2], [3.0], FB, FC, FX, FS, **io)) as se:
                assert se.in_delay == 0 and se.out_delay == 0 and se.latency_ms == 10.0
                assert se.block_in == FB * 160 and se.block_out == FB * 48 and se.upp == 48 and not se.out_resampled
                assert se.tail_len == (FB + FX + FS) * 48 and se.skip_head == se.frames - (FB + FX + FS)
                g = np.random.default_rng(11)
                got = []
                for k in range(5):
                    got.append(se.step(blocks[k], noise=g.standard_normal((1, se.noise_len)).astype(np.float32), taps=True))
                in16k, native = se.last_taps()
                assert native is None and np.array_equal(in16k, blocks[4])
                runs.append(got)
        assert np.abs(runs[0][-1][0]).max() > 1e-3
        for other in runs[1:]:
            for k in range(5):
                for a, b in zip(runs[0][k], other[k]):
                    assert np.array_equal(a, b), k
    finally:
        ctx.unload_synth(mid)


def _run_rate_session(ctx, mid, fb, io, steps, seed, inject_at=None):
    """one S = 1 session with parity noise: (blocks, noises, outs, pre_solas, offsets, in16k taps, native taps)"""
    in_rate, ch = io.get("in_rate", 16000) or 16000, io.get("in_channels", 1)
    mic = _mic(seed, steps, 1, fb=fb, rate=in_rate, channels=ch)
    if ch == 1:
        mic = mic[..., 0]
    g = np.random.default_rng(seed + 1)
    rec = dict(mic=mic, noise=[], out=[], pre=[], offs=[], in16k=[], native=[])
    with ctx.stream_open(mid, _params(), [2], [3.0], fb, FC, FX, FS, **io) as se:
        rec["se"] = se
        for k in range(steps):
            nz = g.standard_normal((1, se.noise_len)).astype(np.float32)
            if k == inject_at:
                n0 = ctx.gru_fallbacks()
                ctx.debug_inject(1)            # the software flag: the step's body runs twice (BiGRU fallback)
            out, pre, offs = se.step(mic[k], noise=nz, taps=True)
            if k == inject_at:
                assert ctx.gru_fallbacks() == n0 + 1
            a, b = se.last_taps()
            for key, v in zip(("noise", "out", "pre", "offs", "in16k", "native"), (nz, out, pre, offs, a, b)):
                rec[key].append(v)
    return rec


def test_a_rate_session_is_the_composition_of_its_parts(ctx):
    """44100 Hz stereo in, 6000 Hz out of the 4800 Hz model, 8 steps: (i) the blocks that entered the ring are the op-level
    resampler on the whole input, (ii) a plain session fed with them gives the native blocks, (iii) the output is the
    op-level resampler on the concatenated native blocks.  (iii) again at 3200 Hz with blocks of one frame."""
    from polgen_rvc_amd import _lib, synthetic as S
    E = _load_front(ctx, 6)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 6, input_dim=E)
    try:
        R = _run_rate_session(ctx, mid, FB, dict(in_rate=44100, in_channels=2, out_rate=6000), 8, 21)
        se = R["se"]
        assert se.block_in == FB * 441 and se.block_out == FB * 60 and se.in_delay == 96 and se.out_delay == 120
        assert se.out_resampled and se.upp == 48 and se.tail_len == (FB + FX + FS) * 48
        assert abs(se.latency_ms - (6.0 + 20.0 + 10.0)) < 1e-9
        # (i)
        assert np.array_equal(_whole(R["in16k"]), ctx.stream_resample(_whole(R["mic"]), 44100, 16000, FB))
        assert np.abs(R["in16k"][-1]).max() > 1e-2
        # (ii)
        with ctx.stream_open(mid, _params(), [2], [3.0], FB, FC, FX, FS) as P:
            for k in range(8):
                out, pre, offs = P.step(R["in16k"][k], noise=R["noise"][k], taps=True)
                assert np.array_equal(out, R["native"][k]) and np.array_equal(pre, R["pre"][k]), k
                assert np.array_equal(offs, R["offs"][k]), k
        assert np.abs(R["native"][-1]).max() > 1e-3
        # (iii)
        assert np.array_equal(_whole(R["out"]), ctx.stream_resample(_whole(R["native"]), 4800, 6000, FB))
        assert not _whole(R["out"])[:, :120].any() and np.abs(_whole(R["out"])).max() > 1e-3
        # (iii) downwards, one frame per block, the input side untouched
        R2 = _run_rate_session(ctx, mid, 1, dict(out_rate=3200), 8, 22)
        assert R2["se"].block_in == 160 and R2["se"].block_out == 32 and R2["se"].out_delay == 96 and R2["se"].in_delay == 0
        assert np.array_equal(_whole(R2["in16k"]), _whole(R2["mic"]))
        assert np.array_equal(_whole(R2["out"]), ctx.stream_resample(_whole(R2["native"]), 4800, 3200, 1))
        assert _lib.stream_resample_delay(4800, 3200) == 96
    finally:
        ctx.unload_synth(mid)


def test_a_repeated_step_leaves_the_session_where_it_was(ctx):
    """step 2 of 5 runs twice (rvcx_debug_inject 1: the injected BiGRU time-out repeats the body on the plain GRU kernel): both
    FIFOs were read from the set the failed attempt did not write, so (i) and (iii) of the composition still hold over the
    whole session, and the 16 kHz blocks are those of a session without the repeat"""
    from polgen_rvc_amd import synthetic as S
    E = _load_front(ctx, 6)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 6, input_dim=E)
    io = dict(in_rate=44100, in_channels=2, out_rate=6000)
    try:
        R = _run_rate_session(ctx, mid, FB, io, 5, 23, inject_at=2)
        Q = _run_rate_session(ctx, mid, FB, io, 5, 23)
        assert np.array_equal(_whole(R["in16k"]), _whole(Q["in16k"]))
        assert np.array_equal(_whole(R["in16k"]), ctx.stream_resample(_whole(R["mic"]), 44100, 16000, FB))
        assert np.array_equal(_whole(R["out"]), ctx.stream_resample(_whole(R["native"]), 4800, 6000, FB))
        for k in (0, 1):
            assert np.array_equal(R["out"][k], Q["out"][k])
    finally:
        ctx.unload_synth(mid)


def test_group_equals_single_and_reset(ctx):
    """S = 3 rate session, one pitch and sid per stream, Philox noise: every stream equals the same stream alone in a session
    opened with seed + s; after reset() the same blocks give the bits of a fresh session"""
    from polgen_rvc_amd import synthetic as S
    E = _load_front(ctx, 7)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 7, input_dim=E)
    io = dict(in_rate=44100, in_channels=2, out_rate=6000)
    sids, pitches, seed, steps = [0, 3, 1], [0.0, 3.5, -2.0], 21, 4
    mic = _mic(31, steps, 3)
    try:
        with ctx.stream_open(mid, _params(seed=seed), sids, pitches, FB, FC, FX, FS, **io) as grp:
            first = [grp.step(mic[k]) for k in range(steps)]
            grp.reset()
            again = [grp.step(mic[k]) for k in range(steps)]
        assert all(o.shape == (3, FB * 60) and np.isfinite(o).all() for o in first) and np.abs(first[-1]).max() > 1e-3
        for k in range(steps):
            assert np.array_equal(first[k], again[k]), k
        for s in range(3):
            with ctx.stream_open(mid, _params(seed=seed + s), sids[s:s + 1], pitches[s:s + 1], FB, FC, FX, FS, **io) as one:
                for k in range(steps):
                    assert np.array_equal(one.step(mic[k, s:s + 1])[0], first[k][s]), (s, k)
        assert not np.array_equal(first[-1][0], first[-1][1])
    finally:
        ctx.unload_synth(mid)


def test_live_controls(ctx):
    """A: +0 / sid 0 / protect 0.33, three steps, set(+7, sid 3, protect 0.1), three more.  B: opened with +7 / 3 / 0.1.  Ring,
    FIFOs and noise counters are the same, so pre_sola (which does not see the carry) is B's from step 3 on."""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd._lib import RvcxError
    E = _load_front(ctx, 8)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 8, input_dim=E)
    io = dict(in_rate=44100, in_channels=2, out_rate=6000)
    mic = _mic(41, 7, 1)
    try:
        with ctx.stream_open(mid, _params(seed=9, protect=0.33), [0], [0.0], FB, FC, FX, FS, **io) as A, \
                ctx.stream_open(mid, _params(seed=9, protect=0.1), [3], [7.0], FB, FC, FX, FS, **io) as B:
            pa, pb = [], []
            for k in range(7):
                if k == 3:
                    A.set(pitches=[7.0], sids=[3], protect=0.1)
                if k == 6:
                    A.set()                                    # nothing given: nothing changes
                    with pytest.raises(RvcxError, match="speaker id"):
                        A.set(pitches=[-5.0], sids=[99], protect=0.5)
                pa.append(A.step(mic[k], taps=True)[1])
                pb.append(B.step(mic[k], taps=True)[1])
                assert np.array_equal(A.last_taps()[0], B.last_taps()[0])
        for k in range(7):
            same = np.array_equal(pa[k], pb[k])
            assert same == (k >= 3), k
        assert np.abs(pa[-1]).max() > 1e-3
    finally:
        ctx.unload_synth(mid)


def test_open_refuses_bad_rates(ctx):
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd._lib import RvcxError
    E = _load_front(ctx, 8)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 8, input_dim=E)
    try:
        for io in (dict(in_rate=22050), dict(in_rate=11025), dict(in_rate=7900), dict(out_rate=22050), dict(out_rate=48000),
                   dict(in_rate=192100)):
            with pytest.raises(RvcxError, match="multiple of 100 Hz"):
                ctx.stream_open(mid, _params(), [0], [0.0], FB, FC, FX, FS, **io)
        with pytest.raises(RvcxError, match="in_channels"):
            ctx.stream_open(mid, _params(), [0], [0.0], FB, FC, FX, FS, in_channels=0)
        # equal rates, two channels: the mono mix alone, no delay
        with ctx.stream_open(mid, _params(), [0], [0.0], FB, FC, FX, FS, in_rate=16000, in_channels=2) as se:
            x = _mic(5, 1, 1, rate=16000, channels=2)[0]
            se.step(x)
            want = ((x[..., 0].astype(np.float64) + x[..., 1].astype(np.float64)) / 2).astype(np.float32)
            assert se.in_delay == 0 and se.block_in == FB * 160 and np.array_equal(se.last_taps()[0], want)
    finally:
        ctx.unload_synth(mid)
