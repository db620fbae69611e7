"""The rvcx_get_f0*_x entry points and the F0 stage of a live-stream step all go through one routine (get_f0_device,
csrc/pipeline.hip).  Entry points that state the same request must return the same bits; the frame-count rules of each
back-end (rmvpe un-truncated, fcpe resized to p_len) and the per-stream pitch of a session must survive.

Bars: bit equality everywhere -- both sides of every comparison run the same kernels on the same input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SIG = 16000 + 37                    # F = 1 + n // 160 = 101 frames, and n // 160 = 100 is not F
FRAMES = 1 + N_SIG // 160
FC, FX, FS, FB = 20, 2, 1, 6          # the ring of test_gpu_stream.py: N = 29 frames, T = 28


def _params(f0_method=0, pitch=0.0, seed=5, x_pad=1):
    from polgen_rvc_amd import _lib
    p = _lib.Params(pitch, 50.0, 1100.0, 0.0, 0.33, 1.0, 0, x_pad, 1, 2, 3, seed)
    p.f0_method = f0_method
    return p


@pytest.fixture(scope="module")
def front(ctx):
    """tiny HuBERT, RMVPE and FCPE, and one signal shared by the tests (never written to).  The synthetic RMVPE's output bias
    (-11.5) keeps its salience below the 0.03 voicing threshold nearly everywhere, and an unvoiced track ignores the pitch
    shift: the bias is raised by 9 here, so that frames are voiced and the pitch enters what is compared."""
    from polgen_rvc_amd import synthetic as S, weights as W
    hcfg, rcfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, 12))
    rs = dict(S.rmvpe_state(rcfg, 12))
    rs["fc.1.bias"] = (rs["fc.1.bias"] + np.float32(9.0)).astype(np.float32)
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), rs)
    sd = S.fcpe_state(S.FCPE_CFG_TINY, 12)
    ctx.load_fcpe(W.fcpe_cfg_struct(W.fcpe_cfg_from_state(sd)), sd)
    x = S.make_clip(90, N_SIG / 16000.0 + 0.01).astype(np.float32)[:N_SIG]
    assert x.shape[0] == N_SIG
    x.setflags(write=False)
    return hcfg["embed_dim"], x


def test_rmvpe_x_equals_x_ex_and_f0_file(ctx, front):
    """rvcx_get_f0_x is rvcx_get_f0_x_ex without a file: the same 101 frames, bit for bit, with a pitch shift in the params.
    An f0 file of two rows at 0.03 s and 0.07 s makes a track of int16(round(0.04 * 100 + 1)) = 5 frames, which VC.get_f0
    writes from frame x_pad * 100 on (pipeline.py:186-191): with x_pad = 0 that is frames 0 - 4.  Inside that span the result
    is the file's (and differs from the model's), outside it nothing moves."""
    _, x = front
    p = _params(pitch=2.0, x_pad=0)
    c0, f0 = ctx.get_f0_x(x, p)
    c1, f1 = ctx.get_f0_x_ex(x, N_SIG // 160, p)
    assert c0.shape == f0.shape == (FRAMES,) and c1.shape == f1.shape == (FRAMES,)
    assert np.array_equal(c0, c1) and np.array_equal(f0, f1)
    assert np.isfinite(f0).all() and c0.min() >= 1 and c0.max() <= 255
    assert (f0 > 0).sum() >= FRAMES // 4                         # voiced: the pitch shift is in these numbers
    tab = np.array([[0.03, 431.5], [0.07, 470.25]], np.float32)
    c2, f2 = ctx.get_f0_x_ex(x, N_SIG // 160, p, inp_f0=tab)
    assert c2.shape == (FRAMES,)
    span = slice(0, 5)
    want = np.interp(np.arange(5), tab[:, 0] * 100, tab[:, 1]).astype(np.float32)
    print("f0 file span:", f2[span], "model:", f1[span])
    assert np.array_equal(f2[span], want)
    assert (f2[span] != f1[span]).all() and (c2[span] != c1[span]).any()
    assert np.array_equal(f2[5:], f1[5:]) and np.array_equal(c2[5:], c1[5:])


@pytest.mark.parametrize("extra", [-1, 3])
def test_fcpe_x_equals_x_ex(ctx, front, extra):
    """p_len = F - 1 is VC.pipeline's own case, p_len = F + 3 makes compute_f0 stretch the track"""
    from polgen_rvc_amd import _lib
    _, x = front
    p = _params(f0_method=_lib.F0_FCPE, pitch=-1.5)
    p_len = FRAMES + extra
    c0, f0 = ctx.get_f0_fcpe_x(x, p_len, p)
    c1, f1 = ctx.get_f0_x_ex(x, p_len, p)
    assert c0.shape == f0.shape == c1.shape == f1.shape == (p_len,)
    assert np.array_equal(c0, c1) and np.array_equal(f0, f1)
    assert np.isfinite(f0).all() and c0.min() >= 1 and c0.max() <= 255


def test_fcpe_p_len_zero_raises(ctx, front):
    from polgen_rvc_amd import _lib
    _, x = front
    p = _params(f0_method=_lib.F0_FCPE)
    with pytest.raises(_lib.RvcxError):
        ctx.get_f0_fcpe_x(x, 0, p)
    with pytest.raises(_lib.RvcxError):
        ctx.get_f0_x_ex(x, 0, p)
    assert ctx.get_f0_fcpe_x(x, FRAMES - 1, p)[0].shape == (FRAMES - 1,)      # the context is usable after the refusals


def test_stream_pitch_per_stream(ctx, front):
    """A step's F0 does not leave the library, so the per-stream pitch is pinned the way test_gpu_stream.py pins groups: five
    steps of S = 2 streams with pitches (0, +3.5) from a zeroed ring (the fifth fills it) equal, bit for bit, each stream
    stepped alone with its own pitch.  Controls: rvcx_get_f0_x_ex on the last ring rebuilt on the host gives voiced frames
    and different tracks for the two pitches, and the same blocks stepped with pitch 0 on stream 1's speaker and noise
    differ from stream 1's audio -- so a build that dropped the per-stream pitch would fail here.  The ring is
    test_gpu_stream.py's (29 frames): the shortest ring stream_open takes has a single HuBERT frame, a geometry none of the
    models' kernels is run at anywhere."""
    from polgen_rvc_amd import synthetic as S, weights as W
    E, x = front
    cfg = S.SYNTH_CFG_TINY
    mid = ctx.load_synth(W.synth_cfg_struct(cfg, E), S.synth_state(cfg, 12, input_dim=E))
    steps, N = 5, FC + FX + FS + FB
    sig = np.ascontiguousarray(x[4000:4000 + steps * FB * 160])
    blocks = np.stack([sig.reshape(steps, FB * 160)] * 2, axis=1)          # (steps, 2, block): both streams hear the same
    sids, pitches, seed = [1, 1], [0.0, 3.5], 9
    try:
        with ctx.stream_open(mid, _params(seed=seed), sids, pitches, FB, FC, FX, FS) as grp:
            got = [grp.step(blocks[k]) for k in range(steps)]
            T = grp.frames
        assert all(o.shape == (2, grp.block_out) and np.isfinite(o).all() for o in got)
        for s in range(2):
            with ctx.stream_open(mid, _params(seed=seed + s), sids[s:s + 1], pitches[s:s + 1], FB, FC, FX, FS) as one:
                for k in range(steps):
                    assert np.array_equal(one.step(blocks[k, s:s + 1])[0], got[k][s]), (s, k)
        ring = np.ascontiguousarray(sig[-N * 160:])
        tracks = [ctx.get_f0_x_ex(ring, N, _params(pitch=v)) for v in pitches]
        voiced = int((tracks[0][1][:T] > 0).sum())
        moved = int((tracks[0][0][:T] != tracks[1][0][:T]).sum())
        print(f"ring of {N} frames: {voiced} of {T} frames voiced, the pitch moves coarse in {moved}")
        assert voiced >= 1 and moved >= 1
        with ctx.stream_open(mid, _params(seed=seed + 1), [1], [0.0], FB, FC, FX, FS) as flat:
            last = [flat.step(blocks[k, :1])[0] for k in range(steps)][-1]
        assert not np.array_equal(last, got[-1][1])
    finally:
        ctx.unload_synth(mid)
