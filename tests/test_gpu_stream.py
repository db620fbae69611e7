"""Live streams on the GPU: Synthesizer.infer's `rate` as `skip_head` (rvcx_synth_infer_head) against the reference's own
goldens, SOLA on the device (rvcx_op_sola) against its float64 restatement, and sessions (rvcx_stream_*) against the
composition of the reference-pinned stage entry points, alone and in groups.

Bars.  1e-4 relative RMS / 1e-4 absolute: the bars of test_synth_vs_reference_golden.  1e-5 relative RMS: this suite's bar
for "same arithmetic, other launch shape".  Offsets: the rule of `_check_offset` (worst-case fp32 summation error)."""
import json
import os

import numpy as np
import pytest

from conftest import rms

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

FC, FX, FS, FB = 20, 2, 1, 6          # frames: N = 29 ring frames, T = 28, skip_head = 19
HEAD, T28 = 19, 28


def rel(a, b):
    return rms(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(rms(b), 1e-30)


def _load_synth(ctx, cfg, seed, input_dim=768):
    from polgen_rvc_amd import synthetic as S, weights as W
    return ctx.load_synth(W.synth_cfg_struct(cfg, input_dim), S.synth_state(cfg, seed, input_dim=input_dim))


def _load_front(ctx, seed, fcpe=False):
    from polgen_rvc_amd import synthetic as S, weights as W
    hcfg, rcfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, seed))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, seed))
    if fcpe:
        sd = S.fcpe_state(S.FCPE_CFG_TINY, seed)
        ctx.load_fcpe(W.fcpe_cfg_struct(W.fcpe_cfg_from_state(sd)), sd)
    return hcfg["embed_dim"]


def _params(index_rate=0.0, protect=0.33, seed=5, f0_method=0, pitch=0.0):
    from polgen_rvc_amd import _lib
    p = _lib.Params(pitch, 50.0, 1100.0, index_rate, protect, 1.0, 0, 1, 1, 2, 3, seed)
    p.f0_method = f0_method
    return p


def _blocks(index, n_blocks, S=1):
    from polgen_rvc_amd import synthetic as Sy
    out = np.empty((n_blocks, S, FB * 160), np.float32)
    for s in range(S):
        clip = Sy.make_clip(index + s, n_blocks * FB / 100.0 + 0.05).astype(np.float32)
        out[:, s] = clip[:n_blocks * FB * 160].reshape(n_blocks, FB * 160)
    return out


def _check_offset(y, b, Lb, Lx, Ls, got):
    """The GPU's offset must score, in float64, within tol of the float64 maximum, tol = 2 Lx 2^-24 max_d(sum|y b| / den): the
    worst-case forward error of any fp32 summation order of Lx terms, numerator and denominator together.  Where the float64
    runner-up is farther away than that, the offset must be the argmax itself."""
    from polgen_rvc_amd._lib import sola_reference
    _, _, d64, scores, mags = sola_reference(y, b, Lb, Lx, Ls)
    tol = 2.0 * Lx * 2.0 ** -24 * float(mags.max())
    assert 0 <= got <= Ls
    print(f"sola offset: gpu {got}, float64 {d64}, score gap {scores[d64] - scores[got]:.3e}, tol {tol:.3e}")
    assert scores[got] >= scores[d64] - tol, (got, d64, scores[got], scores[d64], tol)
    others = np.delete(scores, d64)
    if others.size == 0 or others.max() < scores[d64] - tol:
        assert got == d64, (got, d64)
    return d64


# ---------------------------------------------------------------------------------------------- 1. skip_head vs the reference
@pytest.mark.parametrize("tag", ["tiny_h30", "tiny_h27", "48k_h15"])
def test_skip_head_vs_reference_golden(ctx, tag):
    """Synthesizer.infer(..., rate) of the reference itself (tools/gen_golden.py, step synth_head).  Negative control: the tail
    of the FULL evaluation misses the golden by more than 100x the bar (0.2 - 0.4 relative for the reference on the CPU)."""
    d = np.load(os.path.join(GOLD, f"synth_head_{tag}.npz"))
    cfg = json.loads(str(d["cfg"]))
    mid = _load_synth(ctx, cfg, int(d["seed"]))
    head = int(d["head"])
    got, z = ctx.synth_infer(mid, d["phone"], d["pitch"], d["f0"], z_noise=d["z_noise"], src_noise=d["src_noise"][:, :, 0],
                             skip_head=head)
    ez = rel(z, d["z"])
    ref = d["audio"][:, 0]
    e = rms(got - ref)
    print(f"synth_head {tag}: head {head}, z rel err {ez:.3e}, audio rms_ref={rms(ref):.4f} rms_err={e:.3e}")
    assert z.shape == d["z"].shape and ez < 1e-4
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert e / rms(ref) < 1e-4 and e < 1e-4
    miss = rms(d["audio_full_tail"][:, 0] - ref) / rms(ref)
    print(f"synth_head {tag}: tail of the full evaluation misses by {miss:.3f} relative")
    assert miss > 100 * 1e-4
    ctx.unload_synth(mid)


# ---------------------------------------------------------------------------------------------- 2. skip_head, batches, errors
def test_skip_head_zero_batches_and_errors(ctx):
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd._lib import RvcxError
    from oracle import synth as O
    cfg = S.SYNTH_CFG_TINY
    mid = _load_synth(ctx, cfg, 3)
    c = O.cfg_fields(cfg)
    g = np.random.default_rng(2)
    B, T = 3, T28
    phone = g.standard_normal((B, T, 768)).astype(np.float32)
    pitch = g.integers(1, 256, (B, T)).astype(np.int32)
    f0 = (100 + 300 * g.random((B, T))).astype(np.float32)
    f0[:, 8:12] = 0
    f0[1, 20:25] = 0                       # an unvoiced stretch inside the tail of one item
    pitch[f0 == 0] = 1
    sid = np.array([0, 3, 1], np.int32)
    zn = g.standard_normal((B, c["inter"], T)).astype(np.float32)
    sn_full = g.standard_normal((B, T * c["upp"])).astype(np.float32)
    # skip_head = 0 is the plain call, bit for bit
    plain = ctx.synth_infer(mid, phone, pitch, f0, sid=sid, z_noise=zn, src_noise=sn_full)
    zero, _ = ctx.synth_infer(mid, phone, pitch, f0, sid=sid, z_noise=zn, src_noise=sn_full, skip_head=0)
    assert np.array_equal(plain, zero)
    # B = 3 with skip_head = 19 equals each item alone, bit for bit
    sn = np.ascontiguousarray(sn_full[:, HEAD * c["upp"]:])
    both, zb = ctx.synth_infer(mid, phone, pitch, f0, sid=sid, z_noise=zn, src_noise=sn, skip_head=HEAD)
    assert both.shape == (B, (T - HEAD) * c["upp"]) and np.isfinite(both).all()
    for i in range(B):
        one, z1 = ctx.synth_infer(mid, phone[i:i + 1], pitch[i:i + 1], f0[i:i + 1], sid=sid[i:i + 1], z_noise=zn[i:i + 1],
                                  src_noise=sn[i:i + 1], skip_head=HEAD)
        assert np.array_equal(one[0], both[i]) and np.array_equal(z1[0], zb[i]), i
    # the slice is not the tail of the whole (the flow and the source see the slice)
    assert rel(both, plain[:, HEAD * c["upp"]:]) > 1e-2
    # errors
    with pytest.raises(RvcxError, match="equal lengths"):
        ctx.synth_infer(mid, phone, pitch, f0, lens=[T, T - 3, T], sid=sid, z_noise=zn, src_noise=sn, skip_head=HEAD)
    with pytest.raises(RvcxError, match="exclude"):
        ctx.synth_infer(mid, phone, pitch, f0, sid=sid, z_noise=zn, src_noise=sn, skip_head=HEAD, dec_skip=2)
    for bad in (T, T + 5, -1):
        with pytest.raises(RvcxError, match="skip_head"):
            ctx.synth_infer(mid, phone, pitch, f0, sid=sid, z_noise=zn, skip_head=bad)
    ctx.unload_synth(mid)


# ---------------------------------------------------------------------------------------------- 3. SOLA
SOLA_SHAPES = [(48, 48, 96), (37, 5, 11), (2400, 480, 4800)]       # (Lx, Ls, Lb): tiny upp; nothing a multiple of 4 or 64; 48 k


@pytest.mark.parametrize("shape", SOLA_SHAPES)
def test_sola_vs_float64(ctx, shape):
    from polgen_rvc_amd._lib import sola_reference
    Lx, Ls, Lb = shape
    g = np.random.default_rng(Lx + Ls)
    b = g.standard_normal(Lx).astype(np.float32)
    # a scaled copy of the carry planted at offset 0, at Ls (the inclusive end) and in the middle: found exactly
    for d0 in (0, Ls, Ls // 2):
        y = g.standard_normal(Lb + Lx + Ls).astype(np.float32)
        y[d0:d0 + Lx] = 0.7 * b
        out, nb, off, sc = ctx.sola(y, b, Lb, Lx, Ls, scores=True)
        assert off == d0, (off, d0)
        _check_offset(y, b, Lb, Lx, Ls, off)
        ro, rb, _, rs, _ = sola_reference(y, b, Lb, Lx, Ls)
        eo, eb, es = rel(out, ro), rel(nb, rb), rel(sc, rs)
        print(f"sola {shape} plant {d0}: out {eo:.2e} carry {eb:.2e} scores {es:.2e}")
        assert eo < 1e-5 and eb < 1e-5 and es < 1e-5
    # noise without a plant: the general offset rule
    for k in range(3):
        y = g.standard_normal(Lb + Lx + Ls).astype(np.float32)
        out, nb, off = ctx.sola(y, b, Lb, Lx, Ls)
        _check_offset(y, b, Lb, Lx, Ls, off)
        ro, rb, _, _, _ = sola_reference(y, b, Lb, Lx, Ls, offset=off)
        assert rel(out, ro) < 1e-5 and rel(nb, rb) < 1e-5
    # silence ties exactly: the first index, finite output
    zeros = np.zeros(Lb + Lx + Ls, np.float32)
    for carry in (b, np.zeros(Lx, np.float32)):
        out, nb, off, sc = ctx.sola(zeros, carry, Lb, Lx, Ls, scores=True)
        assert off == 0 and np.isfinite(out).all() and np.isfinite(nb).all() and np.all(sc == 0.0)
        ro, rb, _, _, _ = sola_reference(zeros, carry, Lb, Lx, Ls)
        assert not nb.any() and np.abs(out - ro).max() <= 1e-6 * max(1.0, np.abs(ro).max())


# ---------------------------------------------------------------------------------------------- 4. session vs composition
def test_session_vs_composition(ctx):
    """S = 1, rmvpe+, a 6-row index at index_rate 0.5, protect 0.33, parity noise: every step against get_f0_x_ex +
    hubert_features + index_blend + x2 upsample / protect mix (numpy) + synth_infer(skip_head=19) on the ring rebuilt in
    numpy, and against the float64 SOLA with the GPU's offset and the previous step's carry."""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd._lib import sola_reference
    from oracle import synth as O
    E = _load_front(ctx, 6)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 6, input_dim=E)
    inter, upp = O.cfg_fields(S.SYNTH_CFG_TINY)["inter"], ctx.synth_upp(mid)
    Lb, Lx, Ls = FB * upp, FX * upp, FS * upp
    N = FC + FX + FS + FB
    ctx.load_index(S.make_index(6, E, 1))
    try:
        p = _params(index_rate=0.5, protect=0.33)
        with ctx.stream_open(mid, p, [2], [3.0], FB, FC, FX, FS) as se:
            assert se.frames == T28 and se.skip_head == HEAD and se.block_out == Lb
            assert se.noise_len == inter * T28 + Lb + Lx + Ls and se.tail_len == Lb + Lx + Ls
            blocks = _blocks(50, 6)
            g = np.random.default_rng(11)
            ring, carry = np.zeros(N * 160, np.float32), np.zeros(Lx, np.float64)
            pk = _params(index_rate=0.5, protect=0.33, pitch=3.0)
            for k in range(6):
                noise = g.standard_normal((1, se.noise_len)).astype(np.float32)
                out, pre, offs = se.step(blocks[k], noise=noise, taps=True)
                ring = np.concatenate([ring[FB * 160:], blocks[k, 0]])
                coarse, f0 = ctx.get_f0_x_ex(ring, N, pk)
                feats0 = ctx.hubert_features(ring, E)[0]
                feats, _, _ = ctx.index_blend(feats0, 0.5)
                up, up0 = np.repeat(feats, 2, axis=0)[:T28], np.repeat(feats0, 2, axis=0)[:T28]
                assert up.shape[0] == T28                        # 2 * Th = N - 1: the p_len clamp
                pf = f0[:T28]
                w = np.where(pf > 0, np.float32(1), np.float32(0.33)).astype(np.float32)[:, None]
                phone = up * w + up0 * (np.float32(1) - w)
                zn = noise[:, :inter * T28].reshape(1, inter, T28)
                sn = noise[:, inter * T28:]
                want, _ = ctx.synth_infer(mid, phone[None], coarse[None, :T28], pf[None], sid=[2], z_noise=zn, src_noise=sn,
                                          skip_head=HEAD)
                e_pre = rel(pre[0], want[0])
                _check_offset(pre[0], carry, Lb, Lx, Ls, int(offs[0]))
                ro, rb, _, _, _ = sola_reference(pre[0], carry, Lb, Lx, Ls, offset=int(offs[0]))
                e_out = rel(out[0], ro)
                print(f"session step {k}: pre_sola {e_pre:.2e} (rms {rms(want):.3f}), offset {int(offs[0])}, out {e_out:.2e}")
                assert np.isfinite(out).all() and e_pre < 1e-5 and e_out < 1e-5
                if k == 0:
                    assert int(offs[0]) == 0                     # an all-zero carry ties every offset
                carry = rb
    finally:
        ctx.load_index(None)
        ctx.unload_synth(mid)


# ---------------------------------------------------------------------------------------------- 5. groups
@pytest.mark.parametrize("method", ["rmvpe", "fcpe"])
def test_group_equals_single(ctx, method):
    """S = 3 with different sid and pitch per stream: every stream's blocks equal the same stream stepped alone, bit for bit
    (stream s of a group draws from Philox(seed + s): alone it is opened with that seed)."""
    from polgen_rvc_amd import _lib, synthetic as S
    E = _load_front(ctx, 7, fcpe=method == "fcpe")
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 7, input_dim=E)
    code = _lib.F0_FCPE if method == "fcpe" else _lib.F0_RMVPE
    steps = 2 if method == "fcpe" else 4
    sids, pitches, seed = [0, 3, 1], [0.0, 3.5, -2.0], 21
    blocks = _blocks(60, steps, S=3)
    try:
        with ctx.stream_open(mid, _params(seed=seed, f0_method=code), sids, pitches, FB, FC, FX, FS) as grp:
            got = [grp.step(blocks[k]) for k in range(steps)]
        assert all(np.isfinite(o).all() and o.shape == (3, grp.block_out) for o in got)
        assert rms(got[-1]) > 1e-3
        for s in range(3):
            with ctx.stream_open(mid, _params(seed=seed + s, f0_method=code), sids[s:s + 1], pitches[s:s + 1], FB, FC, FX,
                                 FS) as one:
                for k in range(steps):
                    assert np.array_equal(one.step(blocks[k, s:s + 1])[0], got[k][s]), (s, k)
        assert not np.array_equal(got[-1][0], got[-1][1])
    finally:
        ctx.unload_synth(mid)


# ---------------------------------------------------------------------------------------------- 6. replay
def test_replay_reset_and_seeds(ctx):
    from polgen_rvc_amd import synthetic as S
    E = _load_front(ctx, 8)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 8, input_dim=E)
    blocks = _blocks(70, 3, S=2)
    try:
        def run(se):
            return np.stack([se.step(blocks[k]) for k in range(3)])
        with ctx.stream_open(mid, _params(seed=31), [0, 1], [0.0, 1.0], FB, FC, FX, FS) as a:
            first = run(a)
            a.reset()
            again = run(a)
        with ctx.stream_open(mid, _params(seed=31), [0, 1], [0.0, 1.0], FB, FC, FX, FS) as b:
            fresh = run(b)
        with ctx.stream_open(mid, _params(seed=32), [0, 1], [0.0, 1.0], FB, FC, FX, FS) as c:
            other = run(c)
        assert np.array_equal(first, fresh) and np.array_equal(first, again)
        assert not np.array_equal(first, other)
        assert not np.array_equal(first[1], first[2])            # the steps of one session draw different noise
    finally:
        ctx.unload_synth(mid)


# ---------------------------------------------------------------------------------------------- 7. lifetime and neighbours
def test_lifetime_and_neighbours(ctx):
    from polgen_rvc_amd import _lib, synthetic as S
    from polgen_rvc_amd._lib import RvcxError
    E = _load_front(ctx, 9)
    mid = _load_synth(ctx, S.SYNTH_CFG_TINY, 9, input_dim=E)
    blocks = _blocks(80, 2)
    p = _params(seed=41)
    try:
        # a step after unload_synth
        mid2 = _load_synth(ctx, S.SYNTH_CFG_TINY, 10, input_dim=E)
        se = ctx.stream_open(mid2, p, [0], [0.0], FB, FC, FX, FS)
        se.step(blocks[0])
        ctx.unload_synth(mid2)
        with pytest.raises(RvcxError, match="unloaded"):
            se.step(blocks[1])
        se.close()
        # refused at open
        with pytest.raises(RvcxError, match="mangio-crepe"):
            ctx.stream_open(mid, _params(f0_method=_lib.F0_CREPE), [0], [0.0], FB, FC, FX, FS)
        with pytest.raises(RvcxError, match="exceed"):
            ctx.stream_open(mid, p, [0], [0.0], FB, 0, FX, FS)           # N = 9 frames, T = 8 < 9
        for bad in ((0, FC, FX, FS), (FB, FC, 0, FS), (FB, FC, FX, -1)):
            with pytest.raises(RvcxError):
                ctx.stream_open(mid, p, [0], [0.0], *bad)
        v1 = _load_synth(ctx, S.SYNTH_CFG_TINY, 9, input_dim=S.HUBERT_CFG_TINY["final_dim"])
        ctx.load_index(S.make_index(16, 768, 2))
        try:
            with pytest.raises(RvcxError, match="index"):
                ctx.stream_open(v1, p, [0], [0.0], FB, FC, FX, FS)
        finally:
            ctx.load_index(None)
        with ctx.stream_open(v1, p, [0], [0.0], FB, FC, FX, FS) as s1:    # the v1 path itself (layer 9 + final_proj) runs
            assert np.isfinite(s1.step(blocks[0])).all()
        ctx.unload_synth(v1)
        # a ticket submitted just before a step, and the step itself, each give what they give alone
        clip = S.make_clip(81, 1.3)
        pc = _params(seed=43)
        want_pcm, want_f32 = ctx.convert_batch(mid, [clip], pc, want_f32=True)
        with ctx.stream_open(mid, p, [0], [0.0], FB, FC, FX, FS) as a:
            want_step = [a.step(blocks[k]) for k in range(2)]
        with ctx.stream_open(mid, p, [0], [0.0], FB, FC, FX, FS) as b:
            first = b.step(blocks[0])
            t = ctx.convert_submit(mid, [clip], pc, want_f32=True)
            second = b.step(blocks[1])                                    # completes the ticket first
            assert ctx.convert_inflight() == 0
            got_pcm, got_f32 = t.wait()
        assert np.array_equal(first, want_step[0]) and np.array_equal(second, want_step[1])
        assert np.array_equal(got_pcm[0], want_pcm[0]) and np.array_equal(got_f32[0], want_f32[0])
    finally:
        ctx.unload_synth(mid)
