"""Round 5 (GPU): the shared context under threads; the Cout = 1 kernel of conv_post against torch; HuBERT
with planted outlier units against the HF twin's golden and the range guard's counters (item 4); the whole-block k = 3 ResBlock
kernel against three fused steps, bit for bit (item 6)."""
import json
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_two_threads_share_one_context_through_the_mirror(tmp_path):
    """The reference builds fresh model objects per request (rvc/scripts/voice_conversion.py:71-100), so two Gradio
    worker threads never share state there.  Here every thread of the process gets the ONE resident context and ctypes
    releases the GIL: every C entry point takes the context's mutex (csrc/api_internal.h) and the mirror holds the context's lock
    around its call sequences.  Two threads x 4 requests on one context -- different clips, different index files (so
    "make the index resident, then convert" must not interleave), one thread also asking for the F0 track -- give, bit for
    bit, what each request gives alone; no error is left on the context."""
    import faiss_writer as FW
    from polgen_rvc_amd import _lib, synthetic as S
    from polgen_rvc_amd.infer import infer as I, _state
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    seed = 3
    saved = (dict(_state._CTX), dict(_state._RESIDENT), dict(_state._SYNTHS), dict(_state._INDEX_RESIDENT))
    ctx = _lib.Context(0)
    _state._CTX.clear()
    _state._CTX[0] = ctx
    try:
        hub = I.load_hubert("cuda:0", False, None, state=S.hubert_state(hcfg, seed), cfg=hcfg)
        I.load_rmvpe("cuda:0", state=S.rmvpe_state(rcfg, seed), cfg=rcfg)
        cpt = S.synth_checkpoint(scfg, seed)
        cpt["weight"] = S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"])
        cpt, version, net_g, tgt_sr, _ = I.get_vc("cuda:0", False, I.Config(), None, cpt=cpt)
        idx = []
        for k in range(2):
            path = str(tmp_path / f"added_{k}.index")
            open(path, "wb").write(FW.flat_bytes(S.make_index(512 + 64 * k, hcfg["embed_dim"], 40 + k)))
            idx.append(path)
        clips = [S.make_clip(60 + k, 1.5 + 0.4 * k).astype(np.float64) for k in range(2)]

        def request(k):
            vc = I.VC(tgt_sr, I.Config())          # a new VC per request, like get_vc gives every caller
            vc.seed = 100 + k
            pcm = vc.pipeline(hub, net_g, 0, clips[k], "x.wav", 0.0, "rmvpe+", idx[k], 0.6, 1, 3, tgt_sr, 0, 1.0, "v2",
                              0.33, 128, None, 50, 1100)
            f0 = vc.get_f0_rmvpe(clips[k].astype(np.float32)) if k == 1 else None
            return pcm, f0

        solo = [request(k) for k in range(2)]
        assert not np.array_equal(solo[0][0][:1000], solo[1][0][:1000])
        outs, errs = [[], []], []

        def work(k):
            try:
                for _ in range(4):
                    outs[k].append(request(k))
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert len(outs[k]) == 4
            for i, (pcm, f0) in enumerate(outs[k]):
                assert np.array_equal(pcm, solo[k][0]), f"thread {k} request {i}: PCM differs from the solo run"
                if f0 is not None:
                    assert np.array_equal(f0, solo[k][1])
        assert (_lib.lib().rvcx_last_error(ctx._h) or b"") == b""
        assert ctx.gru_fallbacks() == 0
    finally:
        I.clear_cache()
        for dst, src in zip((_state._CTX, _state._RESIDENT, _state._SYNTHS, _state._INDEX_RESIDENT), saved):
            dst.clear()
            dst.update(src)
        del net_g
        ctx.close()


def test_raw_c_abi_calls_from_two_threads_queue_on_the_context_mutex():
    """Below the mirror: two threads call rvcx_convert_batch on ONE context with no Python lock at all (ctypes drops the
    GIL for the call).  Without the mutex in api_call the two calls would share the arena and the streams."""
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    c = _lib.Context(0)
    try:
        c.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, 1))
        c.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, 1))
        mid = c.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 1, input_dim=hcfg["embed_dim"]))
        params = _lib.Params(0.0, 50.0, 1100.0, 0.0, 0.33, 1.0, 0, 1, 6, 38, 41, 9)
        clips = [S.make_clip(70, 2.0), S.make_clip(71, 1.3)]
        solo = [c.convert_batch(mid, [clips[k]], params)[0].copy() for k in range(2)]
        outs, errs = [[], []], []

        def work(k):
            try:
                for _ in range(6):
                    outs[k].append(c.convert_batch(mid, [clips[k]], params)[0].copy())
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert solo[k].ndim == 1 and solo[k].shape[0] > 1000
            assert all(np.array_equal(o, solo[k]) for o in outs[k]) and len(outs[k]) == 6
    finally:
        c.close()


@pytest.mark.parametrize("B,Cin,T", [(1, 32, 4096), (2, 32, 1000), (1, 32, 20), (1, 64, 2052), (3, 16, 516)])
def test_conv_post_shape_runs_the_cout1_kernel_and_matches_torch(ctx, B, Cin, T):
    """NSF conv_post (nsf.py:142-144): leaky_relu(0.01) -> Conv1d(C, 1, 7, padding 3, no bias) -> tanh.  Round 5 gives
    Cout = 1 layers a vector-FMA kernel (csrc/conv_fast.hip: conv_cout1_kernel, exact fp32) instead of a 32-row MFMA tile
    with 31 rows of padding; per-item lengths zero the input beyond len and the output beyond len."""
    import torch
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(B * 1000 + Cin + T)
    x = torch.randn(B, Cin, T, generator=gen)
    w = torch.randn(1, Cin, 7, generator=gen) / (Cin * 7) ** 0.5
    ref = torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), w, None, padding=3)).numpy()
    got = ctx.conv1d(x.numpy(), w.numpy(), None, pad_left=3, pre_lrelu=0.01, act=4)
    assert got.shape == ref.shape and np.abs(got - ref).max() < 2e-6
    if B > 1:
        lens = np.array([T - 5 * (i + 1) - 2 for i in range(B)], np.int32)
        xm = x.clone()
        for i, n in enumerate(lens):
            xm[i, :, n:] = 0
        ref = torch.tanh(F.conv1d(F.leaky_relu(xm, 0.01), w, None, padding=3)).numpy()
        for i, n in enumerate(lens):
            ref[i, :, n:] = 0
        got = ctx.conv1d(x.numpy(), w.numpy(), None, pad_left=3, pre_lrelu=0.01, act=4, lens_in=lens, lens_out=lens)
        assert np.abs(got - ref).max() < 2e-6


def test_hubert_with_planted_outlier_units_pins_exactly_the_two_attention_layers(tmp_path):
    """real ContentVec / HuBERT-base weights have massive-activation units.  synthetic.hubert_state(
    outliers=True) plants them at published magnitudes: FFN units of 400-900 in layers 2 / 6 / 10 (inside the split
    kernels' range of 6e4: nothing may be pinned for them) and a V head of ~1200 in layers 4 / 8 (beyond the attention
    kernel's fp16 range for K / V, 255).  Expected: the layer-12 features match the golden of the HF twin on the same
    weights (fixture hubert_base_1s_outliers, tools/gen_golden.py), exactly TWO layers end up pinned to the exact-fp32
    kernels -- found during the first call, one repeated call per offender -- and the second call repeats nothing."""
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    from conftest import rms
    d = np.load(os.path.join(GOLD, "hubert_base_1s_outliers.npz"))
    cfg = json.loads(str(d["cfg"]))
    assert float(d["outlier_max_v"]) > 255 and 300 < float(d["outlier_max_ffn"]) < 6e4
    c = _lib.Context(0)
    try:
        c.load_hubert(W.hubert_cfg_struct(cfg), S.hubert_state(cfg, int(d["seed"]), outliers=True))
        assert c.fp32_layers() == 0
        r0 = c.fp32_reruns()
        got = c.hubert_features(d["wav"], cfg["embed_dim"], cfg["layers"])
        e = rms(got - d["out"]) / rms(d["out"])
        pinned, reruns = c.fp32_layers(), c.fp32_reruns() - r0
        print(f"hubert with planted outliers: rel err {e:.3e}; layers pinned to fp32 {pinned}, repeated calls {reruns}")
        assert e < 1e-4
        assert pinned == len(S.OUTLIER_V_LAYERS) == 2 and reruns == 2
        again = c.hubert_features(d["wav"], cfg["embed_dim"], cfg["layers"])
        assert c.fp32_reruns() - r0 == 2 and c.fp32_layers() == 2 and np.array_equal(again, got)
    finally:
        c.close()


@pytest.mark.parametrize("C,T,B", [(32, 5000, 1), (32, 488 * 3, 1), (32, 100, 1), (64, 4100, 1), (64, 168 * 2 + 4, 2), (32, 2048, 3)])
def test_resblock3_equals_three_fused_steps(ctx, C, T, B):
    """the three dilation steps (d = 1, 3, 5) of a kernel-size-3 ResBlock1 (residuals.py:15-62) in ONE
    kernel (csrc/resblock3.hip) -- bit-identical to three launches of the fused single step (and so to the six conv
    launches), with per-item lengths, for tiles at both ends of the sequence and sequences shorter than one tile."""
    g = np.random.Generator(np.random.PCG64(C * 7 + T))
    x = g.standard_normal((B, C, T)).astype(np.float32)
    w1 = (g.standard_normal((3, C, C, 3)) / np.sqrt(3 * C)).astype(np.float32)
    w2 = (g.standard_normal((3, C, C, 3)) / np.sqrt(3 * C)).astype(np.float32)
    b1 = (0.1 * g.standard_normal((3, C))).astype(np.float32)
    b2 = (0.1 * g.standard_normal((3, C))).astype(np.float32)
    lens = None if B == 1 else np.array([T - 4 * (7 * i + 3) for i in range(B)], np.int32)
    ref = x
    for s, d in enumerate((1, 3, 5)):
        ref = ctx.resblock_pair(ref, w1[s], b1[s], w2[s], b2[s], dil=d, slope=0.1, fused=True, lens=lens)
    got = ctx.resblock3(x, w1, b1, w2, b2, dils=(1, 3, 5), slope=0.1, lens=lens)
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref), f"max abs diff {np.abs(got - ref).max():.3e}"
    if lens is not None:
        for i, n in enumerate(lens):
            assert not got[i, :, n:].any() and got[i, :, :n].any()

