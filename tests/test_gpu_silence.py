"""Digital silence through VC.pipeline against the reference's own output (tools/gen_golden.py SILENCE_RECIPES): clips of
zeros, zero gaps under every cut window, zero ends.  Real inputs (separated or gated vocals) have all three; the other
fixtures are voiced everywhere and never exactly zero.

Bars: those of test_gpu_pipeline.test_pipeline_vs_reference_golden, unchanged (TINY_RMS_BAR on the float waveform,
FULL_PCM_BAR and < 2 % of samples over 1 LSB on PCM, the reference's output length, coarse / voicing / f0 as there), plus
f0 == 0 on exactly the reference's unvoiced frames inside every zero span, and the reference's cut points exactly."""
import json
import os

import numpy as np
import pytest

from conftest import FULL_PCM_BAR, TINY_RMS_BAR, rms
from test_gpu_pipeline import _pack_noise, _setup

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TAGS = ["tiny_silent", "tiny_silent_env", "tiny_silent_cut", "tiny_gap_cut", "tiny_lead_trail", "gap_real_geo"]


def _clip(d):
    from polgen_rvc_amd import synthetic as S
    return S.make_gapped_clip(int(d["clip"]), float(d["seconds"]), [tuple(s) for s in d["zero_spans"]])


def _noise(d, tgt_sr):
    """the reference's Gaussian draws: stored, or (long clips) regenerated from the private generator's seed in its draw
    order, z_noise then src_noise per chunk"""
    if "z_noise_0" in d.files:
        return _pack_noise(d)
    import torch
    inter, upp = json.loads(str(d["cfgs"]))[2][2], int(tgt_sr) // 100
    gen = torch.Generator().manual_seed(int(d["noise_seed"]))
    parts = []
    for n in d["chunk_lens"]:
        T = int(n) // upp
        parts += [torch.randn((1, inter, T), generator=gen).numpy().ravel(), torch.randn((1, T * upp, 1), generator=gen).numpy().ravel()]
    return np.concatenate(parts).astype(np.float32)


def _vc(ctx, d):
    from polgen_rvc_amd.infer import infer as I
    hub, cpt = _setup(ctx, json.loads(str(d["cfgs"])), int(d["seed"]))
    cfg = I.Config()
    cfg.x_pad, cfg.x_query, cfg.x_center, cfg.x_max = [int(v) for v in d["geo"]]
    cpt, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, cfg, None, cpt=cpt)
    return hub, net_g, tgt_sr, vc


@pytest.mark.parametrize("tag", TAGS)
def test_silence_vs_reference_golden(ctx, tag):
    """The cut points must equal the reference's exactly, not just per frame: the cut search runs on a filter that
    reproduces scipy.signal.filtfilt bit for bit (tests/test_silence_recipes.py checks that on every recipe), and the
    window sums keep numpy's order, so there is no rounding that could move a cut by even one sample."""
    d = np.load(os.path.join(GOLD, f"pipeline_{tag}.npz"))
    hub, net_g, tgt_sr, vc = _vc(ctx, d)
    audio = _clip(d)
    pcm, f32 = vc.pipeline(hub, net_g, 0, audio.astype(np.float64), "x.wav", float(d["pitch"]), "rmvpe+", None, 0, 1, 3,
                           tgt_sr, 0, float(d["volume_envelope"]), "v2", float(d["protect"]), 128, None,
                           float(d["f0_min"]), float(d["f0_max"]), noise=_noise(d, tgt_sr), return_f32=True)
    ref = d["pcm"]
    assert pcm.shape == ref.shape, (pcm.shape, ref.shape)
    diff = np.abs(pcm.astype(np.int32) - ref.astype(np.int32))
    print(f"{tag}: pcm max diff {diff.max()} LSB, frac>1 {np.mean(diff > 1):.2e}, peak {np.abs(ref).max()}")
    assert diff.max() <= FULL_PCM_BAR and np.mean(diff > 1) < 0.02, f"{tag}: pcm max diff {diff.max()} LSB"
    if not ref.any():
        # the envelope over silence: rms1 = 0, so the reference's output is 0 * max(rms2, 1e-6)^(rate-1) = exact zeros
        assert not pcm.any() and not f32.any()
    if float(d["volume_envelope"]) == 1.0:
        tp = int(tgt_sr) * int(d["geo"][0])
        lens = [int(v) for v in d["chunk_lens"]]
        offs = np.concatenate([[0], np.cumsum(lens)])
        st = int(d["stride"])
        # the trimmed, concatenated vc() outputs (pipeline.py:397,449); a long clip's fixture holds every st-th raw sample
        keep = np.concatenate([np.arange(offs[i] + tp, offs[i + 1] - tp) for i in range(len(lens))])
        pos = np.arange(len(keep))
        on_grid = keep % st == 0
        raw = d["raw"] if st == 1 else d["raw_samples"]
        ref_f32 = raw[keep[on_grid] // st]
        e = rms(f32[pos[on_grid]] - ref_f32)
        print(f"{tag}: float rms err {e:.3e} (rms {rms(ref_f32):.3f})")
        assert e < TINY_RMS_BAR, f"{tag}: float rms err {e:.3e}"
    # f0 / coarse as VC.get_f0 returns them (pipeline.py:348,362)
    x = np.pad(ctx.highpass(audio.astype(np.float64)), (vc.t_pad, vc.t_pad), mode="reflect")
    coarse, f0 = vc.get_f0("x.wav", x, len(d["f0"]), float(d["pitch"]), "rmvpe+", 3, 128, None,
                           float(d["f0_min"]), float(d["f0_max"]))
    coarse, f0 = coarse[:len(d["f0"])], f0[:len(d["f0"])]
    assert np.mean(coarse != d["coarse"]) < 1e-3
    v = (d["f0"] > 0) & (f0 > 0)
    assert np.mean((d["f0"] > 0) != (f0 > 0)) < 1e-2
    if v.any():
        assert np.abs(f0[v] - d["f0"][v]).max() / d["f0"][v].max() < 1e-3
    # inside every zero span (frames wholly in it, in padded coordinates): unvoiced exactly where the reference is
    spans = [(0.0, float(d["seconds"]))] if int(d["clip"]) < 0 else [tuple(s) for s in d["zero_spans"]]
    for a, b in spans:
        f_lo = -(-(int(round(a * 16000)) + vc.t_pad) // 160)
        f_hi = (int(round(b * 16000)) + vc.t_pad) // 160 - 1
        if f_hi <= f_lo:
            continue
        sl = slice(f_lo, f_hi)
        assert np.array_equal(f0[sl] == 0, d["f0"][sl] == 0), (a, b)
        if int(d["clip"]) < 0:
            assert not (d["f0"] > 0).any() and not (f0 > 0).any()     # silence is unvoiced: SineGen's unvoiced branch only
    cuts = ctx.last_cuts()                    # of the vc.pipeline call above (get_f0 is no convert_batch call)
    print(f"{tag}: cuts {cuts} (reference {d['cuts'].tolist()})")
    assert cuts == [d["cuts"].tolist()], (cuts, d["cuts"].tolist())


def test_gap_cut_protect_with_index_vs_reference_golden(ctx):
    """The gapped clip with the protect mix live: a retrieval index (4 centres in 8 identical copies, stored in the
    fixture) at index_rate 0.75 makes feats0 != feats, so the unvoiced frames of the gaps take
    feats * 0.33 + feats0 * 0.67 (pipeline.py:237-270).  The bars of test_silence_vs_reference_golden."""
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    d = np.load(os.path.join(GOLD, "pipeline_tiny_gap_cut_index.npz"))
    hcfg, rcfg, scfg = json.loads(str(d["cfgs"]))
    seed = int(d["seed"])
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, seed))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, seed))
    mid = ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"]))
    ctx.load_index(np.ascontiguousarray(d["index_rows"], np.float32))
    try:
        p = _lib.Params()
        p.pitch, p.f0_min, p.f0_max, p.index_rate, p.protect, p.volume_envelope = 0, 50, 1100, float(d["index_rate"]), 0.33, 1.0
        p.sid, p.x_pad, p.x_query, p.x_center, p.x_max, p.seed = 0, *[int(v) for v in d["geo"]], 0
        (pcm,), (f32,) = ctx.convert_batch(mid, [_clip(d)], p, noises=[_pack_noise(d)], want_f32=True)
        cuts = ctx.last_cuts()
        ref = d["pcm"]
        assert pcm.shape == ref.shape, (pcm.shape, ref.shape)
        diff = np.abs(pcm.astype(np.int32) - ref.astype(np.int32))
        tp = int(scfg[-1]) * int(d["geo"][0])
        lens = [int(v) for v in d["chunk_lens"]]
        offs = np.concatenate([[0], np.cumsum(lens)])
        ref_f32 = np.concatenate([d["raw"][offs[i] + tp: offs[i + 1] - tp] for i in range(len(lens))])
        e = rms(f32 - ref_f32)
        print(f"gap_cut_index: pcm max diff {diff.max()} LSB, frac>1 {np.mean(diff > 1):.2e}; float rms err {e:.3e}; "
              f"cuts {cuts}; unvoiced frames {int((d['f0'] == 0).sum())}")
        assert diff.max() <= FULL_PCM_BAR and np.mean(diff > 1) < 0.02
        assert e < TINY_RMS_BAR
        assert cuts == [d["cuts"].tolist()]
        assert (d["f0"] == 0).any()          # the blend is reached
    finally:
        ctx.load_index(None)
        _lib.lib().rvcx_unload_synth(ctx._h, mid)


def test_silence_batch_members_equal_single_runs(ctx):
    """The gapped clip and the silent clip (both cut, one micro-batch) and a ragged uncut member with zero ends in one
    convert_batch: each bit-identical to its single run (Philox seed + position), with the same cut points, which are
    the reference's."""
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    dg = np.load(os.path.join(GOLD, "pipeline_tiny_gap_cut.npz"))
    ds = np.load(os.path.join(GOLD, "pipeline_tiny_silent_cut.npz"))
    hcfg, rcfg, scfg = json.loads(str(dg["cfgs"]))
    seed = int(dg["seed"])
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, seed))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, seed))
    mid = ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"]))
    try:
        clips = [_clip(dg), _clip(ds), S.make_gapped_clip(45, 2.3, [(0.0, 0.4), (2.0, 2.3)])]

        def params(seed_):
            p = _lib.Params()
            p.pitch, p.f0_min, p.f0_max, p.index_rate, p.protect, p.volume_envelope = 0, 50, 1100, 0, 0.33, 1.0
            p.sid, p.x_pad, p.x_query, p.x_center, p.x_max, p.seed = 0, 1, 1, 2, 3, seed_
            return p

        pcm, f32 = ctx.convert_batch(mid, clips, params(7), want_f32=True)
        cuts = ctx.last_cuts()
        print(f"batch: micro-batches {ctx.last_micro_batches()}, cuts {cuts}")
        assert cuts == [dg["cuts"].tolist(), ds["cuts"].tolist(), []]
        for i, c in enumerate(clips):
            a_pcm, a_f32 = ctx.convert_batch(mid, [c], params(7 + i), want_f32=True)
            assert ctx.last_cuts() == [cuts[i]], i
            assert np.array_equal(a_f32[0], f32[i]), i
            assert np.array_equal(a_pcm[0], pcm[i]), i
    finally:
        _lib.lib().rvcx_unload_synth(ctx._h, mid)
