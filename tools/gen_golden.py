#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own modules (imported read-only from
/root/reference in the build container) on deterministic synthetic weights, and check the
oracle (oracle/*.py) against them while doing so.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py [--full]

Nothing from /root/reference is copied: the fixtures hold inputs and expected outputs only;
weights are regenerated on both sides from polgen-rvc_amd/synthetic.py.  Absent third-party
modules are replaced by import-time stubs; HuBERT (fairseq, absent)
is represented by transformers.HubertModel with the same synthetic weights mapped onto HF
names, which is also the cross-check that pins oracle/hubert.py.
"""
import argparse
import hashlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import numpy as np
import torch
import transformers  # noqa: E402  (must be imported before the stubs, Appendix A.1)
from transformers import HubertConfig, HubertModel

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_stubs"))
REF = "/root/reference"
sys.path.append(REF)
for name in ("torchcrepe", "faiss", "soundfile", "torchaudio", "local_attention"):
    sys.modules[name] = types.ModuleType(name)
ta = types.ModuleType("torchaudio.transforms")
ta.Resample = object
sys.modules["torchaudio.transforms"] = ta
sys.modules["torchaudio"].transforms = ta
sys.modules["local_attention"].LocalAttention = object



class _FlatIndex:
    """Stand-in for ``faiss.read_index`` (faiss-cpu 1.7.3 is not installed): exact squared-L2 top-k, the
    IndexFlatL2 semantics.  Only ``search`` / ``reconstruct_n`` / ``ntotal`` are restated -- the blend arithmetic
    around them (pipeline.py:239-250) is the REFERENCE's own code.  Parity with real faiss stays unpinned."""

    def __init__(self, big):
        self.big = np.ascontiguousarray(big, np.float32)
        self.ntotal, self.d = self.big.shape
        self.searches = []
        self.dists = []

    def reconstruct_n(self, i0, n):
        return self.big[i0:i0 + n]

    def search(self, x, k):
        q, b = x.astype(np.float64), self.big.astype(np.float64)
        d2 = (q * q).sum(1)[:, None] - 2.0 * q @ b.T + (b * b).sum(1)[None, :]
        ix = np.argsort(d2, axis=1, kind="stable")[:, :k]
        self.searches.append(ix.copy())
        self.dists.append(np.sort(d2, axis=1)[:, :9])
        return np.take_along_axis(d2, ix, axis=1).astype(np.float32), ix.astype(np.int64)


_INDEX_FILES = {}
sys.modules["faiss"].read_index = lambda path: _INDEX_FILES[path]

import polgen_rvc_amd  # noqa: E402
from polgen_rvc_amd import synthetic as S  # noqa: E402
from oracle import synth as O_synth, rmvpe as O_rmvpe, hubert as O_hubert, pipeline as O_pipe, fcpe as O_fcpe  # noqa: E402

import rvc.infer.pipeline as P  # noqa: E402  (reference)
from rvc.lib.algorithm.synthesizers import Synthesizer  # noqa: E402
from rvc.lib.predictors import RMVPE as R  # noqa: E402
from rvc.lib.predictors import FCPE as RF  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
os.makedirs(GOLD, exist_ok=True)
torch.set_grad_enabled(False)


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


def report(tag, ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    err = rms(ref - got)
    print(f"  {tag:34s} rms_ref={rms(ref):.4e} rms_err={err:.3e} max_err={np.abs(ref - got).max():.3e}")
    return err


# ------------------------------------------------------------------ reference model builders
def ref_synth(cfg, sd):
    net = Synthesizer(*cfg, use_f0=1, input_dim=sd["enc_p.emb_phone.weight"].shape[1], is_half=False)
    del net.enc_q
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    return net.eval()


def ref_rmvpe(cfg, sd):
    pred = R.RMVPE0Predictor.__new__(R.RMVPE0Predictor)
    pred.is_half, pred.device, pred.resample_kernel = False, "cpu", {}
    pred.mel_extractor = R.MelSpectrogram(False, 128, 16000, 1024, 160, None, 30, 8000)
    model = R.E2E(cfg["n_blocks"], cfg["n_gru"], (2, 2), cfg["en_de_layers"], cfg["inter_layers"],
                  cfg["in_channels"], cfg["en_out_channels"])
    model.load_state_dict(sd)
    pred.model = model.eval()
    pred.cents_mapping = np.pad(20 * np.arange(360) + 1997.3794084376191, (4, 4))
    return pred


def hf_hubert(cfg, sd):
    hc = HubertConfig(hidden_size=cfg["embed_dim"], num_hidden_layers=cfg["layers"],
                      num_attention_heads=cfg["heads"], intermediate_size=cfg["ffn_dim"],
                      conv_dim=[cfg["conv_dim"]] * 7, conv_kernel=cfg["conv_kernels"],
                      conv_stride=cfg["conv_strides"], num_conv_pos_embeddings=cfg["pos_kernel"],
                      num_conv_pos_embedding_groups=cfg["pos_groups"], hidden_dropout=0.0,
                      attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0,
                      layerdrop=0.0, final_dropout=0.0, mask_time_prob=0.0)
    hc._attn_implementation = "eager"
    m = HubertModel(hc).eval()
    mp = {}
    for i in range(7):
        mp[f"feature_extractor.conv_layers.{i}.conv.weight"] = sd[f"feature_extractor.conv_layers.{i}.0.weight"]
    mp["feature_extractor.conv_layers.0.layer_norm.weight"] = sd["feature_extractor.conv_layers.0.2.weight"]
    mp["feature_extractor.conv_layers.0.layer_norm.bias"] = sd["feature_extractor.conv_layers.0.2.bias"]
    mp["feature_projection.layer_norm.weight"] = sd["layer_norm.weight"]
    mp["feature_projection.layer_norm.bias"] = sd["layer_norm.bias"]
    mp["feature_projection.projection.weight"] = sd["post_extract_proj.weight"]
    mp["feature_projection.projection.bias"] = sd["post_extract_proj.bias"]
    mp["encoder.pos_conv_embed.conv.bias"] = sd["encoder.pos_conv.0.bias"]
    mp["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = sd["encoder.pos_conv.0.weight_g"]
    mp["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = sd["encoder.pos_conv.0.weight_v"]
    mp["encoder.layer_norm.weight"] = sd["encoder.layer_norm.weight"]
    mp["encoder.layer_norm.bias"] = sd["encoder.layer_norm.bias"]
    for l in range(cfg["layers"]):
        a, b = f"encoder.layers.{l}", f"encoder.layers.{l}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            for wb in ("weight", "bias"):
                mp[f"{a}.attention.{n}.{wb}"] = sd[f"{b}.self_attn.{n}.{wb}"]
        for wb in ("weight", "bias"):
            mp[f"{a}.layer_norm.{wb}"] = sd[f"{b}.self_attn_layer_norm.{wb}"]
            mp[f"{a}.feed_forward.intermediate_dense.{wb}"] = sd[f"{b}.fc1.{wb}"]
            mp[f"{a}.feed_forward.output_dense.{wb}"] = sd[f"{b}.fc2.{wb}"]
            mp[f"{a}.final_layer_norm.{wb}"] = sd[f"{b}.final_layer_norm.{wb}"]
    res = m.load_state_dict(mp, strict=False)
    assert not res.unexpected_keys and all("masked_spec_embed" in k for k in res.missing_keys), res
    return m


class HubertAdapter(torch.nn.Module):
    """``extract_features(source, padding_mask, output_layer)`` around the HF twin (Appendix A.6)."""

    def __init__(self, hf, sd=None):
        super().__init__()
        self.hf = hf
        if sd is not None and "final_proj.weight" in sd:       # fairseq's HubertModel.final_proj: RVC v1 voice models (pipeline.py:236)
            w = sd["final_proj.weight"]
            self.final_proj = torch.nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                self.final_proj.weight.copy_(w)
                self.final_proj.bias.copy_(sd["final_proj.bias"])

    def extract_features(self, source, padding_mask=None, output_layer=12):
        out = self.hf(source, output_hidden_states=True)
        return out.hidden_states[min(output_layer, len(out.hidden_states) - 1)], None


class Cfg:
    def __init__(self, geo):
        self.device, self.is_half = "cpu", False
        self.x_pad, self.x_query, self.x_center, self.x_max = geo


# ------------------------------------------------------------------ stage goldens
def gold_synth(tag, cfg, T, seed, outliers=False):
    print(f"[synth {tag}] T={T} outliers={outliers}")
    sd = S.to_torch(S.synth_state(cfg, seed, outliers=outliers))
    net = ref_synth(cfg, sd)
    c = O_synth.cfg_fields(cfg)
    g = torch.Generator().manual_seed(100 + seed)
    phone = torch.randn(1, T, 768, generator=g)
    pitch = torch.randint(1, 256, (1, T), generator=g)
    f0 = 100 + 300 * torch.rand(1, T, generator=g)
    f0[:, T // 3: T // 3 + max(2, T // 8)] = 0          # an unvoiced stretch
    pitch[f0 == 0] = 1
    z_noise = torch.randn(1, c["inter"], T, generator=g)
    src_noise = torch.randn(1, T * c["upp"], 1, generator=g)
    draws = [z_noise, src_noise]
    orig = torch.randn_like
    it = iter(draws)
    torch.randn_like = lambda x, **kw: next(it)
    try:
        o, x_mask, (z, z_p, m_p, logs_p) = net.infer(phone, torch.tensor([T]), pitch, f0, torch.tensor([0]))
    finally:
        torch.randn_like = orig
    oo, parts = O_synth.synthesizer_infer(sd, cfg, phone, torch.tensor([T]), pitch, f0, torch.tensor([0]),
                                          z_noise, src_noise, return_parts=True)
    report("m_p", m_p, parts["m_p"]); report("logs_p", logs_p, parts["logs_p"])
    report("z", z, parts["z"])
    e = report("audio", o, oo)
    assert e < 1e-5, e
    np.savez_compressed(os.path.join(GOLD, f"synth_{tag}.npz"), seed=seed, cfg=json.dumps(cfg), outliers=bool(outliers),
                        phone=phone.numpy(), pitch=pitch.numpy(), f0=f0.numpy(), z_noise=z_noise.numpy(),
                        src_noise=src_noise.numpy().astype(np.float32), m_p=m_p.numpy(), logs_p=logs_p.numpy(),
                        z_p=z_p.numpy(), z=z.numpy(), audio=o.numpy())


def gold_synth_head(tag, cfg, T, seed, rate):
    """Synthesizer.infer(..., rate=torch.tensor(rate)) (synthesizers.py:175-181): the flow, the source and the decoder see
    frames [head:] only.  Inputs as gold_synth draws them; the first randn_like draw is (1, inter, T), the second
    (1, (T - head) * upp, 1).  audio_full_tail: the tail of the FULL evaluation with the same z_noise (and a source noise
    whose tail is src_noise) -- what slicing a plain call would give, the negative control of the GPU test."""
    from polgen_rvc_amd._lib import head_from_rate
    sd = S.to_torch(S.synth_state(cfg, seed))
    net = ref_synth(cfg, sd)
    c = O_synth.cfg_fields(cfg)
    g = torch.Generator().manual_seed(100 + seed)
    phone = torch.randn(1, T, 768, generator=g)
    pitch = torch.randint(1, 256, (1, T), generator=g)
    f0 = 100 + 300 * torch.rand(1, T, generator=g)
    f0[:, T // 3: T // 3 + max(2, T // 8)] = 0          # an unvoiced stretch
    pitch[f0 == 0] = 1
    z_noise = torch.randn(1, c["inter"], T, generator=g)
    src_full = torch.randn(1, T * c["upp"], 1, generator=g)
    r = torch.tensor(rate)                               # float32, as a caller of the reference passes it
    head = int(T * (1.0 - r.item()))
    assert head == head_from_rate(T, rate), (head, head_from_rate(T, rate))
    print(f"[synth_head {tag}] T={T} rate={rate} head={head}")
    src_noise = src_full[:, head * c["upp"]:].contiguous()
    orig = torch.randn_like

    def run(draws, **kw):
        it = iter(draws)
        torch.randn_like = lambda x, **k2: next(it)
        try:
            return net.infer(phone, torch.tensor([T]), pitch, f0, torch.tensor([0]), **kw)
        finally:
            torch.randn_like = orig
    o, x_mask, (z, z_p, m_p, logs_p) = run([z_noise, src_noise], rate=r)
    assert o.shape[-1] == (T - head) * c["upp"] and z.shape[-1] == T - head, (o.shape, z.shape)
    o_full = run([z_noise, src_full])[0]
    tail = o_full[..., head * c["upp"]:]
    # oracle/synth.py restates rate=None only: the sliced result is the reference's alone
    print(f"  reference only (the oracle has no slice): rms(audio)={rms(o):.4e}, tail of the full evaluation differs by "
          f"{rms(o - tail):.3e} rms = {rms(o - tail) / rms(o):.3f} relative")
    np.savez_compressed(os.path.join(GOLD, f"synth_head_{tag}.npz"), seed=seed, cfg=json.dumps(cfg), rate=np.float32(rate),
                        head=head, phone=phone.numpy(), pitch=pitch.numpy(), f0=f0.numpy(), z_noise=z_noise.numpy(),
                        src_noise=src_noise.numpy().astype(np.float32), z=z.numpy(), audio=o.numpy(),
                        audio_full_tail=tail.numpy())


def stable_seed(rcfg, audio_pad_f32, seed, f0_min=50, f0_max=1100, pitch=0.0, tries=40):
    """First seed >= `seed` (step 100) for which every frame's f0 decision is well-conditioned (None if `tries`
    seeds were not enough)."""
    for k in range(tries):
        sd_ = S.to_torch(S.rmvpe_state(rcfg, seed + 100 * k))
        f0_, hid_, _ = O_rmvpe.infer_f0(sd_, rcfg, audio_pad_f32, 0.03, f0_min, f0_max, return_hidden=True)
        bad = O_rmvpe.unstable_frames(hid_, 0.03, f0_min, f0_max)
        # coarse quantisation ties (np.rint at .5)
        f0m = 1127 * np.log(1 + f0_ * 2 ** (pitch / 12) / 700)
        m0, m1 = 1127 * np.log(1 + f0_min / 700), 1127 * np.log(1 + f0_max / 700)
        q = (f0m - m0) * 254 / (m1 - m0) + 1
        tie = (f0_ > 0) & (np.abs(q - np.floor(q) - 0.5) < 1e-3)
        vf = (f0_ > 0).mean()
        print(f"  seed {seed + 100 * k}: unstable frames {len(bad)}, coarse ties {int(tie.sum())}, voiced {vf:.2f}")
        if len(bad) == 0 and not tie.any() and 0.15 < vf < 0.995:
            return seed + 100 * k
    if tries < 40:
        return None
    raise RuntimeError("no stable seed found")


def gold_rmvpe(tag, cfg, seconds, seed, stride=1, outliers=False):
    print(f"[rmvpe {tag}] {seconds}s outliers={outliers}")
    audio = S.make_clip(7 + seed, seconds).astype(np.float64)
    seed = stable_seed(cfg, audio.astype(np.float32), seed)      # the planting is function-preserving: same conditioning
    sd = S.to_torch(S.rmvpe_state(cfg, seed, outliers=outliers))
    pred = ref_rmvpe(cfg, sd)
    a = torch.from_numpy(audio).float().unsqueeze(0)
    mel = pred.mel_extractor(a, center=True)
    hid = pred.mel2hidden(mel).squeeze(0).numpy()
    f0 = pred.infer_from_audio_with_pitch(audio, thred=0.03, f0_min=50, f0_max=1100)
    of0, ohid, omel = O_rmvpe.infer_f0(sd, cfg, audio, return_hidden=True)
    report("mel", mel, omel); e1 = report("hidden", hid, ohid); e2 = report("f0", f0, of0)
    assert e1 < 1e-5 and e2 < 1e-2, (e1, e2)
    print(f"  voiced frames {int((f0 > 0).sum())}/{len(f0)}  hidden max {hid.max():.3f}")
    np.savez_compressed(os.path.join(GOLD, f"rmvpe_{tag}.npz"), seed=seed, cfg=json.dumps(cfg), outliers=bool(outliers),
                        audio=audio.astype(np.float32), mel=mel.numpy()[:, :, ::stride],
                        hidden=hid[::stride], f0=f0, stride=stride)


def gold_rmvpe_illcond(tag="illcond", cfg=None, clip=60, seconds=1.5, seed=4):
    """An instance the other fixtures avoid on purpose: one frame whose salience argmax is a near-tie
    (oracle.rmvpe.unstable_frames), so its f0 may legitimately flip under fp32 rounding noise -- for the reference
    itself across BLAS builds too.  The fixture records WHICH frames are ill-conditioned; the GPU test bounds the
    number and the location of differing frames instead of requiring equality there."""
    cfg = cfg or S.RMVPE_CFG_TINY
    audio = S.make_clip(clip, seconds).astype(np.float64)
    sd = S.to_torch(S.rmvpe_state(cfg, seed))
    pred = ref_rmvpe(cfg, sd)
    a = torch.from_numpy(audio).float().unsqueeze(0)
    hid = pred.mel2hidden(pred.mel_extractor(a, center=True)).squeeze(0).numpy()
    f0 = pred.infer_from_audio_with_pitch(audio, thred=0.03, f0_min=50, f0_max=1100)
    of0, ohid, _ = O_rmvpe.infer_f0(sd, cfg, audio, return_hidden=True)
    bad = O_rmvpe.unstable_frames(hid, 0.03, 50, 1100)
    print(f"[rmvpe {tag}] unstable frames {bad.tolist()}  voiced {int((f0 > 0).sum())}/{len(f0)}")
    assert 1 <= len(bad) <= 8, "pick another (clip, seed): this one is not ill-conditioned"
    report("hidden", hid, ohid)
    np.savez_compressed(os.path.join(GOLD, f"rmvpe_{tag}.npz"), seed=seed, cfg=json.dumps(cfg), clip=clip, seconds=seconds,
                        hidden=hid, f0=f0, unstable=bad.astype(np.int32))


def gold_hubert(tag, cfg, seconds, seed, outliers=False):
    print(f"[hubert {tag}] {seconds}s  (HF twin; fairseq absent -> parity unpinned by the reference)")
    sd = S.to_torch(S.hubert_state(cfg, seed, outliers=outliers))
    hf = hf_hubert(cfg, sd)
    wav = torch.from_numpy(S.make_clip(3 + seed, seconds)).unsqueeze(0)
    out = hf(wav, output_hidden_states=True)
    L = cfg["layers"]
    mine, parts = O_hubert.extract_features(sd, cfg, wav, L, return_parts=True)
    e = report(f"layer{L}", out.hidden_states[L], mine)
    report("layer1", out.hidden_states[1], O_hubert.extract_features(sd, cfg, wav, 1))
    assert e < 2e-5, e
    extra = {}
    if outliers:
        # the magnitudes the planted units really reach on this clip (HF twin's own activations), for the record and the test
        acts = {}
        hooks = []
        for l in set(S.OUTLIER_FFN_LAYERS) | set(S.OUTLIER_V_LAYERS):
            lay = hf.encoder.layers[l]
            hooks.append(lay.feed_forward.intermediate_act_fn.register_forward_hook(
                lambda m, i, o, l=l: acts.__setitem__(f"ffn{l}", float(o.abs().max()))) if hasattr(lay.feed_forward.intermediate_act_fn, "register_forward_hook") else None)
            hooks.append(lay.attention.v_proj.register_forward_hook(lambda m, i, o, l=l: acts.__setitem__(f"v{l}", float(o.abs().max()))))
            hooks.append(lay.feed_forward.intermediate_dense.register_forward_hook(
                lambda m, i, o, l=l: acts.__setitem__(f"fc1_{l}", float(o.abs().max()))))
        hf(wav)
        for hk in hooks:
            if hk is not None:
                hk.remove()
        print("   planted-outlier magnitudes:", {k: round(v, 1) for k, v in sorted(acts.items())})
        extra = dict(outlier_max_v=max(v for k, v in acts.items() if k.startswith("v")),
                     outlier_max_ffn=max(v for k, v in acts.items() if k.startswith("fc1_")))
    np.savez_compressed(os.path.join(GOLD, f"hubert_{tag}.npz"), seed=seed, cfg=json.dumps(cfg),
                        wav=wav.numpy(), out=out.hidden_states[L].numpy(),
                        out_l1=out.hidden_states[1].numpy(), **extra)


VC_IN_LENS = []


def run_ref_pipeline(models_cfg, geo, audio, pitch, volume_envelope, protect, f0_min, f0_max, seed,
                     tgt_sr, file_index=None, index_rate=0, prebuilt=None, f0_method="rmvpe+", version="v2", sid=0):
    (hcfg, hsd), (rcfg, rsd), (scfg, ssd) = models_cfg
    vc = P.VC(tgt_sr, Cfg(geo))
    if prebuilt is None:
        prebuilt = (ref_rmvpe(rcfg, rsd), HubertAdapter(hf_hubert(hcfg, hsd), hsd))
    vc.model_rmvpe, hub = prebuilt
    net = ref_synth(scfg, ssd)
    draws = []
    orig = torch.randn_like
    # the two Gaussian draws come from a PRIVATE generator (seeded with `seed`) so that a test can
    # regenerate them without depending on what else consumed torch's global RNG (the HF HuBERT twin
    # calls torch.rand([]) per layer for layerdrop even in eval mode)
    gen = torch.Generator().manual_seed(int(seed))

    def cap(x, **kw):
        d = torch.randn(x.shape, generator=gen, dtype=x.dtype)
        draws.append(d.clone())
        return d
    raw = []
    orig_vc = vc.vc

    def vc_cap(*a, **kw):
        r = orig_vc(*a, **kw)
        raw.append(r.copy())
        VC_IN_LENS.append(len(a[3]))          # the audio_pad slice this vc() call got
        return r
    vc.vc = vc_cap
    VC_IN_LENS.clear()
    torch.randn_like = cap
    torch.manual_seed(seed)
    try:
        pcm = vc.pipeline(hub, net, sid, audio.astype(np.float64), "x.wav", pitch, f0_method, file_index, index_rate,
                          1, 3, tgt_sr, 0, volume_envelope, version, protect, 128, None, f0_min, f0_max)
    finally:
        torch.randn_like = orig
    noises = [(draws[2 * i], draws[2 * i + 1]) for i in range(len(draws) // 2)]
    return pcm, raw, noises


def gold_pipeline(tag, cfgs, geo, seconds, clip, seed, pitch, volume_envelope, protect, f0_min, f0_max,
                  full_store=True, fixed_seed=None, version="v2", sid=0):
    """version "v1": the voice model takes final_proj(HuBERT layer 9) -- emb_phone's input width is the HuBERT's final_dim
    (pipeline.py:228-236, infer.py:91-97)"""
    hcfg, rcfg, scfg = cfgs
    in_dim = hcfg["final_dim"] if version == "v1" else hcfg["embed_dim"]
    print(f"[pipeline {tag}] {seconds}s geo={geo} pitch={pitch} env={volume_envelope}")
    a_ = O_pipe.highpass(S.make_clip(clip, seconds).astype(np.float64))
    a_ = np.pad(a_, (16000 * geo[0], 16000 * geo[0]), mode="reflect").astype(np.float32)
    # fixed_seed: found beforehand by tools/find_stable_seed.py (the same criteria, scanned over processes: ~1 % of the
    # seeds qualify on a 9 700-frame clip)
    seed = fixed_seed if fixed_seed is not None else stable_seed(rcfg, a_, seed, f0_min, f0_max, pitch)
    hsd, rsd, ssd = (S.to_torch(S.hubert_state(hcfg, seed)), S.to_torch(S.rmvpe_state(rcfg, seed)),
                     S.to_torch(S.synth_state(scfg, seed, input_dim=in_dim)))
    tgt_sr = scfg[-1]
    audio = S.make_clip(clip, seconds)
    t0 = time.time()
    pcm, raw, noises = run_ref_pipeline(((hcfg, hsd), (rcfg, rsd), (scfg, ssd)), geo, audio, pitch,
                                        volume_envelope, protect, f0_min, f0_max, seed, tgt_sr, version=version, sid=sid)
    t_ref = time.time() - t0
    models = O_pipe.Models(hsd, hcfg, rsd, rcfg, ssd, scfg, version=version)
    t0 = time.time()
    opcm, parts = O_pipe.pipeline(models, O_pipe.Geometry(tgt_sr, *geo), audio, pitch, sid, None, 0.0,
                                  volume_envelope, protect, f0_min, f0_max, noises=noises, return_parts=True)
    t_or = time.time() - t0
    print(f"  chunks={len(raw)}  ref {t_ref:.1f}s  oracle {t_or:.1f}s  out={pcm.shape}")
    e = 0.0
    for i, (a, b) in enumerate(zip(raw, parts["raw"])):
        e = max(e, report(f"vc chunk {i} f32", a, b))
    d = np.abs(pcm.astype(np.int32) - opcm.astype(np.int32))
    print(f"  pcm: max |diff| = {d.max()} LSB, frac>1LSB = {(d > 1).mean():.2e}")
    assert e < 1e-4 and d.max() <= 8, (e, d.max())
    rawcat = np.concatenate(raw)
    store = dict(seed=seed, clip=clip, seconds=seconds, geo=np.array(geo), pitch=pitch, version=version, sid=sid,
                 volume_envelope=volume_envelope, protect=protect, f0_min=f0_min, f0_max=f0_max,
                 cfgs=json.dumps([hcfg, rcfg, scfg]), n_chunks=len(raw),
                 chunk_lens=np.array([len(r) for r in raw]), f0=parts["f0"].astype(np.float32),
                 coarse=parts["coarse"].astype(np.int16),
                 sha256=hashlib.sha256(pcm.tobytes()).hexdigest(),
                 block_rms=np.array([rms(rawcat[i:i + 4096]) for i in range(0, len(rawcat), 4096)], np.float32))
    if full_store:
        store.update(pcm=pcm, raw=rawcat.astype(np.float32))
        for i, (zn, sn) in enumerate(noises):
            store[f"z_noise_{i}"] = zn.numpy()
            store[f"src_noise_{i}"] = sn.numpy()
    else:
        store.update(pcm_samples=pcm[::997], raw_samples=rawcat[::997].astype(np.float32), noise_seed=seed)
    np.savez_compressed(os.path.join(GOLD, f"pipeline_{tag}.npz"), **store)

# ------------------------------------------------------------------ digital silence
def silence_recipe_cuts(clip, seconds, zero_spans, geo):
    """The recipe's input, scipy's filtfilt of it, the reference's opt_ts on that (oracle.chunk_points restates
    pipeline.py:329-344) and the conditioning of every cut window (oracle.pipeline.cut_margins)."""
    audio = S.make_gapped_clip(clip, seconds, zero_spans)
    filt = O_pipe.highpass(audio.astype(np.float64))
    g = O_pipe.Geometry(48000, *geo)
    return audio, filt, [int(t) for t in O_pipe.chunk_points(filt, g)], O_pipe.cut_margins(filt, g)


def gold_pipeline_silence(tag, clip, seconds, zero_spans, geo, volume_envelope, seed=1, silent=False, stride=1,
                          index_centers=0, index_rate=0.75):
    """VC.pipeline on a clip with digital silence (make_gapped_clip: a make_clip index, or -1 for zeros, and the zeroed
    spans), tiny models.  Stores the recipe, the reference's cut points and what gold_pipeline stores.  stride > 1 (long
    clips, 1 MiB per file): the Gaussian draws are left to be regenerated from the private generator's seed, and the float
    waveform is kept at every stride-th sample (block_rms still covers every sample).  index_centers > 0: a retrieval index
    of that many random centres in 8 identical copies each (the top 8 of a query are the copies of its nearest centre, so
    the ids are unambiguous when the nearest centre is: asserted at >= 1e-3 relative distance gap for every query of every
    chunk; one centre lies near the features, the others far out), searched at index_rate -- with the protect mix (0.33) this makes feats0 != feats on unvoiced frames."""
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    print(f"[pipeline {tag}] clip {clip} {seconds}s zeros {zero_spans} geo={geo} env={volume_envelope}")
    audio, filt, cuts, margins = silence_recipe_cuts(clip, seconds, zero_spans, geo)
    # Condition on the input, not a tolerance: every cut window is all exact zeros (every index ties, the first wins), or
    # every index of another frame than the chosen one has |audio_sum| >= 1.01 x the minimum -- a filter that is off by
    # rounding (~1e-8 relative) cannot move the cut to another frame.  A failing window means: move the gap.
    print(f"  cuts {cuts}, window margins {margins}")
    assert all(m is None or m >= 1.01 for m in margins), (tag, margins)
    if silent:
        assert not filt.any() and all(m is None for m in margins), tag
    a_ = np.pad(filt, (16000 * geo[0], 16000 * geo[0]), mode="reflect").astype(np.float32)
    if silent:
        # the RMVPE seed must leave digital silence unvoiced (f0 == 0 on every frame) and well-conditioned
        for k in range(40):
            sd_ = S.to_torch(S.rmvpe_state(rcfg, seed + 100 * k))
            f0_, hid_, _ = O_rmvpe.infer_f0(sd_, rcfg, a_, 0.03, 50, 1100, return_hidden=True)
            if not (f0_ > 0).any() and len(O_rmvpe.unstable_frames(hid_, 0.03, 50, 1100)) == 0:
                seed += 100 * k
                break
        else:
            raise RuntimeError("no seed leaves silence unvoiced")
    else:
        seed = stable_seed(rcfg, a_, seed)
    hsd, rsd, ssd = (S.to_torch(S.hubert_state(hcfg, seed)), S.to_torch(S.rmvpe_state(rcfg, seed)),
                     S.to_torch(S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"])))
    tgt_sr = scfg[-1]
    big, path, irate = None, None, 0.0
    for iseed in range(20 if index_centers else 1):
        if index_centers:
            cen = S.make_index(index_centers, hcfg["embed_dim"], iseed)
            cen[0] *= 0.1                         # one centre near the features, the others 10x farther out
            cen[1:] *= 10.0
            big = np.repeat(cen, 8, axis=0)
            idx = _FlatIndex(big)
            path = os.path.join("/tmp", f"rvcx_{tag}.index")
            open(path, "wb").close()
            _INDEX_FILES[path] = idx
            irate = index_rate
        pcm, raw, noises = run_ref_pipeline(((hcfg, hsd), (rcfg, rsd), (scfg, ssd)), geo, audio, 0, volume_envelope, 0.33,
                                            50, 1100, seed, tgt_sr, file_index=path, index_rate=irate)
        if not index_centers:
            break
        os.remove(path)
        assert len(idx.searches) == len(raw), "the reference did not search the index"
        gap = min(float(np.min((d[:, 8] - d[:, 7]) / d[:, 7])) for d in idx.dists)
        print(f"  index seed {iseed}: smallest relative gap nearest / next centre {gap:.2e}")
        if gap >= 1e-3:
            break
    else:
        raise RuntimeError("no index seed with unambiguous neighbours")
    # the reference's cuts from its own vc() calls: chunk i < last gets audio_pad[s : t + 2 t_pad + 160] with
    # t = opt_ts[i] // 160 * 160 and s the previous t (pipeline.py:381-415)
    t_pad = 16000 * geo[0]
    s_, got = 0, []
    for ln in VC_IN_LENS[:-1]:
        s_ = s_ + ln - 2 * t_pad - 160
        got.append(s_)
    assert len(raw) == len(cuts) + 1 and got == [c // 160 * 160 for c in cuts], (tag, got, cuts)
    assert VC_IN_LENS[-1] == len(audio) + 2 * t_pad - (got[-1] if got else 0), tag
    models = O_pipe.Models(hsd, hcfg, rsd, rcfg, ssd, scfg)
    opcm, parts = O_pipe.pipeline(models, O_pipe.Geometry(tgt_sr, *geo), audio, 0, 0, big, irate, volume_envelope, 0.33,
                                  50, 1100, noises=noises, return_parts=True)
    e = 0.0
    for i, (a, b) in enumerate(zip(raw, parts["raw"])):
        e = max(e, report(f"vc chunk {i} f32", a, b))
    d = np.abs(pcm.astype(np.int32) - opcm.astype(np.int32))
    print(f"  chunks={len(raw)} pcm: max |diff| = {d.max()} LSB; voiced frames {int((parts['f0'] > 0).sum())}/"
          f"{len(parts['f0'])}; pcm peak {np.abs(pcm).max()}")
    assert e < 1e-4 and d.max() <= 8, (e, d.max())
    rawcat = np.concatenate(raw)
    store = dict(seed=seed, clip=clip, seconds=seconds, zero_spans=np.array(zero_spans, np.float64).reshape(-1, 2),
                 cuts=np.array(cuts, np.int64), geo=np.array(geo), pitch=0.0, version="v2", sid=0,
                 volume_envelope=volume_envelope, protect=0.33, f0_min=50, f0_max=1100,
                 cfgs=json.dumps([hcfg, rcfg, scfg]), n_chunks=len(raw), chunk_lens=np.array([len(r) for r in raw]),
                 f0=parts["f0"].astype(np.float32), coarse=parts["coarse"].astype(np.int16),
                 sha256=hashlib.sha256(pcm.tobytes()).hexdigest(),
                 block_rms=np.array([rms(rawcat[i:i + 4096]) for i in range(0, len(rawcat), 4096)], np.float32),
                 pcm=pcm, stride=stride, noise_seed=seed)
    if index_centers:
        store.update(index_rows=big.astype(np.float32), index_rate=irate, index_seed=iseed)
    if stride == 1:
        store["raw"] = rawcat.astype(np.float32)
        for i, (zn, sn) in enumerate(noises):
            store[f"z_noise_{i}"] = zn.numpy()
            store[f"src_noise_{i}"] = sn.numpy()
    else:
        store["raw_samples"] = rawcat[::stride].astype(np.float32)
        gen = torch.Generator().manual_seed(int(seed))       # what tests/test_gpu_silence.py regenerates
        for zn, sn in noises:
            assert torch.equal(torch.randn(zn.shape, generator=gen), zn) and torch.equal(torch.randn(sn.shape, generator=gen), sn)
    np.savez_compressed(os.path.join(GOLD, f"pipeline_{tag}.npz"), **store)


# tag -> recipe (make_gapped_clip's clip index, -1 = zeros, and zeroed spans in seconds) and settings.  The gaps sit under
# every cut window; tests/test_silence_recipes.py re-derives the cuts and the window check from these recipes.
SILENCE_RECIPES = {
    "tiny_silent": dict(clip=-1, seconds=3.0, zero_spans=[], geo=(1, 6, 38, 41), volume_envelope=1.0, silent=True),
    "tiny_silent_env": dict(clip=-1, seconds=3.0, zero_spans=[], geo=(1, 6, 38, 41), volume_envelope=0.25, silent=True),
    "tiny_silent_cut": dict(clip=-1, seconds=7.0, zero_spans=[], geo=(1, 1, 2, 3), volume_envelope=1.0, silent=True),
    "tiny_gap_cut": dict(clip=41, seconds=7.0, zero_spans=[(1.5, 2.5), (3.6, 4.8), (5.4, 6.2)], geo=(1, 1, 2, 3),
                         volume_envelope=1.0),
    # the same clip with the protect mix live: a retrieval index at index_rate 0.75 makes feats0 != feats, and the gaps'
    # unvoiced frames take the blend (pipeline.py:252-262)
    "tiny_gap_cut_index": dict(clip=41, seconds=7.0, zero_spans=[(1.5, 2.5), (3.6, 4.8), (5.4, 6.2)], geo=(1, 1, 2, 3),
                               volume_envelope=1.0, index_centers=4),
    "tiny_lead_trail": dict(clip=44, seconds=3.6, zero_spans=[(0.0, 0.6), (3.0, 3.6)], geo=(1, 1, 2, 3),
                            volume_envelope=0.25),
    "gap_real_geo": dict(clip=47, seconds=45.0, zero_spans=[(36.0, 37.5)], geo=(1, 6, 38, 41), volume_envelope=1.0,
                         stride=3),
}


# ------------------------------------------------------------------ FCPE
def fcpe_file(cfg, seed):
    """fcpe.pt as FCPEInfer.__init__ reads it (FCPE.py:708-736), with synthetic weights, in a scratch directory;
    the reference's VC.get_f0 opens the module constant FCPE_DIR (pipeline.py:16,170-171), pointed there."""
    ck = S.fcpe_checkpoint(cfg, seed)
    ck["model"] = S.to_torch(ck["model"])
    path = os.path.join("/tmp", f"fcpe_{cfg['n_layers']}x{cfg['n_chans']}_{seed}.pt")
    torch.save(ck, path)
    P.FCPE_DIR = path
    return path, ck["model"]


def fcpe_stable_seed(cfg, x, seed, pitch=0.0, f0_min=50, f0_max=1100, tries=40, min_margin=2e-3):
    """First seed >= `seed` (step 100) whose voiced / unvoiced decisions (salience maximum vs the 0.03 threshold)
    and coarse quantisation are all well-conditioned."""
    mel = O_fcpe.mel_spectrogram(torch.from_numpy(x)[None])
    for k in range(tries):
        sd = S.to_torch(S.fcpe_state(cfg, seed + 100 * k))
        sal = O_fcpe.salience(sd, mel)[0]
        conf = sal.max(-1).values.numpy()
        margin = np.abs(conf - 0.03).min() / 0.03
        f0 = O_fcpe.compute_f0(sd, x, len(x) // 160)
        _, q = O_pipe.f0_to_coarse(f0, pitch, f0_min, f0_max)
        f0m = 1127 * np.log(1 + q / 700)
        m0, m1 = 1127 * np.log(1 + f0_min / 700), 1127 * np.log(1 + f0_max / 700)
        qq = (f0m - m0) * 254 / (m1 - m0) + 1
        tie = (q > 0) & (np.abs(qq - np.floor(qq) - 0.5) < 1e-3)
        vf = (conf > 0.03).mean()
        print(f"  seed {seed + 100 * k}: threshold margin {margin:.2e}, coarse ties {int(tie.sum())}, voiced {vf:.2f}")
        if margin > min_margin and not tie.any() and 0.15 < vf < 0.95:
            return seed + 100 * k
    raise RuntimeError("no stable fcpe seed found")


def gold_fcpe(tag, cfg, seconds, clip, seed, pitch, stride=1):
    """FCPE stage by stage against the reference's own module, through the reference's own call site VC.get_f0."""
    print(f"[fcpe {tag}] {seconds}s pitch={pitch}")
    a_ = O_pipe.highpass(S.make_clip(clip, seconds).astype(np.float64))
    x = np.pad(a_, (16000, 16000), mode="reflect").astype(np.float32)       # audio_pad, pipeline.py:357
    p_len = len(x) // 160
    seed = fcpe_stable_seed(cfg, x, seed, pitch)
    path, sd = fcpe_file(cfg, seed)
    pred = RF.FCPEF0Predictor(path, f0_min=50, f0_max=1100, dtype=torch.float32, device="cpu", sample_rate=16000,
                              threshold=0.03)
    xt = torch.from_numpy(x)
    mel = pred.fcpe.wav2mel(audio=xt[None], sample_rate=16000)               # (1, F, 128)
    m = pred.fcpe.model
    h = m.stack(mel.transpose(1, 2)).transpose(1, 2)
    sal = torch.sigmoid(m.dense_out(m.norm(m.decoder(h))))[0]                # FCPE.forward up to :646
    raw = pred.fcpe(xt, sr=16000, threshold=0.03)[0, :, 0].numpy()
    vc = P.VC(48000, Cfg((1, 6, 38, 41)))
    coarse, f0bak = vc.get_f0("x.wav", x, p_len, pitch, "fcpe", 3, 128, None, 50, 1100)
    o_mel = O_fcpe.mel_spectrogram(xt[None])
    o_sal = O_fcpe.salience(sd, o_mel)[0]
    o_raw = O_fcpe.infer_hz(sd, x, 0.03)
    o_coarse, o_f0 = O_pipe.f0_to_coarse(O_fcpe.compute_f0(sd, x, p_len), pitch, 50, 1100)
    report("mel", mel, o_mel); e1 = report("salience", sal, o_sal); e2 = report("raw f0", raw, o_raw)
    e3 = report("get_f0 f0", f0bak, o_f0)
    print(f"  voiced {int((raw > 0).sum())}/{len(raw)}; coarse differs at {int((coarse != o_coarse).sum())} frames")
    assert e1 < 1e-5 and e2 < 1e-2 and e3 < 1e-2 and (coarse == o_coarse).all(), (e1, e2, e3)
    np.savez_compressed(os.path.join(GOLD, f"fcpe_{tag}.npz"), seed=seed, cfg=json.dumps(cfg), clip=clip,
                        seconds=seconds, pitch=pitch, x=x, mel=mel[0].numpy().T[:, ::stride],
                        salience=sal.numpy()[::stride], raw_f0=raw, f0=f0bak.astype(np.float64),
                        coarse=coarse.astype(np.int16), stride=stride)


def gold_pipeline_fcpe(tag, cfgs, fcfg, geo, seconds, clip, seed, pitch, volume_envelope, protect, full_store=True,
                       min_margin=2e-3):
    """VC.pipeline(..., f0_method="fcpe") end to end (pipeline.py:169-181 inside :362-380)."""
    hcfg, rcfg, scfg = cfgs
    print(f"[pipeline {tag}] fcpe {seconds}s geo={geo} pitch={pitch}")
    a_ = O_pipe.highpass(S.make_clip(clip, seconds).astype(np.float64))
    a_ = np.pad(a_, (16000 * geo[0], 16000 * geo[0]), mode="reflect").astype(np.float32)
    seed = fcpe_stable_seed(fcfg, a_, seed, pitch, min_margin=min_margin)
    path, fsd = fcpe_file(fcfg, seed)
    hsd, ssd = S.to_torch(S.hubert_state(hcfg, seed)), S.to_torch(S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"]))
    tgt_sr = scfg[-1]
    audio = S.make_clip(clip, seconds)
    pcm, raw, noises = run_ref_pipeline(((hcfg, hsd), (rcfg, None), (scfg, ssd)), geo, audio, pitch, volume_envelope,
                                        protect, 50, 1100, seed, tgt_sr, f0_method="fcpe",
                                        prebuilt=(None, HubertAdapter(hf_hubert(hcfg, hsd))))
    models = O_pipe.Models(hsd, hcfg, None, rcfg, ssd, scfg, fcpe_sd=fsd)
    opcm, parts = O_pipe.pipeline(models, O_pipe.Geometry(tgt_sr, *geo), audio, pitch, 0, None, 0.0, volume_envelope,
                                  protect, 50, 1100, noises=noises, return_parts=True, f0_method="fcpe")
    e = 0.0
    for i, (a, b) in enumerate(zip(raw, parts["raw"])):
        e = max(e, report(f"vc chunk {i} f32", a, b))
    d = np.abs(pcm.astype(np.int32) - opcm.astype(np.int32))
    print(f"  chunks={len(raw)} pcm: max |diff| = {d.max()} LSB, frac>1LSB = {(d > 1).mean():.2e}")
    assert e < 1e-4 and d.max() <= 8, (e, d.max())
    rawcat = np.concatenate(raw)
    store = dict(seed=seed, clip=clip, seconds=seconds, geo=np.array(geo), pitch=pitch, version=version, sid=sid, volume_envelope=volume_envelope,
                 protect=protect, f0_min=50, f0_max=1100, cfgs=json.dumps([hcfg, fcfg, scfg]), n_chunks=len(raw),
                 chunk_lens=np.array([len(r) for r in raw]), f0=parts["f0"].astype(np.float32),
                 coarse=parts["coarse"].astype(np.int16), sha256=hashlib.sha256(pcm.tobytes()).hexdigest(),
                 block_rms=np.array([rms(rawcat[i:i + 4096]) for i in range(0, len(rawcat), 4096)], np.float32))
    if full_store:
        store.update(pcm=pcm, raw=rawcat.astype(np.float32))
        for i, (zn, sn) in enumerate(noises):
            store[f"z_noise_{i}"] = zn.numpy()
            store[f"src_noise_{i}"] = sn.numpy()
    else:
        store.update(pcm_samples=pcm[::997], raw_samples=rawcat[::997].astype(np.float32), noise_seed=seed)
    np.savez_compressed(os.path.join(GOLD, f"pipeline_{tag}.npz"), **store)


def _full_store(pcm, raw, parts, stride):
    rawcat = np.concatenate(raw)
    return dict(n_chunks=len(raw), chunk_lens=np.array([len(r) for r in raw]), f0=parts["f0"].astype(np.float32),
                coarse=parts["coarse"].astype(np.int16), sha256=hashlib.sha256(pcm.tobytes()).hexdigest(),
                block_rms=np.array([rms(rawcat[i:i + 4096]) for i in range(0, len(rawcat), 4096)], np.float32),
                pcm_samples=pcm[::stride], raw_samples=rawcat[::stride].astype(np.float32), stride=stride)


def gold_pipeline_c3(tag="c3_30s_48k_index", seconds=30.0, clip=0, seed=1900, n_rows=65536, index_rate=0.75):
    """BASELINE configs[2] for one utterance of the batch: full-size models, retrieval blend at index_rate 0.75 over
    a 65 536 x 768 index (S.make_index_from_feats of the reference-side HuBERT features: unambiguous neighbours).
    The reference's own VC.vc blend code runs; only faiss' search is the exact-L2 stand-in above."""
    cfgs = (S.HUBERT_CFG_BASE, S.RMVPE_CFG_FULL, S.SYNTH_CFG_48K)
    hcfg, rcfg, scfg = cfgs
    geo = (1, 6, 38, 41)
    print(f"[pipeline {tag}] {seconds}s index {n_rows}x768 rate {index_rate}")
    audio = S.make_clip(clip, seconds)
    a_ = np.pad(O_pipe.highpass(audio.astype(np.float64)), (16000, 16000), mode="reflect").astype(np.float32)
    assert stable_seed(rcfg, a_, seed) == seed
    hsd, rsd, ssd = (S.to_torch(S.hubert_state(hcfg, seed)), S.to_torch(S.rmvpe_state(rcfg, seed)),
                     S.to_torch(S.synth_state(scfg, seed)))
    hub = HubertAdapter(hf_hubert(hcfg, hsd))
    feats = hub.extract_features(torch.from_numpy(a_)[None], None, 12)[0][0].numpy()
    big = S.make_index_from_feats(feats, n_rows, 0)
    idx = _FlatIndex(big)
    path = os.path.join("/tmp", f"rvcx_{tag}.index")
    open(path, "wb").close()
    _INDEX_FILES[path] = idx
    t0 = time.time()
    pcm, raw, noises = run_ref_pipeline(((hcfg, hsd), (rcfg, rsd), (scfg, ssd)), geo, audio, 0, 1.0, 0.33, 50, 1100,
                                        seed, 48000, file_index=path, index_rate=index_rate,
                                        prebuilt=(ref_rmvpe(rcfg, rsd), hub))
    t_ref = time.time() - t0
    assert len(idx.searches) == 1, "the reference did not search the index"
    models = O_pipe.Models(hsd, hcfg, rsd, rcfg, ssd, scfg)
    opcm, parts = O_pipe.pipeline(models, O_pipe.Geometry(48000, *geo), audio, 0, 0, big, index_rate, 1.0, 0.33, 50,
                                  1100, noises=noises, return_parts=True)
    e = report("vc chunk f32 (ref vs oracle)", raw[0], parts["raw"][0])
    d = np.abs(pcm.astype(np.int32) - opcm.astype(np.int32))
    print(f"  ref {t_ref:.1f}s  pcm max |diff| {d.max()} LSB")
    assert e < 1e-4 and d.max() <= 8
    # the same run without the index must differ: the blend is live in the fixture
    store = dict(seed=seed, clip=clip, seconds=seconds, geo=np.array(geo), pitch=0, volume_envelope=1.0, protect=0.33,
                 f0_min=50, f0_max=1100, cfgs=json.dumps([hcfg, rcfg, scfg]), noise_seed=seed, index_rate=index_rate,
                 index_rows=n_rows, ids_sha256=hashlib.sha256(idx.searches[0].astype(np.int64).tobytes()).hexdigest(),
                 ids_head=idx.searches[0][:16].astype(np.int64))
    store.update(_full_store(pcm, raw, parts, 997))
    np.savez_compressed(os.path.join(GOLD, f"pipeline_{tag}.npz"), **store)
    os.remove(path)


def gold_pipeline_c5(tag="c5_two_models", seed0=2500):
    """BASELINE configs[4] in small: two resident voice models (40 k and 48 k, full size) sharing ONE HuBERT and
    ONE RMVPE, utterances of different lengths -- the reference's VC.pipeline output per (utterance, model)."""
    hcfg, rcfg = S.HUBERT_CFG_BASE, S.RMVPE_CFG_FULL
    geo = (1, 6, 38, 41)
    jobs = [(30, 4.2, S.SYNTH_CFG_40K), (31, 6.1, S.SYNTH_CFG_48K), (32, 3.3, S.SYNTH_CFG_48K)]
    pads = [np.pad(O_pipe.highpass(S.make_clip(c, sec).astype(np.float64)), (16000, 16000), mode="reflect")
            .astype(np.float32) for c, sec, _ in jobs]
    seed = seed0
    for _ in range(200):                              # one RMVPE seed that is well-conditioned on every utterance
        if all(stable_seed(rcfg, a_, seed, tries=1) == seed for a_ in pads):
            break
        seed += 100
    else:
        raise RuntimeError("no common stable seed")
    print(f"[pipeline {tag}] shared HuBERT/RMVPE seed {seed}")
    hsd, rsd = S.to_torch(S.hubert_state(hcfg, seed)), S.to_torch(S.rmvpe_state(rcfg, seed))
    pre = (ref_rmvpe(rcfg, rsd), HubertAdapter(hf_hubert(hcfg, hsd)))
    store = dict(seed=seed, geo=np.array(geo), n_utts=len(jobs), hcfg=json.dumps(hcfg), rcfg=json.dumps(rcfg))
    for u, (clip, sec, scfg) in enumerate(jobs):
        sseed = seed + (3 if scfg is S.SYNTH_CFG_40K else 7)
        ssd = S.to_torch(S.synth_state(scfg, sseed))
        audio = S.make_clip(clip, sec)
        nseed = seed + 11 * (u + 1)
        pcm, raw, noises = run_ref_pipeline(((hcfg, hsd), (rcfg, rsd), (scfg, ssd)), geo, audio, 0, 1.0, 0.33, 50,
                                            1100, nseed, scfg[-1], prebuilt=pre)
        models = O_pipe.Models(hsd, hcfg, rsd, rcfg, ssd, scfg)
        opcm, parts = O_pipe.pipeline(models, O_pipe.Geometry(scfg[-1], *geo), audio, 0, 0, None, 0.0, 1.0, 0.33, 50,
                                      1100, noises=noises, return_parts=True)
        e = report(f"utt {u} vc f32 (ref vs oracle)", raw[0], parts["raw"][0])
        assert e < 1e-4
        st = _full_store(pcm, raw, parts, 97)
        st.update(clip=clip, seconds=sec, scfg=json.dumps(scfg), synth_seed=sseed, noise_seed=nseed)
        for k, v in st.items():
            store[f"u{u}_{k}"] = v
    np.savez_compressed(os.path.join(GOLD, f"pipeline_{tag}.npz"), **store)


def gold_layouts():
    """Key/shape listings of the reference's own modules (the checkpoint contracts)."""
    out = {}
    net = Synthesizer(*S.SYNTH_CFG_48K, use_f0=1, input_dim=768, is_half=False)
    del net.enc_q
    out["synth_48k"] = {k: list(v.shape) for k, v in net.state_dict().items()}
    m = R.E2E(4, 1, (2, 2))
    out["rmvpe"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    with open(os.path.join(GOLD, "layouts.json"), "w") as f:
        json.dump(out, f)
    mine = S.synth_state(S.SYNTH_CFG_48K)
    assert set(mine) == set(out["synth_48k"]), set(mine) ^ set(out["synth_48k"])
    for k, v in mine.items():
        assert list(v.shape) == out["synth_48k"][k], k
    mine = S.rmvpe_state(S.RMVPE_CFG_FULL)
    assert set(mine) == set(out["rmvpe"]), set(mine) ^ set(out["rmvpe"])
    for k, v in mine.items():
        assert list(v.shape) == out["rmvpe"][k], (k, v.shape, out["rmvpe"][k])
    print("[layouts] synthetic layouts == reference module layouts "
          f"(synth {len(out['synth_48k'])} tensors, rmvpe {len(out['rmvpe'])} tensors)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="also run the full-size C1/C2 pipelines (minutes)")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    tiny = (S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY)
    steps = {
        "layouts": gold_layouts,
        "synth_tiny": lambda: gold_synth("tiny", S.SYNTH_CFG_TINY, 37, 1),
        "synth_48k": lambda: gold_synth("48k_T24", S.SYNTH_CFG_48K, 24, 0),
        # Synthesizer.infer's `rate` (live streams): head = int(T * (1 - float32(rate))) -- 40 * (1 - 0.3f) is 27, not 28
        "synth_head_h30": lambda: gold_synth_head("tiny_h30", S.SYNTH_CFG_TINY, 40, 3, 0.25),
        "synth_head_h27": lambda: gold_synth_head("tiny_h27", S.SYNTH_CFG_TINY, 40, 3, 0.3),
        "synth_head_48k": lambda: gold_synth_head("48k_h15", S.SYNTH_CFG_48K, 24, 0, 0.375),
        "rmvpe_tiny": lambda: gold_rmvpe("tiny", S.RMVPE_CFG_TINY, 0.7, 1),
        "rmvpe_full": lambda: gold_rmvpe("full_1s", S.RMVPE_CFG_FULL, 1.0, 0),
        "rmvpe_illcond": gold_rmvpe_illcond,
        # round 6: planted outlier channels in the NSF decoder (weight-norm g spread 1 : 150, c1 -> c2 hand-off values of a
        # few hundred) and in the F0 U-Net (BatchNorm scale x 150 on the block-internal hand-off): synthetic.py
        "synth_outliers": lambda: gold_synth("48k_T24_outliers", S.SYNTH_CFG_48K, 24, 0, outliers=True),
        "rmvpe_outliers": lambda: gold_rmvpe("full_1s_outliers", S.RMVPE_CFG_FULL, 1.0, 0, outliers=True),
        "hubert_tiny": lambda: gold_hubert("tiny", S.HUBERT_CFG_TINY, 0.5, 1),
        "hubert_base": lambda: gold_hubert("base_1s", S.HUBERT_CFG_BASE, 1.0, 0),
        # the same model with planted outlier units (synthetic.py: _plant_outliers): what real ContentVec-shaped weights do
        "hubert_outliers": lambda: gold_hubert("base_1s_outliers", S.HUBERT_CFG_BASE, 1.0, 0, outliers=True),
        "pipe_tiny": lambda: gold_pipeline("tiny_single", tiny, (1, 6, 38, 41), 2.0, 11, 1, 0, 1.0, 0.33, 50, 1100),
        # CI's canonical argument set (test_cli.yml:43): -p -0.5 -rms 0.25 -pro 0.33 -f0min 1 -f0max 1100
        "pipe_tiny_ci": lambda: gold_pipeline("tiny_ciargs", tiny, (1, 6, 38, 41), 2.5, 12, 1, -0.5, 0.25, 0.33, 1, 1100),
        # a clip SHORTER than the 1 s reflect padding: np.pad reflects repeatedly (pipeline.py:348 on 0.4 s of audio)
        "pipe_tiny_short": lambda: gold_pipeline("tiny_short", tiny, (1, 6, 38, 41), 0.4, 15, 1, 0, 1.0, 0.33, 50, 1100),
        # small geometry to force the multi-chunk branch (pipeline.py:381-415)
        "fcpe_tiny": lambda: gold_fcpe("tiny", S.FCPE_CFG_TINY, 1.2, 21, 1, 0.0),
        "fcpe_full": lambda: gold_fcpe("full_2s", S.FCPE_CFG_FULL, 2.0, 22, 0, -3.0, stride=2),
        "pipe_fcpe_tiny": lambda: gold_pipeline_fcpe("tiny_fcpe", tiny, S.FCPE_CFG_TINY, (1, 6, 38, 41), 2.0, 14, 1, 1.0, 1.0, 0.33),
        "pipe_tiny_chunks": lambda: gold_pipeline("tiny_chunked", tiny, (1, 1, 2, 3), 7.3, 13, 1, 2, 1.0, 0.33, 50, 1100),
        # round 6: an RVC v1 voice model (HuBERT output layer 9 + final_proj, emb_phone on final_dim features)
        # round 6: a speaker id other than 0 (row 3 of emb_g) and the protect mix switched off (protect >= 0.5, pipeline.py:252-262)
        "pipe_tiny_sid": lambda: gold_pipeline("tiny_sid3_noprotect", tiny, (1, 6, 38, 41), 2.1, 17, 1, 1.5, 0.6, 0.5, 50, 1100, sid=3),
        "pipe_tiny_v1": lambda: gold_pipeline("tiny_v1", tiny, (1, 6, 38, 41), 2.2, 16, 1, 0, 1.0, 0.33, 50, 1100, version="v1"),
        # digital silence (SILENCE_RECIPES): zero clips, zero gaps under the cut windows, zero ends
        **{f"pipe_{tag}": (lambda tag=tag: gold_pipeline_silence(tag, **SILENCE_RECIPES[tag])) for tag in SILENCE_RECIPES},
    }
    if a.full:
        full40 = (S.HUBERT_CFG_BASE, S.RMVPE_CFG_FULL, S.SYNTH_CFG_40K)
        full48 = (S.HUBERT_CFG_BASE, S.RMVPE_CFG_FULL, S.SYNTH_CFG_48K)
        steps["pipe_c1"] = lambda: gold_pipeline("c1_5s_40k", full40, (1, 6, 38, 41), 5.0, 0, 0, 0, 1.0, 0.33,
                                                 50, 1100, full_store=False)
        steps["pipe_c2"] = lambda: gold_pipeline("c2_30s_48k", full48, (1, 6, 38, 41), 30.0, 0, 0, 0, 1.0, 0.33,
                                                 50, 1100, full_store=False)
        steps["pipe_fcpe_c2"] = lambda: gold_pipeline_fcpe("c2_30s_48k_fcpe", full48, S.FCPE_CFG_FULL, (1, 6, 38, 41), 30.0,
                                                           0, 2100, 0, 1.0, 0.33, full_store=False,
                                                           min_margin=2e-4)   # 3200 frames: the salience
        # maximum of some frame always comes within ~1e-4 of the 0.03 threshold; 2e-4 is ~30x the GPU's error
        # round 6: the cut-point / per-chunk / trim / concat branch (pipeline.py:330-344,381-447) at the REAL geometry and
        # model size: a 95 s clip is cut into three chunks at silence-aligned points, F0 once over 9 700 frames
        # seed 12800: `tools/find_stable_seed.py --start 7000 --n 200 --rel 2e-4 --tie-margin 5e-4` (no ill-conditioned frame,
        # no coarse value within 5e-4 of a rounding tie -- 7x the error bound of an f0 that is 1e-6 off)
        steps["pipe_long95"] = lambda: gold_pipeline("long95_48k", full48, (1, 6, 38, 41), 95.0, 3, 3000, 0, 1.0, 0.33,
                                                     50, 1100, full_store=False,
                                                     fixed_seed=int(os.environ.get("RVCX_LONG95_SEED", "12800")))
        # an RVC v1 voice model at full size: HuBERT-base layer 9 (not 12) + final_proj 768 -> 256, 40 k synthesizer on 256 features
        steps["pipe_v1_full"] = lambda: gold_pipeline("v1_5s_40k", full40, (1, 6, 38, 41), 5.0, 4, 0, 0, 1.0, 0.33,
                                                      50, 1100, full_store=False, version="v1")
        # round 6: the third geometry RVC v2 ships (32 k: upsample rates 10 x 8 x 2 x 2, kernels 20 / 16 / 4 / 4 -- a stride-8
        # ConvTranspose1d, noise convs of 64 / 8 / 4 / 1 taps, upp = 320)
        full32 = (S.HUBERT_CFG_BASE, S.RMVPE_CFG_FULL, S.SYNTH_CFG_32K)
        steps["pipe_32k"] = lambda: gold_pipeline("v2_4s_32k", full32, (1, 6, 38, 41), 4.0, 5, 0, 0, 1.0, 0.33,
                                                  50, 1100, full_store=False)
        steps["pipe_c3"] = gold_pipeline_c3
        steps["pipe_c5"] = gold_pipeline_c5
    for k, fn in steps.items():
        if a.only and a.only not in k:
            continue
        fn()


if __name__ == "__main__":
    main()
