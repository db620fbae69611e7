"""Conversion tickets (rvcx_convert_submit / _wait / _poll / _inflight, rvcx_ticket_lead_ms; Context.convert_submit,
VC.pipeline_async / pipeline_stream, rvc_infer_many): two requests in flight per context.

The contract under test is EQUALITY: what a ticket writes is byte for byte what the synchronous call writes for the same
arguments (np.array_equal on PCM, float waveform, sample counts and cut points), whatever is in flight beside it, in
whatever order the tickets are waited for, and across the range guard's and the BiGRU fallback's repeats.  The goldens
(the reference's own VC.pipeline output) are met with the existing bars of conftest.  `lead_ms > 0` at full size shows that
the second ticket's front end really started before the first had finished (a renamed synchronous call fails it)."""
import gc
import json
import os
import threading

import numpy as np
import pytest
import torch

from conftest import FULL_PCM_BAR, FULL_RMS_BAR, TINY_RMS_BAR, rms

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(ctx, seed, synth_cfgs):
    from polgen_rvc_amd import synthetic as S, weights as W
    hcfg, rcfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, seed))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, seed))
    mids = []
    for i, scfg in enumerate(synth_cfgs):
        st = S.synth_state(scfg, seed + 10 * i, input_dim=hcfg["embed_dim"])
        mids.append(ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), st))
    return mids


def _params(index_rate=0.0, protect=0.33, seed=5, volume_envelope=1.0, geo=(1, 1, 2, 3), f0_method=0):
    from polgen_rvc_amd import _lib
    p = _lib.Params(0.0, 50.0, 1100.0, index_rate, protect, volume_envelope, 0, geo[0], geo[1], geo[2], geo[3], seed)
    p.f0_method = f0_method
    return p


def _same(a, b):
    """two convert_batch-shaped results ((pcm list, f32 list)) are equal bit for bit"""
    (pa, fa), (pb, fb) = a, b
    assert [len(x) for x in pa] == [len(x) for x in pb]
    for x, y in zip(pa, pb):
        assert x.dtype == np.int16 and np.array_equal(x, y)
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)


def _pack_noise(d):
    parts = []
    for i in range(int(d["n_chunks"])):
        parts += [d[f"z_noise_{i}"].ravel(), d[f"src_noise_{i}"].ravel()]
    return np.concatenate(parts).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. one ticket = the call
def test_one_ticket_equals_the_call(ctx):
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    (mid,) = _load(ctx, 3, [S.SYNTH_CFG_TINY])
    fc = S.FCPE_CFG_TINY
    sd = S.fcpe_state(fc, 3)
    ctx.load_fcpe(W.fcpe_cfg_struct(W.fcpe_cfg_from_state(sd)), sd)
    d = np.load(os.path.join(GOLD, "pipeline_tiny_chunked.npz"))
    table = np.array([[0.0, 110.0], [0.5, 220.0], [1.0, 180.0], [1.6, 140.0]], np.float32)
    cases = {
        "short": dict(wavs=[S.make_clip(40, 1.3)], p=_params()),
        "cut": dict(wavs=[S.make_clip(41, 5.3)], p=_params()),
        "f0_file": dict(wavs=[S.make_clip(43, 2.0)], p=_params(), inp_f0=[table]),
        "fcpe": dict(wavs=[S.make_clip(44, 2.1)], p=_params(f0_method=_lib.F0_FCPE)),
        "parity_noise": dict(wavs=[S.make_clip(int(d["clip"]), float(d["seconds"])).astype(np.float64)],
                             p=_params(geo=[int(v) for v in d["geo"]], protect=float(d["protect"]),
                                       volume_envelope=float(d["volume_envelope"])), noises=[_pack_noise(d)]),
    }
    for name, c in cases.items():
        kw = {k: v for k, v in c.items() if k not in ("wavs", "p")}
        want = ctx.convert_batch(mid, c["wavs"], c["p"], want_f32=True, **kw)
        cuts, mbs = ctx.last_cuts(), ctx.last_micro_batches()
        t = ctx.convert_submit(mid, c["wavs"], c["p"], want_f32=True, **kw)
        got = t.wait()
        _same(want, got)
        assert ctx.last_cuts() == cuts and ctx.last_micro_batches() == mbs, name
        assert t.lead_ms == 0.0, name               # submitted into an idle context
        if name == "cut":
            assert len(cuts[0]) >= 1
    # a ragged ticket of three clips with the retrieval blend, protect and the RMS envelope
    ctx.load_index(S.make_index(2048, S.HUBERT_CFG_TINY["embed_dim"], 1))
    try:
        clips = [S.make_clip(40, 1.7), S.make_clip(41, 5.3), S.make_clip(42, 2.9)]
        p = _params(index_rate=0.75, protect=0.33, volume_envelope=0.25)
        want = ctx.convert_batch(mid, clips, p, want_f32=True)
        cuts, mbs = ctx.last_cuts(), ctx.last_micro_batches()
        got = ctx.convert_submit(mid, clips, p, want_f32=True).wait()
        _same(want, got)
        assert ctx.last_cuts() == cuts and ctx.last_micro_batches() == mbs
    finally:
        ctx.load_index(None)


# ---------------------------------------------------------------------------------------------- 2. a stream
def test_a_stream_of_tickets_in_submit_order_and_in_reverse_pairs(ctx):
    from polgen_rvc_amd import synthetic as S
    (mid,) = _load(ctx, 4, [S.SYNTH_CFG_TINY])
    secs = [1.2, 2.9, 5.3, 1.7, 2.9, 0.9, 3.0, 2.2]          # one cut (5.3 s at x_max = 3), two equal
    clips = [S.make_clip(70 + i, s) for i, s in enumerate(secs)]
    p = _params(seed=9)
    want = [ctx.convert_batch(mid, [c], p, want_f32=True) for c in clips]      # a one-clip ticket draws from Philox(seed + 0)
    # waited for in submit order, two in flight
    got, pending = [], []
    for c in clips:
        pending.append(ctx.convert_submit(mid, [c], p, want_f32=True))
        assert ctx.convert_inflight() <= 2
        if len(pending) == 2:
            got.append(pending.pop(0).wait())
    got += [t.wait() for t in pending]
    for w, g in zip(want, got):
        _same(w, g)
    # each pair waited for in reverse order
    for i in range(0, len(clips), 2):
        t0 = ctx.convert_submit(mid, [clips[i]], p, want_f32=True)
        t1 = ctx.convert_submit(mid, [clips[i + 1]], p, want_f32=True)
        g1 = t1.wait()
        assert t0.done()                   # completions settle in submit order
        g0 = t0.wait()
        _same(want[i], g0)
        _same(want[i + 1], g1)


# ---------------------------------------------------------------------------------------------- 3. against the reference
def _setup(ctx, cfgs, seed):
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.infer import infer as I
    hcfg, rcfg, scfg = cfgs
    I._CTX[0] = ctx
    hub = I.load_hubert("cuda:0", False, None, state=S.hubert_state(hcfg, seed), cfg=hcfg)
    I.load_rmvpe("cuda:0", state=S.rmvpe_state(rcfg, seed), cfg=rcfg)
    cpt = S.synth_checkpoint(scfg, seed)
    cpt["weight"] = S.synth_state(scfg, seed, input_dim=hcfg["embed_dim"])
    return hub, cpt


@pytest.mark.parametrize("tag", ["tiny_chunked", "tiny_silent_cut", "tiny_ciargs"])
def test_pipeline_async_vs_reference_goldens_two_in_flight(ctx, tag):
    """The goldens are the reference's own VC.pipeline output.  Each golden has model weights of its own (its seed), and a
    context holds one HuBERT, so the two conversions in flight are two submissions of the golden's request; both are held
    to the golden with the existing bars."""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.infer import infer as I
    d = np.load(os.path.join(GOLD, f"pipeline_{tag}.npz"))
    hub, cpt = _setup(ctx, json.loads(str(d["cfgs"])), int(d["seed"]))
    cfg = I.Config()
    cfg.x_pad, cfg.x_query, cfg.x_center, cfg.x_max = [int(v) for v in d["geo"]]
    _, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, cfg, None, cpt=cpt)
    if "zero_spans" in d.files:
        audio = S.make_gapped_clip(int(d["clip"]), float(d["seconds"]), [tuple(s) for s in d["zero_spans"]])
    else:
        audio = S.make_clip(int(d["clip"]), float(d["seconds"]))
    hs = [vc.pipeline_async(hub, net_g, 0, audio.astype(np.float64), "x.wav", float(d["pitch"]), "rmvpe+", None, 0, 1, 3,
                            tgt_sr, 0, float(d["volume_envelope"]), "v2", float(d["protect"]), 128, None,
                            float(d["f0_min"]), float(d["f0_max"]), noise=_pack_noise(d), return_f32=True)
          for _ in range(2)]
    assert ctx.convert_inflight() <= 2
    for h in hs:
        _check_tiny(tag, d, tgt_sr, h)
    if "cuts" in d.files:
        assert ctx.last_cuts() == [d["cuts"].tolist()]


def _check_tiny(tag, d, tgt_sr, h):
    pcm, f32 = h.result()
    ref = d["pcm"]
    assert pcm.shape == ref.shape, (tag, pcm.shape, ref.shape)
    diff = np.abs(pcm.astype(np.int32) - ref.astype(np.int32))
    print(f"{tag}: pcm max diff {diff.max()} LSB, frac>1 {np.mean(diff > 1):.2e}")
    assert diff.max() <= 4 and np.mean(diff > 1) < 0.02, f"{tag}: pcm max diff {diff.max()} LSB"
    if float(d["volume_envelope"]) == 1.0:
        tp = int(tgt_sr) * int(d["geo"][0])
        lens = [int(v) for v in d["chunk_lens"]]
        offs = np.concatenate([[0], np.cumsum(lens)])
        ref_f32 = np.concatenate([d["raw"][offs[i] + tp: offs[i + 1] - tp] for i in range(len(lens))])
        e = rms(f32 - ref_f32)
        print(f"{tag}: float rms err {e:.3e}")
        assert e < TINY_RMS_BAR, f"{tag}: float rms err {e:.3e}"


def test_full_size_c2_twice_in_flight_overlaps(ctx):
    """The C2 golden (30 s, v2 48 k, full-size models) twice in flight: both against the golden with the full-size bars,
    both byte-equal to VC.pipeline, and the second ticket's front end starts before the first has finished (lead_ms > 0).
    The first ticket has ~24 ms of device work queued when the second is submitted and enqueueing a clip takes a few ms
    of host time, so the sign is not a timing bar.  One pair goes first so that every arena has its size for this shape
    (the first request of a new shape may have to complete what is in flight before memory grows); the sign is asserted on
    the very next pair."""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.infer import infer as I
    d = np.load(os.path.join(GOLD, "pipeline_c2_30s_48k.npz"))
    cfgs = json.loads(str(d["cfgs"]))
    hub, cpt = _setup(ctx, cfgs, int(d["seed"]))
    cpt, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, I.Config(), None, cpt=cpt)
    audio = S.make_clip(int(d["clip"]), float(d["seconds"]))
    T = int(d["chunk_lens"][0]) // (tgt_sr // 100)
    gen = torch.Generator().manual_seed(int(d["noise_seed"]))
    z = torch.randn((1, cfgs[2][2], T), generator=gen)
    src = torch.randn((1, T * (tgt_sr // 100), 1), generator=gen)
    noise = np.concatenate([z.numpy().ravel(), src.numpy().ravel()])
    args = (hub, net_g, 0, audio, "x.wav", 0.0, "rmvpe+", None, 0, 1, 3, tgt_sr, 0, 1.0, "v2", 0.33, 128, None, 50, 1100)
    want_pcm, want_f32 = vc.pipeline(*args, noise=noise, return_f32=True)
    leads = []
    for _ in range(2):                      # the warm-up pair, then the asserted one
        h0 = vc.pipeline_async(*args, noise=noise, return_f32=True)
        h1 = vc.pipeline_async(*args, noise=noise, return_f32=True)
        r0, r1 = h0.result(), h1.result()
        for pcm, f32 in (r0, r1):
            assert np.array_equal(pcm, want_pcm) and np.array_equal(f32, want_f32)
        assert h0.lead_ms == 0.0
        leads.append(h1.lead_ms)
    print(f"C2 twice in flight: lead of the second ticket {leads} ms (warm-up pair, asserted pair)")
    pcm, f32 = r1
    t_pad_tgt = tgt_sr
    ref_pcm = d["pcm_samples"].astype(np.int32)
    diff = np.abs(pcm[::997].astype(np.int32) - ref_pcm)
    idx = np.arange(0, int(d["chunk_lens"][0]), 997)
    keep = (idx >= t_pad_tgt) & (idx < int(d["chunk_lens"][0]) - t_pad_tgt)
    e = rms(f32[idx[keep] - t_pad_tgt] - d["raw_samples"][keep])
    print(f"C2 ticket: float rms err {e:.3e}, pcm max diff {diff.max()} LSB")
    assert e < FULL_RMS_BAR and diff.max() <= FULL_PCM_BAR and np.mean(diff > 1) < 0.02
    assert leads[-1] > 0, leads


# ---------------------------------------------------------------------------------------------- 4. two voice models
def test_tickets_alternating_between_two_voice_models(ctx):
    from polgen_rvc_amd import synthetic as S
    cfg_b = list(S.SYNTH_CFG_TINY)
    cfg_b[12], cfg_b[14], cfg_b[17] = [5, 2, 2, 2], [9, 4, 4, 4], 4000      # upp 40 -> 4 kHz
    m_a, m_b = _load(ctx, 6, [S.SYNTH_CFG_TINY, cfg_b])
    clips = [S.make_clip(50 + i, 1.5 + 0.4 * i) for i in range(4)]
    p = _params()
    want = [ctx.convert_batch(m_a if i % 2 == 0 else m_b, [c], p, want_f32=True) for i, c in enumerate(clips)]
    ts = []
    got = []
    for i, c in enumerate(clips):
        ts.append(ctx.convert_submit(m_a if i % 2 == 0 else m_b, [c], p, want_f32=True))
        if len(ts) == 2:
            got.append(ts.pop(0).wait())
    got += [t.wait() for t in ts]
    for w, g in zip(want, got):
        _same(w, g)


# ---------------------------------------------------------------------------------------------- 5. third submit
def test_third_submit_completes_the_oldest(ctx):
    from polgen_rvc_amd import synthetic as S
    (mid,) = _load(ctx, 7, [S.SYNTH_CFG_TINY])
    clips = [S.make_clip(80 + i, 2.0 + 0.5 * i) for i in range(3)]
    p = _params()
    want = [ctx.convert_batch(mid, [c], p, want_f32=True) for c in clips]
    ts = []
    for c in clips:
        ts.append(ctx.convert_submit(mid, [c], p, want_f32=True))
        assert ctx.convert_inflight() <= 2
    assert ts[0].done()
    for w, t in zip(want, ts):
        _same(w, t.wait())
    assert ctx.convert_inflight() == 0


# ---------------------------------------------------------------------------------------------- 6. interleaving
def test_other_entry_points_complete_the_tickets_in_flight(ctx):
    from polgen_rvc_amd import synthetic as S, weights as W
    (mid,) = _load(ctx, 8, [S.SYNTH_CFG_TINY])
    hcfg = S.HUBERT_CFG_TINY
    st_extra = S.synth_state(S.SYNTH_CFG_TINY, 99, input_dim=hcfg["embed_dim"])
    unused = ctx.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), st_extra)
    a, b, other = S.make_clip(90, 2.0), S.make_clip(91, 2.6), S.make_clip(92, 1.4)
    p = _params()
    want_a, want_b = ctx.convert_batch(mid, [a], p, want_f32=True), ctx.convert_batch(mid, [b], p, want_f32=True)
    idle_conv = ctx.convert_batch(mid, [other], p, want_f32=True)
    idle_f0 = ctx.rmvpe_f0(other)
    big = S.make_index(512, hcfg["embed_dim"], 2)
    new_ids = []

    def between(what):
        ta, tb = ctx.convert_submit(mid, [a], p, want_f32=True), ctx.convert_submit(mid, [b], p, want_f32=True)
        what()
        assert ctx.convert_inflight() == 0          # the entry point completed them
        _same(want_a, ta.wait())
        _same(want_b, tb.wait())

    between(lambda: _same(idle_conv, ctx.convert_batch(mid, [other], p, want_f32=True)))
    between(lambda: np.testing.assert_array_equal(idle_f0, ctx.rmvpe_f0(other)))
    try:
        between(lambda: ctx.load_index(big))
    finally:
        ctx.load_index(None)
    between(lambda: ctx.unload_synth(unused))
    between(lambda: new_ids.append(ctx.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), st_extra)))
    _same(ctx.convert_batch(new_ids[0], [other], p, want_f32=True),
          ctx.convert_submit(new_ids[0], [other], p, want_f32=True).wait())


# ---------------------------------------------------------------------------------------------- 7. BiGRU fallback
def test_bigru_fallback_is_attributed_to_its_ticket():
    """Full-size RMVPE (the cluster kernel only runs there; the plain kernel differs from it in the last bits, so each twin
    must take the same path).  Only the host-side "behave as if it had timed out" hook (what = 1) is used."""
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    hcfg, scfg, rcfg = S.HUBERT_CFG_TINY, S.SYNTH_CFG_TINY, S.RMVPE_CFG_FULL
    c = _lib.Context(0)
    try:
        c.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, 5))
        c.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, 1900))
        mid = c.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 5, input_dim=hcfg["embed_dim"]))
        A, B = S.make_clip(3, 2.0), S.make_clip(4, 2.4)
        p = _params()
        want_a = c.convert_batch(mid, [A], p, want_f32=True)
        n0 = c.gru_fallbacks()
        c.debug_inject(1)
        want_b = c.convert_batch(mid, [B], p, want_f32=True)
        assert c.gru_fallbacks() == n0 + 1
        clean_b = c.convert_batch(mid, [B], p, want_f32=True)
        n1 = c.gru_fallbacks()
        ta = c.convert_submit(mid, [A], p, want_f32=True)
        c.debug_inject(1)
        tb = c.convert_submit(mid, [B], p, want_f32=True)
        _same(want_a, ta.wait())
        _same(want_b, tb.wait())
        assert c.gru_fallbacks() == n1 + 1
        _same(clean_b, c.convert_submit(mid, [B], p, want_f32=True).wait())       # back on the cluster kernel
        assert c.gru_fallbacks() == n1 + 1
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- 8. range guard
def _overflow_ctx():
    from polgen_rvc_amd import _lib, synthetic as S, weights as W
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    st = {k: np.array(v) for k, v in S.hubert_state(hcfg, 3).items()}
    st["encoder.layers.1.fc1.weight"] *= np.float32(2e5)
    st["encoder.layers.1.fc1.bias"] *= np.float32(2e5)
    st["encoder.layers.1.fc2.weight"] *= np.float32(1.0 / 2e5)
    c = _lib.Context(0)
    c.load_hubert(W.hubert_cfg_struct(hcfg), st)
    c.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, 3))
    mid = c.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 3, input_dim=hcfg["embed_dim"]))
    return c, mid


def test_range_guard_with_tickets_equals_synchronous_calls_in_submit_order():
    from polgen_rvc_amd import _lib, synthetic as S
    clips = [S.make_clip(60 + i, 2.0 + 0.3 * i) for i in range(3)]
    p = _lib.Params(0.0, 50.0, 1100.0, 0.0, 0.33, 1.0, 0, 1, 6, 38, 41, 7)
    ca, mid = _overflow_ctx()
    try:
        want = [ca.convert_batch(mid, [c], p, want_f32=True) for c in clips]
        pinned, layers = ca.fp32_pinned(), ca.fp32_layers()
        assert ca.fp32_reruns() >= 1 and layers >= 1
    finally:
        ca.close()
    for reverse in (False, True):
        cb, mid = _overflow_ctx()
        try:
            t0, t1 = cb.convert_submit(mid, [clips[0]], p, want_f32=True), cb.convert_submit(mid, [clips[1]], p, want_f32=True)
            if reverse:                 # completions settle in submit order whatever the order of the waits
                g1, g0 = t1.wait(), t0.wait()
                g2 = cb.convert_submit(mid, [clips[2]], p, want_f32=True).wait()
            else:                       # two in flight throughout
                g0 = t0.wait()
                t2 = cb.convert_submit(mid, [clips[2]], p, want_f32=True)
                g1, g2 = t1.wait(), t2.wait()
            for w, g in zip(want, (g0, g1, g2)):
                _same(w, g)
            assert cb.fp32_pinned() == pinned and cb.fp32_layers() == layers
            assert cb.fp32_reruns() >= 1
        finally:
            cb.close()


# ---------------------------------------------------------------------------------------------- 9. misuse
def test_misuse_is_an_error_with_a_message_and_leaves_the_context_usable(ctx):
    from polgen_rvc_amd import _lib, synthetic as S
    (mid,) = _load(ctx, 9, [S.SYNTH_CFG_TINY])
    clip = S.make_clip(95, 1.5)
    p = _params()
    want = ctx.convert_batch(mid, [clip], p, want_f32=True)
    t = ctx.convert_submit(mid, [clip], p, want_f32=True)
    _same(want, t.wait())
    with pytest.raises(_lib.RvcxError, match="already"):
        t.wait()
    rc = _lib.lib().rvcx_convert_wait(ctx._h, t.id)                      # twice at the ABI
    assert rc == -1 and b"ticket" in _lib.lib().rvcx_last_error(ctx._h)
    other = _lib.Context(0)
    try:
        assert _lib.lib().rvcx_convert_wait(other._h, t.id) == -1      # a ticket of another context
        assert b"ticket" in _lib.lib().rvcx_last_error(other._h)
        t2 = ctx.convert_submit(mid, [clip], p, want_f32=True)
        assert _lib.lib().rvcx_convert_wait(other._h, t2.id) == -1
        _same(want, t2.wait())
    finally:
        other.close()
    with pytest.raises(_lib.RvcxError):
        ctx.convert_submit(1234, [clip], p)
    with pytest.raises(_lib.RvcxError, match="18 samples"):
        ctx.convert_submit(mid, [clip[:18]], p)
    assert ctx.convert_inflight() == 0
    # with a ticket in flight a failing submit leaves that ticket intact
    t3 = ctx.convert_submit(mid, [clip], p, want_f32=True)
    with pytest.raises(_lib.RvcxError):
        ctx.convert_submit(mid, [clip[:18]], p)
    _same(want, t3.wait())
    assert ctx.convert_inflight() == 0
    _same(want, ctx.convert_submit(mid, [clip], p, want_f32=True).wait())


def test_wait_from_other_threads_in_any_order(ctx):
    from polgen_rvc_amd import synthetic as S
    (mid,) = _load(ctx, 9, [S.SYNTH_CFG_TINY])
    clips = [S.make_clip(96, 2.0), S.make_clip(97, 2.5)]
    p = _params()
    want = [ctx.convert_batch(mid, [c], p, want_f32=True) for c in clips]
    ts = [ctx.convert_submit(mid, [c], p, want_f32=True) for c in clips]
    got = [None, None]

    def waiter(i):
        got[i] = ts[i].wait()

    th = [threading.Thread(target=waiter, args=(i,)) for i in (1, 0)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for w, g in zip(want, got):
        _same(w, g)


# ---------------------------------------------------------------------------------------------- 10. Python layer
def test_python_layer_stream_files_and_dropped_ticket(ctx, tmp_path):
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.infer import infer as I
    from polgen_rvc_amd.infer.audio import write_output
    cfgs = (S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY)
    hub, cpt = _setup(ctx, cfgs, 11)
    cfg = I.Config()
    cfg.x_pad, cfg.x_query, cfg.x_center, cfg.x_max = 1, 1, 2, 3
    cpt, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, cfg, None, cpt=cpt)
    vc.seed = 21
    clips = [S.make_clip(100 + i, s).astype(np.float64) for i, s in enumerate([1.3, 2.9, 5.2, 1.3, 0.8, 2.0])]
    args = (0.0, "rmvpe+", None, 0, 1, 3, tgt_sr, 0, 1.0, "v2", 0.33, 128, None)
    want = [vc.pipeline(hub, net_g, 0, c, "x.wav", *args) for c in clips]
    got = list(vc.pipeline_stream(hub, net_g, 0, iter(clips), "x.wav", *args))
    assert len(got) == len(want)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    # rvc_infer_many writes what rvc_infer writes (WAV bytes, and a real FLAC stream for ".flac")
    ins = []
    for i, c in enumerate(clips[:3]):
        path = str(tmp_path / f"in{i}.wav")
        write_output(path, np.clip(c * 32767.0, -32768, 32767).astype(np.int16), 16000)
        ins.append(path)
    names = ["a.wav", "b.flac", "c.wav"]
    for path, name in zip(ins, names):
        I.rvc_infer(None, 0, path, str(tmp_path / ("one_" + name)), 0.0, "rmvpe+", cpt, version, net_g, 3, tgt_sr, 1.0, 0.33,
                    128, vc, hub)
    I.rvc_infer_many(None, 0, ins, [str(tmp_path / ("many_" + n)) for n in names], 0.0, "rmvpe+", cpt, version, net_g, 3,
                     tgt_sr, 1.0, 0.33, 128, vc, hub)
    for name in names:
        one, many = (tmp_path / ("one_" + name)).read_bytes(), (tmp_path / ("many_" + name)).read_bytes()
        assert len(one) > 1000 and one == many, name
    # Files that are not at 16 kHz (the usual case of a folder): load_audio resamples on the GPU between two submits, and
    # that must not complete the conversions in flight.  A ticket's lead is exactly 0 only when it was submitted into an
    # idle context; every ticket after the first must have found its predecessor still in flight (lead != 0; the sign is
    # a matter of timing at this model size and is asserted at full size, test_full_size_c2_twice_in_flight_overlaps).
    from scipy.io import wavfile
    g = np.random.Generator(np.random.PCG64(3))
    ins48 = []
    for i, secs in enumerate([1.1, 1.6, 2.3, 1.4, 0.9]):
        path = str(tmp_path / f"in48_{i}.wav")
        tt = np.arange(int(48000 * secs)) / 48000.0
        x = 0.3 * np.sin(2 * np.pi * (150 + 20 * i) * tt) * (1 + 0.3 * np.sin(2 * np.pi * 3 * tt)) + 0.01 * g.standard_normal(tt.size)
        wavfile.write(path, 48000, np.clip(x * 32767.0, -32768, 32767).astype(np.int16))
        ins48.append(path)
    for i, path in enumerate(ins48):
        I.rvc_infer(None, 0, path, str(tmp_path / f"one48_{i}.wav"), 0.0, "rmvpe+", cpt, version, net_g, 3, tgt_sr, 1.0, 0.33,
                    128, vc, hub)
    handles, loads_seen = [], []
    real_async, real_load = vc.pipeline_async, I.load_audio

    def spy_async(*a, **k):
        handles.append(real_async(*a, **k))
        return handles[-1]

    def spy_load(*a, **k):
        out = real_load(*a, **k)
        loads_seen.append(sum(1 for h in handles if h._res is None))      # conversions submitted and not yet collected
        return out

    vc.pipeline_async, I.load_audio = spy_async, spy_load
    try:
        I.rvc_infer_many(None, 0, ins48, [str(tmp_path / f"many48_{i}.wav") for i in range(len(ins48))], 0.0, "rmvpe+", cpt,
                         version, net_g, 3, tgt_sr, 1.0, 0.33, 128, vc, hub)
    finally:
        I.load_audio = real_load
        del vc.pipeline_async
    for i in range(len(ins48)):
        one, many = (tmp_path / f"one48_{i}.wav").read_bytes(), (tmp_path / f"many48_{i}.wav").read_bytes()
        assert len(one) > 1000 and one == many, i
    leads = [h.lead_ms for h in handles]
    print(f"rvc_infer_many at 48 kHz: held while decoding {loads_seen}, leads {leads}")
    assert loads_seen == [0, 1, 2, 2, 2]            # the third file on is decoded with two conversions held in flight
    assert leads[0] == 0.0 and all(v != 0.0 for v in leads[1:]), leads
    # a Ticket dropped unwaited: its finaliser waits, the borrowed buffers outlive the device's use of them
    p = _params()
    want1 = ctx.convert_batch(net_g.model_id, [clips[1]], p, want_f32=True)
    t = ctx.convert_submit(net_g.model_id, [clips[1]], p, want_f32=True)
    del t
    gc.collect()
    assert ctx.convert_inflight() == 0
    _same(want1, ctx.convert_submit(net_g.model_id, [clips[1]], p, want_f32=True).wait())
