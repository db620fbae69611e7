#!/usr/bin/env python3
"""Driver of the host-side sanitizer build (make host-asan; tools/host_asan.sh runs it with the ASan runtime preloaded and
RVCX_LIBRARY=build/asan/librvcx_asan.so).  The library's HIP runtime is tools/hipstub: "device" memory is host memory and
kernels do not run, so outputs are meaningless -- what is exercised under AddressSanitizer + UBSan is the host code:
checkpoint folding / packing for all five model kinds (+ both index kinds), weight regions (free / reload / clone /
adopt), the micro-batch planner over BASELINE configs[4]'s 256 lengths, bucket lengths, the chunk planner of clips longer
than x_max, the f0-file track, arena arithmetic, error paths, the lifecycle of live-stream sessions, the FLAC codec.  Prints HOST_ASAN_OK at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("RVCX_DEBUG", "1")
import numpy as np

import polgen_rvc_amd  # noqa: F401
from polgen_rvc_amd import _lib, synthetic as S, weights as W

assert "asan" in _lib.LIB_PATH, "run through tools/host_asan.sh (RVCX_LIBRARY must name the sanitizer build)"
L = _lib.lib()
name, total = _lib.device_info(0)
assert "hipstub" in name, name


def params(**kw):
    p = _lib.Params(0.0, 50.0, 1100.0, 0.0, 0.33, 1.0, 0, 1, 6, 38, 41, 7)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def load_all(ctx, full):
    hcfg = S.HUBERT_CFG_BASE if full else S.HUBERT_CFG_TINY
    rcfg = S.RMVPE_CFG_FULL if full else S.RMVPE_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, 1))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, 1))
    sd = S.fcpe_state(S.FCPE_CFG_FULL if full else S.FCPE_CFG_TINY, 2)
    ctx.load_fcpe(W.fcpe_cfg_struct(W.fcpe_cfg_from_state(sd)), sd)
    ctx.load_crepe(S.crepe_state("full" if full else "tiny", 3))
    mids = []
    for scfg in ([S.SYNTH_CFG_48K, S.SYNTH_CFG_40K] if full else [S.SYNTH_CFG_TINY]):
        mids.append(ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 4, input_dim=hcfg["embed_dim"])))
    return hcfg, mids


# ---- live-stream sessions: open, three steps, reset, close; a step after unload_synth; a step with a ticket in flight;
# every refusal of open; destroy with a session open (further down)
def stream_lifecycle(ctx, mid, hcfg, clips, params):
    Fb, Fc, Fx, Fs = 6, 20, 2, 1
    blk = np.stack([clips[1][:Fb * 160], clips[2][:Fb * 160]]).astype(np.float32)
    with ctx.stream_open(mid, params(seed=3), [0, 1], [0.0, 2.0], Fb, Fc, Fx, Fs) as se:
        assert se.frames == 28 and se.skip_head == 19 and se.n_streams == 2
        for k in range(3):
            out = se.step(blk)
            assert out.shape == (2, se.block_out)
        out, pre, offs = se.step(blk, noise=np.zeros((2, se.noise_len), np.float32), taps=True)
        assert pre.shape == (2, se.tail_len) and offs.shape == (2,)
        se.reset()
        se.step(blk)
        t = ctx.convert_submit(mid, [clips[0]], params())        # a step completes the ticket in flight first
        se.step(blk)
        assert ctx.convert_inflight() == 0
        t.wait()
        for bad in (lambda: se.step(blk[:1]), lambda: se.step(blk, noise=np.zeros((2, 3), np.float32))):
            try:
                bad()
                raise SystemExit("misuse was accepted")
            except _lib.RvcxError:
                pass
    assert L.rvcx_stream_step(ctx._h, 12345, None, None, None, None, None) == -1
    assert L.rvcx_stream_close(ctx._h, 12345) == -1 and L.rvcx_stream_reset(ctx._h, 12345) == -1
    assert L.rvcx_stream_out_len(ctx._h, 12345) == -1 and L.rvcx_stream_frames(ctx._h, 12345) == -1
    scfg = S.SYNTH_CFG_TINY
    gone = ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 6, input_dim=hcfg["embed_dim"]))
    se = ctx.stream_open(gone, params(), [0], [0.0], Fb, Fc, Fx, Fs)
    se.step(blk[:1])
    ctx.unload_synth(gone)
    try:
        se.step(blk[:1])
        raise SystemExit("a step on an unloaded voice model was accepted")
    except _lib.RvcxError as e:
        assert "unloaded" in str(e)
    se.close()
    for geo, kw in (((Fb, 0, Fx, Fs), {}), ((0, Fc, Fx, Fs), {}), ((Fb, Fc, 0, Fs), {}), ((Fb, Fc, Fx, Fs), dict(f0_method=_lib.F0_CREPE)),
                    ((Fb, 7000, Fx, Fs), {})):
        try:
            ctx.stream_open(mid, params(**kw), [0], [0.0], *geo)
            raise SystemExit("a bad session was opened")
        except _lib.RvcxError:
            pass
    ctx.load_index(S.make_index(16, hcfg["embed_dim"] + 8, 1))
    try:
        ctx.stream_open(mid, params(), [0], [0.0], Fb, Fc, Fx, Fs)
        raise SystemExit("an index of another width was accepted")
    except _lib.RvcxError:
        pass
    ctx.load_index(S.make_index(6, hcfg["embed_dim"], 1))
    with ctx.stream_open(mid, params(index_rate=0.5), [0], [0.0], Fb, Fc, Fx, Fs) as se:
        se.step(blk[:1])
    ctx.load_index(None)
    y = np.zeros(11 + 37 + 5, np.float32)
    out, carry, off, sc = ctx.sola(y, np.ones(37, np.float32), 11, 37, 5, scores=True)
    assert out.shape == (11,) and carry.shape == (37,) and sc.shape == (6,)
    ph = np.zeros((2, 28, hcfg["embed_dim"]), np.float32)
    o, z = ctx.synth_infer(mid, ph, np.ones((2, 28), np.int32), np.zeros((2, 28), np.float32), skip_head=19,
                           z_noise=np.zeros((2, S.SYNTH_CFG_TINY[2], 28), np.float32))
    assert o.shape[1] == 9 * ctx.synth_upp(mid) and z.shape[2] == 9


# ---- tiny models with real (random) values: folding, packing, fp16 images, legacy weight-norm names, fp16 tensors
ctx = _lib.Context(0)
hcfg, mids = load_all(ctx, full=False)
ss = S.synth_state(S.SYNTH_CFG_TINY, 5, input_dim=hcfg["embed_dim"])
legacy = {k.replace(".parametrizations.weight.original0", ".weight_g").replace(".parametrizations.weight.original1", ".weight_v"):
          np.asarray(v).astype(np.float16) for k, v in ss.items()}
mids.append(ctx.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), legacy))
regions, layout = ctx.weights_regions()
assert len(regions) >= 5 and all(n > 0 for _, n in regions)
big = S.make_index(2048, hcfg["embed_dim"], 1)
ctx.load_index(big)
g = np.random.Generator(np.random.PCG64(1))
cent = big[g.choice(len(big), 16, replace=False)]
assign = np.argmin(((big[:, None, :] - cent[None]) ** 2).sum(-1), axis=1).astype(np.int32)
ctx.load_index_ivf(big, cent, assign, 1)
ctx.load_index(None)
# conversions: single clip, ragged batch, a clip long enough to be cut into chunks, f0 file, fcpe / crepe back-ends
clips = [S.make_clip(i, s) for i, s in enumerate([1.2, 2.5, 2.5, 1.7, 3.1])]
for m in mids:
    ctx.convert_batch(m, clips, params())
    ctx.convert_batch(m, clips[:1], params(volume_envelope=0.25, resample_sr=16000), want_f32=True)
long_clip = S.make_clip(9, 47.0)
ctx.convert_batch(mids[0], [long_clip, long_clip], params())
ctx.convert_batch(mids[0], clips[:2], params(f0_method=_lib.F0_FCPE))
tab = np.stack([np.linspace(0, 2, 21), np.full(21, 220.0)], axis=1).astype(np.float32)
ctx.convert_batch(mids[0], clips[:2], params(), inp_f0=[tab, tab])
assert len(_lib.f0_file_track(tab)) > 0 and len(_lib.f0_file_track(tab[:1])) >= 0
ctx.get_f0_x_ex(np.zeros(16000 * 3, np.float32), 300, params(), tab)
ctx.rmvpe_f0(clips[1], 0.03, 50, 1100)
ctx.hubert_features(clips[1], hcfg["embed_dim"])
ctx.resample(np.stack([clips[1], clips[1]], axis=1).astype(np.float64), 44100, 16000)
# region free / reload cycle, clone into a second context, adopt
for _ in range(3):
    L.rvcx_unload_synth(ctx._h, mids[-1])
    mids[-1] = ctx.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), ss)
ctx2 = _lib.Context(0)
with S.shapes_only():
    load_all(ctx2, full=False)
    ctx2.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), S.synth_state(S.SYNTH_CFG_TINY, 5, input_dim=hcfg["embed_dim"]))
ctx2.weights_clone(ctx)
ctx2.weights_adopt()
ctx2.convert_batch(0, clips[:2], params())
stream_lifecycle(ctx, mids[0], hcfg, clips, params)
open_session = ctx2.stream_open(0, params(), [0, 0], [0.0, 1.0], 6, 20, 2, 1)      # destroy with a session open
open_session.step(np.zeros((2, 960), np.float32))
# error paths: nothing may be read or written out of bounds on the way to the error code
for bad in (lambda: ctx.convert_batch(99, clips[:1], params()), lambda: ctx.convert_batch(mids[0], [np.zeros(0, np.float32)], params()),
            lambda: ctx2.weights_clone(ctx2) if False else ctx.load_synth(W.synth_cfg_struct(S.SYNTH_CFG_TINY, hcfg["embed_dim"]), {"x": np.zeros(3, np.float32)})):
    try:
        bad()
    except _lib.RvcxError:
        pass
ctx2.close()
ctx.close()

# ---- full-size models from shape-only placeholders (what ranks != 0 load): the real layouts, region chunking, the planner
ctx = _lib.Context(0)
with S.shapes_only():
    hcfg, (m48, m40) = load_all(ctx, full=True)
g = np.random.Generator(np.random.PCG64(5))
lengths = [int(round(s * 100)) * 160 for s in g.uniform(3.0, 15.0, 256)]          # bench.py c5_lengths()
p = params()
seen = set()
for n in lengths:
    mb = ctx.micro_batch(m48, n, p)
    bl = int(L.rvcx_bucket_length(ctx._h, m40, n, _lib.C.byref(p)))
    assert 1 <= mb <= 16 and n <= bl < n + 128 * 160, (n, mb, bl)      # the longest clip of the length class (128 frames wide)
    seen.add(bl)
assert 5 < len(seen) < 256
zero_clips = [np.zeros(n, np.float32) for n in lengths[:40]]
pcm = ctx.convert_batch(m40, zero_clips, p)
assert len(pcm) == 40 and sum(ctx.last_micro_batches()) == 40
ctx.convert_batch(m48, [np.zeros(16000 * 30, np.float32)] * 3, params(index_rate=0.0))
ctx.close()

# ---- the FLAC codec is host code too
pcm = (np.sin(np.arange(30000) * 0.01) * 20000).astype(np.int16)
blob = _lib.flac_encode(np.stack([pcm, pcm[::-1]], axis=1), 48000)
back, sr, bits = _lib.flac_decode(blob)
assert sr == 48000 and bits == 16 and np.array_equal(back[:, 0], pcm)
for cut in (10, 50, len(blob) // 2, len(blob) - 3):
    try:
        _lib.flac_decode(blob[:cut])
    except _lib.RvcxError:
        pass
# ---- post-production: the host twins are the product's arithmetic on the host; the chain's planning, grouping and copies run
# on the stub (launches are no-ops there, so every follower settles in its first pass)
g = np.random.Generator(np.random.PCG64(6))
x = (0.3 * g.standard_normal(3000)).astype(np.float32)
for sr in (8000, 192000):
    _lib.fx_highpass_host(x, sr)
    _lib.fx_biquad_host(x, _lib.fx_coeffs(2, sr, 440.0, 2.0 ** -0.5, 6.0))
    _lib.fx_compressor_host(x, sr, 4.0, -12.0)
    _lib.fx_gate_host(x, sr, -40.0, 8.0, 10.0, 100.0)
    _lib.fx_comb_host(x, _lib.fx_delay(sr, 1617 + 23), 0.84, 0.2)
    _lib.fx_allpass_host(x, _lib.fx_delay(sr, 225))
    _lib.fx_chorus_host(x, sr, 1.5, 0.25, 7.0, 0.5, 0.5)
for n in (0, 1, 7):
    _lib.fx_comb_host(x[:n], 5, 0.5, 0.2), _lib.fx_allpass_host(x[:n], 5), _lib.fx_chorus_host(x[:n], 8000, 1.0, 0.1, 2.0, 0.3, 0.5)
v = g.integers(-32768, 32768, (100, 2)).astype(np.int16)
for n_i in (0, 40, 100, 300):
    _lib.fx_mix_host(v, g.integers(-32768, 32768, (n_i, 2)).astype(np.int16), 6.0, -3.0)
ctx = _lib.Context(0)
items = [np.zeros((n, 2), np.float32) for n in (1, 150, 1024, 5000)]
fxp = _lib.FxParams.make(dict(_lib.FX_UI_DEFAULTS, chorus_mix=0.5, chorus_feedback=0.3, chorus_centre_delay_ms=7.0,
                              low_shelf_gain=3.0, high_shelf_gain=-3.0), 8000, 2)
os.environ["RVCX_MAX_BATCH"] = "3"
assert [y.shape for y in ctx.fx_chain(items, fxp)] == [a.shape for a in items] and ctx.fx_last_passes()[1] == 2
del os.environ["RVCX_MAX_BATCH"]
ctx.fx_compressor(items[3][:, 0], 8000, 4.0, -12.0, want_env=True)
ctx.fx_mix(v, v[:30], 0.0, 0.0)
for bad in (lambda: ctx.fx_reverb(items[1][:, 0], 8000, 0.1, 0.9, 0.1, 0.8, 1.0), lambda: ctx.fx_chorus(items[1], 8000, 1, 0.2, 7, 1.0, 0.5),
            lambda: ctx.fx_highpass(items[1], 22050), lambda: _lib.fx_gate_host(x, 8000, -40.0, 0.5, 10.0, 100.0)):
    try:
        bad()
    except _lib.RvcxError:
        pass
ctx.close()
print("HOST_ASAN_OK launches", int(L.hipstub_launches()) if hasattr(L, "hipstub_launches") else -1)
