#!/usr/bin/env python3
"""Driver of the host-side sanitizer runs of the conversion tickets (tools/host_tickets.sh asan | tsan; RVCX_LIBRARY names
the sanitizer build, whose HIP runtime is tools/hipstub: kernels do not run, so sample values are meaningless).  What is
exercised is the host code of rvcx_convert_submit / _wait / _poll / _inflight: four threads sharing one context for a few
hundred tickets, the third-submit rule, loads and unloads between submits, every misuse path, destroy with tickets in
flight, live-stream sessions beside the tickets, and out_n / last_cuts / last_micro_batches of each ticket against the synchronous call's.  Prints
HOST_TICKETS_OK at the end."""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("RVCX_DEBUG", "1")
import numpy as np

import polgen_rvc_amd  # noqa: F401
from polgen_rvc_amd import _lib, synthetic as S, weights as W

assert "san" in _lib.LIB_PATH, "run through tools/host_tickets.sh (RVCX_LIBRARY must name a sanitizer build)"
L = _lib.lib()
assert "hipstub" in _lib.device_info(0)[0]


def params(**kw):
    p = _lib.Params(0.0, 50.0, 1100.0, 0.0, 0.33, 1.0, 0, 1, 1, 2, 3, 7)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def load(ctx):
    hcfg, rcfg, scfg = S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY
    ctx.load_hubert(W.hubert_cfg_struct(hcfg), S.hubert_state(hcfg, 1))
    ctx.load_rmvpe(W.rmvpe_cfg_struct(rcfg), S.rmvpe_state(rcfg, 1))
    return ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 4, input_dim=hcfg["embed_dim"]))


ctx = _lib.Context(0)
mid = load(ctx)
clips = [S.make_clip(i, s) for i, s in enumerate([0.9, 1.7, 2.9, 5.3, 7.1])]        # the last two are cut at x_max = 3


def sync_record(cl, **kw):
    pcm = ctx.convert_batch(mid, cl, params(), **kw)
    return [len(x) for x in pcm], ctx.last_cuts(), ctx.last_micro_batches()


want = {i: sync_record([c]) for i, c in enumerate(clips)}
want_all = sync_record(clips)

# ---- one ticket = the call (sample counts, cut points, micro-batches), single and ragged, f0 file
for i, c in enumerate(clips):
    t = ctx.convert_submit(mid, [c], params())
    assert t.done() in (True, False)
    pcm = t.wait()
    assert ([len(x) for x in pcm], ctx.last_cuts(), ctx.last_micro_batches()) == want[i], i
    assert t.lead_ms == 0.0
t = ctx.convert_submit(mid, clips, params(), want_f32=True)
pcm, f32 = t.wait()
assert ([len(x) for x in pcm], ctx.last_cuts(), ctx.last_micro_batches()) == want_all
tab = np.array([[0.0, 100.0], [0.5, 200.0], [1.0, 150.0]], np.float32)
ctx.convert_submit(mid, clips[:2], params(), inp_f0=[tab, tab]).wait()

# ---- third submit: never more than two in flight, every ticket stays waitable, any order
ts = [ctx.convert_submit(mid, [clips[i % len(clips)]], params()) for i in range(7)]
assert ctx.convert_inflight() <= 2
for k in (6, 0, 3, 5, 1, 2, 4):
    pcm = ts[k].wait()
    assert ([len(x) for x in pcm], ctx.last_cuts(), ctx.last_micro_batches()) == want[k % len(clips)], k

# ---- loads, unloads and synchronous calls with tickets in flight
hcfg, scfg = S.HUBERT_CFG_TINY, S.SYNTH_CFG_TINY
for what in range(4):
    ta, tb = ctx.convert_submit(mid, [clips[1]], params()), ctx.convert_submit(mid, [clips[3]], params())
    if what == 0:
        extra = ctx.load_synth(W.synth_cfg_struct(scfg, hcfg["embed_dim"]), S.synth_state(scfg, 9, input_dim=hcfg["embed_dim"]))
    elif what == 1:
        ctx.unload_synth(extra)
    elif what == 2:
        ctx.load_index(S.make_index(256, hcfg["embed_dim"], 1))
    else:
        ctx.load_index(None)
        assert sync_record([clips[0]]) == want[0]
    assert ctx.convert_inflight() == 0
    assert [len(x) for x in tb.wait()] == want[3][0] and ctx.last_cuts() == want[3][1]
    assert [len(x) for x in ta.wait()] == want[1][0] and ctx.last_cuts() == want[1][1]

# ---- load_audio's resampler runs beside the tickets in flight: it does not complete them
ta, tb = ctx.convert_submit(mid, [clips[1]], params()), ctx.convert_submit(mid, [clips[3]], params())
y = ctx.resample(np.zeros((4800, 2)), 48000, 16000)
assert y.shape[0] == 1600
tc = ctx.convert_submit(mid, [clips[0]], params())
for t, k in ((ta, 1), (tb, 3), (tc, 0)):
    assert [len(x) for x in t.wait()] == want[k][0]
assert tb.lead_ms != 0.0 and tc.lead_ms != 0.0          # each found its predecessor in flight (0 = an idle context)
assert np.isnan(_lib.lib().rvcx_ticket_lead_ms(ctx._h, 987654321))

# ---- the injected BiGRU time-out belongs to the ticket submitted next
n0 = ctx.gru_fallbacks()
ta = ctx.convert_submit(mid, [clips[0]], params())
ctx.debug_inject(1)
tb = ctx.convert_submit(mid, [clips[1]], params())
ta.wait()
assert ctx.gru_fallbacks() == n0
tb.wait()
assert ctx.gru_fallbacks() == n0 + 1

# ---- misuse
t = ctx.convert_submit(mid, [clips[0]], params())
t.wait()
assert L.rvcx_convert_wait(ctx._h, t.id) == -1 and b"ticket" in L.rvcx_last_error(ctx._h)
assert L.rvcx_convert_poll(ctx._h, t.id) == -1
assert L.rvcx_convert_wait(ctx._h, 123456789) == -1
other = _lib.Context(0)
t = ctx.convert_submit(mid, [clips[0]], params())
assert L.rvcx_convert_wait(other._h, t.id) == -1 and b"ticket" in L.rvcx_last_error(other._h)
other.close()
for bad in (lambda: ctx.convert_submit(99, [clips[0]], params()), lambda: ctx.convert_submit(mid, [clips[0][:18]], params()),
            lambda: ctx.convert_submit(mid, [np.zeros(0, np.float32)], params())):
    try:
        bad()
        raise SystemExit("misuse was accepted")
    except _lib.RvcxError as e:
        assert str(e)
t.wait()
assert ctx.convert_inflight() == 0
assert L.rvcx_convert_submit(ctx._h, mid, 1, None, 0, None, None, None, None, None, None, None, None) == -1
t = ctx.convert_submit(mid, [], params())               # an empty ticket is a ticket
assert t.wait() == []

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


stream_lifecycle(ctx, mid, S.HUBERT_CFG_TINY, clips, params)

# ---- four threads share the context: submit / poll / wait, a few hundred tickets, some waited for by another thread
errors, handoff, hand_lock = [], [], threading.Lock()


def worker(k):
    try:
        g = np.random.Generator(np.random.PCG64(k))
        mine = []
        for it in range(60):
            i = int(g.integers(0, len(clips)))
            mine.append((i, ctx.convert_submit(mid, [clips[i]], params(seed=k))))
            if it % 7 == 3:
                with hand_lock:
                    handoff.append(mine.pop(0))
            if it % 5 == 0:
                ctx.convert_inflight()
                mine[-1][1].done()
            if it % 11 == 10:
                ctx.convert_batch(mid, [clips[0]], params())
            if it % 13 == 5:
                ctx.resample(np.zeros(2400), 24000, 16000)
            while len(mine) > 2:
                i0, t0 = mine.pop(int(g.integers(0, len(mine))))
                assert [len(x) for x in t0.wait()] == want[i0][0]
            with hand_lock:
                theirs = handoff.pop() if handoff and it % 3 == 0 else None
            if theirs:
                assert [len(x) for x in theirs[1].wait()] == want[theirs[0]][0]
        for i0, t0 in mine:
            assert [len(x) for x in t0.wait()] == want[i0][0]
    except BaseException as e:  # noqa: BLE001
        errors.append(repr(e))




def stream_worker():
    """a live session stepping while the four ticket threads submit and wait: every step finds the context to itself"""
    try:
        blk = np.stack([clips[1][:960], clips[2][:960]]).astype(np.float32)
        with ctx.stream_open(mid, params(seed=5), [0, 1], [0.0, 1.0], 6, 20, 2, 1) as se:
            for it in range(40):
                assert se.step(blk).shape == (2, se.block_out)
                if it == 20:
                    se.reset()
    except BaseException as e:  # noqa: BLE001
        errors.append(repr(e))


threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
threads.append(threading.Thread(target=stream_worker))
for th in threads:
    th.start()
for th in threads:
    th.join()
assert not errors, errors
for i0, t0 in handoff:
    assert [len(x) for x in t0.wait()] == want[i0][0]
assert ctx.convert_inflight() == 0

# ---- destroy with tickets in flight (and one dropped unwaited)
c2 = _lib.Context(0)
m2 = load(c2)
open_session = c2.stream_open(m2, params(), [0], [0.0], 6, 20, 2, 1)      # and with a session open
open_session.step(clips[1][None, :960].astype(np.float32))
keep = [c2.convert_submit(m2, [clips[i]], params()) for i in (0, 3)]
c2.close()
for t in keep:
    t._waited = True            # their context is gone; the callers' buffers were filled by rvcx_destroy
c3 = _lib.Context(0)
m3 = load(c3)
t = c3.convert_submit(m3, [clips[2]], params())
del t
assert c3.convert_inflight() == 0
c3.close()
ctx.close()
print("HOST_TICKETS_OK")
