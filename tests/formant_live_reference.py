"""float64 restatement of include/rvcx.h stage 19 (the live formant shift of a live-stream session: stage 17 without a source on
stage 16's causal grid) in numpy, written from the definition alone.  The links of a frame are those of formant_reference (stage
17's, unchanged), the grid, the frame count and the synthesis with its delay those of denoise_live_reference (stage 16's,
unchanged).  The signal is taken whole; a stream that has received n samples has emitted the first n samples of what this
returns.  D and A2 carry the float32 roundings of the definition (they are what the library stores); everything behind them is
float64.  Shared by tests/test_formant_live_host.py and tests/test_gpu_stream_formant.py."""
import numpy as np

import denoise_live_reference as G
import formant_reference as F
from denoise_live_reference import frames, geometry, rel, rms  # noqa: F401

DEFAULTS = F.DEFAULTS


def values(**kw):
    """the six values as the ABI carries them (float32 where they are floats); semitones= in place of ratio="""
    if "semitones" in kw:
        kw = dict(kw, ratio=F.ratio_of(kw.pop("semitones")))
    v = F.values(**kw)
    return {k: (int(x) if k in ("iterations", "keep_energy") else float(np.float32(x))) for k, x in v.items()}


def off(v):
    return v["amount"] == 0.0 or v["ratio"] == 1.0


def quefrency_bins(sr, quefrency_ms):
    """nc, and whether it lies in 1 .. N / 8 at the live N"""
    nc = F.quefrency_bins(sr, quefrency_ms)
    return nc, 1 <= nc <= geometry(sr)[0] // 8


def frame_links(D32, sr, v):
    """E, g, s of frames whose float32 spectra are D32 (T, nb): stage 17's rules with Es = E"""
    N = geometry(sr)[0]
    nc, ok = quefrency_bins(sr, v["quefrency_ms"])
    assert ok, (nc, N)
    E = F.envelope(F.log_spectrum(D32), N, nc, v["iterations"])
    g = F.gain(F.warp(E, v["ratio"]), E, v["amount"], v["max_gain_db"])
    s = F.energy_scale(F.a2_of(D32), g) if v["keep_energy"] else np.ones(D32.shape[0], np.float32)
    return E, g, s


def synthesis(D32, g, s, n, sr):
    """what the stream has emitted after n samples, y (n) in float64: Y = fl(g s) D with the imaginary parts of bins 0 and N / 2
    dropped (irfft ignores them), stage 16's overlap-add over the frames t >= 0 and its delay of N"""
    gs = (np.asarray(g, np.float32) * np.asarray(s, np.float32)[:, None]).astype(np.float32).astype(np.float64)
    return G.synthesis(np.asarray(D32).astype(np.complex128), gs, 1.0, n, sr)


def formant_live(x, sr, **kw):
    """stage 19 on one channel, the signal whole -> dict of D, E, g, s and y (float64)"""
    v = values(**kw)
    x = np.asarray(x)
    n = x.shape[0]
    N = geometry(sr)[0]
    D32 = G.round_d(G.analysis(x, sr))
    E, g, s = frame_links(D32, sr, v)
    if off(v):
        y = np.zeros(n)
        y[N:] = np.asarray(x, np.float64)[:max(n - N, 0)]
    else:
        y = synthesis(D32, g, s, n, sr)
    return dict(D=D32, E=E, g=g, s=s, y=y)


def history(x, sr, block, plan):
    """the same under a parameter history: plan = [(first block, values dict), ..] ascending from block 0; frame t takes the
    values in force in the step that completes it, a step emits by the values in force in it -> y (float64)"""
    x = np.asarray(x)
    n = x.shape[0]
    N, H, _ = geometry(sr)
    assert n % block == 0 and plan[0][0] == 0
    D32 = G.round_d(G.analysis(x, sr))
    T = D32.shape[0]
    done = (np.arange(T) * H + N // 2 - 1) // block                    # the step that completes frame t
    starts = [k for k, _ in plan]
    which = np.searchsorted(starts, done, side="right") - 1
    gs = np.zeros((T, D32.shape[1]))
    vs = [values(**kw) for _, kw in plan]
    for i, v in enumerate(vs):
        sel = which == i
        if sel.any():
            _, g, s = frame_links(D32[sel], sr, v)
            gs[sel] = (g.astype(np.float32) * np.asarray(s, np.float32)[:, None]).astype(np.float32)
    y = G.synthesis(D32.astype(np.complex128), gs, 1.0, n, sr)
    delayed = np.zeros(n)
    delayed[N:] = np.asarray(x, np.float64)[:max(n - N, 0)]
    step_of = np.arange(n) // block
    in_force = np.searchsorted(starts, step_of, side="right") - 1
    is_off = np.asarray([off(v) for v in vs])[in_force]
    return np.where(is_off, delayed, y)


# ---- the links of a library (host twin or device) against the functions above --------------------------------------------------
def check_links(y, t, x, sr, worst, **kw):
    """links D, E, g, s, y of one channel, each judged on the library's own input (formant_reference.check_links on the live
    grid); t: the library's taps (D optional: the device has none, the restatement's rounded D then stands in); worst collects
    the largest figures"""
    v = values(**kw)
    n = x.shape[0]
    N, H, nb = geometry(sr)
    T = frames(n, sr)
    assert y.shape == (n,) and t["s"].shape == (T,) and t["E"].shape == (T, nb) and t["g"].shape == (T, nb)
    if T == 0:                         # no frame is complete: nothing has left but the delay's zeros
        assert not y.any()
        return y
    ref_D = G.analysis(x, sr)
    if "D" in t:
        assert t["D"].shape == (T, nb, 2)
        D32 = F.pairs_to_complex(t["D"])
        top = np.abs(ref_D).max(axis=1)
        err = np.abs(ref_D - D32.astype(np.complex128)).max(axis=1)
        worst["D"] = max(worst["D"], float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0)
        assert not err[top == 0].any()
    else:
        D32 = G.round_d(ref_D)
    nc, ok = quefrency_bins(sr, v["quefrency_ms"])
    assert ok
    worst["E"] = max(worst["E"], float(np.abs(t["E"] - F.envelope(F.log_spectrum(D32), N, nc, v["iterations"])).max()))
    g = F.gain(F.warp(t["E"], v["ratio"]), t["E"], v["amount"], v["max_gain_db"])
    worst["g"] = max(worst["g"], float(np.abs(t["g"] / g - 1.0).max()))
    if "D" in t:                       # given the same A2 and g, s is equal bit for bit
        s = F.energy_scale(F.a2_of(D32), t["g"]) if v["keep_energy"] else np.ones(T, np.float32)
        assert np.array_equal(t["s"], s)
    if not off(v):
        ref = synthesis(D32, t["g"], t["s"], n, sr)
        worst["y"] = max(worst["y"], float(np.abs(y - ref).max()) / max(float(np.abs(x).max()), 1e-30))
    return y


def realigned(fn, N):
    """shift(x, sr, semitones) for formant_reference.behaviour from a live fn(x, sr, semitones) -> y delayed by N(sr): the input
    is followed by N(sr) zeros, the output loses its first N(sr) samples"""
    def shift(x, sr, semitones):
        d = N(sr)
        y = fn(np.concatenate([np.asarray(x, np.float32), np.zeros(d, np.float32)]), sr, semitones)
        return np.asarray(y)[d:]
    return shift
