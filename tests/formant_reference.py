"""float64 restatement of include/rvcx.h stages 17 and 18 (envelope transfer: formant shift and formant-preserving pitch
shift) in numpy, written from the definition alone, one function per link: numpy's rfft / irfft for the transforms, stage 13's
grid from stretch_reference.  Every function can start from its own analysis or from arrays that somebody else computed, so
that a test can check the library link by link.  Also the test signals, the measures and the behaviour conditions that
tests/test_formant_host.py and tests/test_gpu_formant.py share."""
import numpy as np

from stretch_reference import a2_of, analysis, geometry, pairs_to_complex, pitch_ratio, pitch_shift, rms, round_d, window  # noqa: F401

DEFAULTS = dict(ratio=1.0, amount=1.0, quefrency_ms=1.5, iterations=8, max_gain_db=24.0, keep_energy=1)


def values(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def frames(n, sr):
    return n // geometry(sr)[1] + 1


def quefrency_bins(sr, quefrency_ms):
    """nc = floor(quefrency_ms sr / 1000), the value as the library holds it (float32)"""
    return int(np.floor(float(np.float32(quefrency_ms)) * sr / 1000.0))


def ratio_of(semitones):
    """the ratio as the library holds it (float32)"""
    return float(np.float32(2.0 ** (semitones / 12.0)))


# ---- the links ---------------------------------------------------------------------------------------------------------------
def log_spectrum(D32):
    """L (.., nb) in float64 from the float32 D: eps and the sum A2 + eps in float32 as defined, the logarithm in double"""
    a2 = a2_of(D32)
    top = a2.max(axis=-1, keepdims=True)
    eps = (np.float32(1e-10) * top).astype(np.float32) + np.float32(1e-20)
    return 0.5 * np.log((a2 + eps).astype(np.float32).astype(np.float64))


def lift(V, N, nc):
    """the real even extension of V (.., nb), its cepstrum cut at nc, back"""
    c = np.fft.irfft(V, N, axis=-1)
    c[..., nc + 1:N - nc] = 0.0
    c[..., N - nc:] = c[..., nc:0:-1]
    return np.fft.rfft(c, axis=-1).real


def envelope(L, N, nc, iterations):
    """the true envelope E (.., nb): iterations + 1 lifts under the maximum with L"""
    L = np.asarray(L, np.float64)
    V = L
    for _ in range(iterations + 1):
        E = lift(V, N, nc)
        V = np.maximum(L, E)
    return E


def warp(Es, ratio):
    """W[k] = Es at k / ratio, linear between bins, Es[nb - 1] beyond the last"""
    Es = np.asarray(Es, np.float64)
    nb = Es.shape[-1]
    u = np.arange(nb) / float(ratio)
    i = np.floor(u).astype(np.int64)
    f = u - i
    inside = i < nb - 1
    i0 = np.where(inside, i, nb - 2)
    W = (1.0 - f) * Es[..., i0] + f * Es[..., i0 + 1]
    return np.where(inside, W, Es[..., nb - 1:nb])


def gain(W, E, amount, max_gain_db):
    lim = max_gain_db * np.log(10.0) / 20.0
    return np.exp(np.clip(amount * (np.asarray(W, np.float64) - np.asarray(E, np.float64)), -lim, lim))


def energy_scale(a2, g):
    """s (T) in float32 from float32 A2 and g (T, nb): the two sums in double in the defined order (256 partials over the bins
    k = p mod 256 in ascending k, then the partials in ascending p)"""
    a2, g = np.asarray(a2, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    T, nb = a2.shape
    c = np.full(nb, 2.0)
    c[0] = c[nb - 1] = 1.0
    rows = -(-nb // 256)
    t0 = np.zeros((T, rows * 256))
    t1 = np.zeros((T, rows * 256))
    t0[:, :nb] = c * a2
    t1[:, :nb] = c * ((g * g) * a2)
    p0, p1 = np.zeros((T, 256)), np.zeros((T, 256))
    for j in range(rows):
        p0 += t0[:, 256 * j:256 * (j + 1)]
        p1 += t1[:, 256 * j:256 * (j + 1)]
    e0, e1 = np.cumsum(p0, axis=1)[:, -1], np.cumsum(p1, axis=1)[:, -1]      # cumsum adds in ascending order
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e1 == 0.0, 1.0, np.sqrt(e0 / e1)).astype(np.float32)


def synthesis(D32, g, s, n, sr):
    """y in float64 from the float32 D, g (T, nb) and s (T): Y = fl(g s) D, windowed inverse transforms, overlap-add"""
    N, H, nb = geometry(sr)
    T = n // H + 1
    w = window(N).astype(np.float64)
    gs = (np.asarray(g, np.float32) * np.asarray(s, np.float32)[:, None]).astype(np.float32).astype(np.float64)
    Y = gs * np.asarray(D32[:T]).astype(np.complex128)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    num = np.zeros(T * H + N)
    den = np.zeros(T * H + N)
    fr = w * np.fft.irfft(Y, N, axis=-1)
    for t in range(T):
        num[t * H:t * H + N] += fr[t]
        den[t * H:t * H + N] += w * w
    num, den = num[N // 2:N // 2 + n], den[N // 2:N // 2 + n]
    y = np.zeros(n)
    ok = den > 1e-8
    y[ok] = num[ok] / den[ok]
    return y


# ---- the stages whole --------------------------------------------------------------------------------------------------------
def stage(x, sr, src=None, D32=None, **kw):
    """stage 17 on one channel from x alone (or from the float32 spectra D32 of x) -> dict of D, E, Es, g, s, y"""
    v = values(**kw)
    x = np.asarray(x)
    n = x.shape[0]
    N, H, nb = geometry(sr)
    T = n // H + 1
    nc = quefrency_bins(sr, v["quefrency_ms"])
    assert 1 <= nc <= N // 8
    if D32 is None:
        D32 = round_d(analysis(x, sr))[:T]
    E = envelope(log_spectrum(D32), N, nc, v["iterations"])
    if src is None:
        Es = E
    else:
        assert np.asarray(src).shape == x.shape
        Es = envelope(log_spectrum(round_d(analysis(src, sr))[:T]), N, nc, v["iterations"])
    g = gain(warp(Es, v["ratio"]), E, v["amount"], v["max_gain_db"])
    s = energy_scale(a2_of(D32), g) if v["keep_energy"] else np.ones(T, np.float32)
    return dict(D=D32, E=E, Es=Es, g=g, s=s, y=synthesis(D32, g, s, n, sr))


def shift(x, sr, semitones, **kw):
    """a formant shift by semitones; the skip rule included"""
    r = ratio_of(semitones)
    if r == 1.0 or kw.get("amount", 1.0) == 0.0:
        return np.asarray(x, np.float64).copy()
    return stage(x, sr, ratio=r, **kw)["y"]


def pitch_shift_preserved(x, sr, semitones, **kw):
    """stage 18 in float64, one channel"""
    x = np.asarray(x, np.float64)
    if pitch_ratio(sr, semitones) == sr:
        return x.copy()
    y = pitch_shift(x, sr, semitones)
    if kw.get("amount", 1.0) == 0.0:
        return y
    return stage(y, sr, src=x, **dict(kw, ratio=1.0))["y"]


# ---- the links of a library (host twin or device) against the functions above --------------------------------------------------
def new_worst():
    return dict(D=0.0, E=0.0, g=0.0, y=0.0)


def check_links(run, x, sr, worst, source=None, **kw):
    """links 1 - 5 on one channel, each judged on the library's own input; run(x, sr, source, **values) -> (y, taps); worst
    collects the largest figures.  Returns y"""
    v = values(**kw)
    n = x.shape[0]
    N, H, nb = geometry(sr)
    T = frames(n, sr)
    nc = quefrency_bins(sr, v["quefrency_ms"])
    y, t = run(x, sr, source, **kw)
    assert y.shape == (n,) and t["D"].shape == (T, nb, 2) and t["s"].shape == (T,)
    assert all(t[k].shape == (T, nb) for k in ("E", "Es", "g"))
    D32 = pairs_to_complex(t["D"])
    ref_D = analysis(x, sr)[:T]
    top = np.abs(ref_D).max(axis=1)
    err = np.abs(ref_D - D32.astype(np.complex128)).max(axis=1)
    worst["D"] = max(worst["D"], float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0)
    assert not err[top == 0].any()
    worst["E"] = max(worst["E"], float(np.abs(t["E"] - envelope(log_spectrum(D32), N, nc, v["iterations"])).max()))
    if source is None:
        assert np.array_equal(t["Es"], t["E"])
    else:
        Ds = round_d(analysis(source, sr))[:T]
        worst["E"] = max(worst["E"], float(np.abs(t["Es"] - envelope(log_spectrum(Ds), N, nc, v["iterations"])).max()))
    g = gain(warp(t["Es"], v["ratio"]), t["E"], v["amount"], v["max_gain_db"])
    worst["g"] = max(worst["g"], float(np.abs(t["g"] / g - 1.0).max()))
    s = energy_scale(a2_of(D32), t["g"]) if v["keep_energy"] else np.ones(T, np.float32)
    assert np.array_equal(t["s"], s)
    ref = synthesis(D32, t["g"], t["s"], n, sr)
    worst["y"] = max(worst["y"], float(np.abs(y - ref).max()) / max(float(np.abs(x).max()), 1e-30))
    return y


CORNERS = (dict(quefrency_ms=0.125), dict(quefrency_ms=8.0), dict(iterations=0), dict(iterations=16), dict(ratio=0.5),
           dict(ratio=2.0), dict(ratio=1.3, amount=0.5), dict(ratio=0.8, keep_energy=0))


# ---- signals and measures ----------------------------------------------------------------------------------------------------
def vowel(sr, f0, bw, seconds=2.0):
    """an impulse wherever a phase accumulator of f0 / sr crosses an integer, plus 1e-4 Gaussian noise (seed 0), through two
    resonators at 700 and 1500 Hz of bandwidth bw, scaled to peak 0.5"""
    from scipy.signal import lfilter
    n = int(round(seconds * sr))
    ph = np.cumsum(np.full(n, f0 / sr))
    x = (np.floor(ph) > np.floor(ph - f0 / sr)).astype(np.float64)
    x = x + 1e-4 * np.random.default_rng(0).standard_normal(n)
    r = np.exp(-np.pi * bw / sr)
    for f in (700.0, 1500.0):
        x = lfilter([1.0 - r], [1.0, -2.0 * r * np.cos(2.0 * np.pi * f / sr), r * r], x)
    return np.ascontiguousarray(0.5 * x / np.abs(x).max(), dtype=np.float32)


def _segment(y):
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    return y[n // 4:n // 4 + 16384]


def centroid(y, sr):
    """the power-weighted mean of log f over 200 Hz <= f < min(4000, 0.45 sr), exponentiated: 16384 samples from n / 4 under a
    Hann window, zero-padded to 32768"""
    seg = _segment(y)
    P = np.abs(np.fft.rfft(seg * np.hanning(seg.shape[0]), 32768)) ** 2
    f = np.arange(P.shape[0]) * sr / 32768.0
    ok = (f >= 200.0) & (f < min(4000.0, 0.45 * sr))
    return float(np.exp((P[ok] * np.log(f[ok])).sum() / P[ok].sum()))


def f0_of(y, sr):
    """the first autocorrelation peak above 0.8 of the largest within 60 .. 500 Hz, parabolically refined, in Hz"""
    seg = _segment(y)
    m = seg.shape[0]
    S = np.fft.rfft(seg, 2 * m)
    ac = np.fft.irfft(S * np.conj(S))[:m]
    lo, hi = int(np.ceil(sr / 500.0)), int(np.floor(sr / 60.0))
    top = ac[lo:hi + 1].max()
    for k in range(lo, hi + 1):
        if ac[k] >= 0.8 * top and ac[k] > ac[k - 1] and ac[k] >= ac[k + 1]:
            a, b, c = ac[k - 1], ac[k], ac[k + 1]
            return sr / (k + 0.5 * (a - c) / (a - 2.0 * b + c))
    raise AssertionError("no autocorrelation peak within 60 .. 500 Hz")


VOWELS = ((8000, 150.0, 150.0), (16000, 220.0, 250.0), (48000, 110.0, 150.0))
FORMANT_MOVES = (-4.0, 4.0)
KEY_CHANGES = (-5.0, 7.0)


def behaviour(fns, cases=VOWELS):
    """the figures of the behaviour table.  fns: dict of shift(x, sr, semitones), pitch(x, sr, semitones) and preserved(x, sr,
    semitones), each returning a signal of x's length; a missing entry leaves its rows out"""
    out = {}
    for sr, f0, bw in cases:
        x = vowel(sr, f0, bw)
        c_in, f_in, r_in = centroid(x, sr), f0_of(x, sr), rms(x)
        tag = f"{sr}"
        if "shift" in fns:
            for st in FORMANT_MOVES:
                y = np.asarray(fns["shift"](x, sr, st), np.float64)
                out[f"share {tag} {st:+.0f}"] = np.log(centroid(y, sr) / c_in) / np.log(2.0 ** (st / 12.0))
                out[f"shift f0 {tag} {st:+.0f}"] = f0_of(y, sr) - f_in
                out[f"shift level {tag} {st:+.0f}"] = rms(y) / r_in
        for st in KEY_CHANGES:
            if "preserved" in fns:
                y = np.asarray(fns["preserved"](x, sr, st), np.float64)
                out[f"kept centroid {tag} {st:+.0f}"] = centroid(y, sr) / c_in
                out[f"kept f0 {tag} {st:+.0f}"] = f0_of(y, sr) - f_in * 2.0 ** (st / 12.0)
                out[f"kept level {tag} {st:+.0f}"] = rms(y) / r_in
            if "pitch" in fns:
                y = np.asarray(fns["pitch"](x, sr, st), np.float64)
                out[f"plain centroid {tag} {st:+.0f}"] = centroid(y, sr) / c_in
    return out


def check_behaviour(f):
    """the asserted bands of the behaviour table"""
    for k, v in f.items():
        if k.startswith("share"):
            assert 0.7 <= v <= 1.15, (k, v)
        elif k.startswith("shift f0") or k.startswith("kept f0"):
            assert abs(v) <= 0.3, (k, v)
        elif k.startswith("shift level") or k.startswith("kept level"):
            assert 0.97 <= v <= 1.03, (k, v)
        elif k.startswith("kept centroid"):
            assert 0.88 <= v <= 1.08, (k, v)
        elif k.startswith("plain centroid"):
            assert not 0.85 <= v <= 1.3, (k, v)
        else:
            raise AssertionError(k)
