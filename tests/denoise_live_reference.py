"""float64 restatement of include/rvcx.h stage 16 (live noise reduction: the causal soft spectral gate of a live-stream
session) in numpy, written from the definition alone: numpy's rfft / irfft for the transforms, plain loops over frames for
the recurrences and the overlap-add.  The signal is taken whole; a stream that has received n samples has emitted the first n
samples of what this returns.  D and A2 carry the float32 roundings of the definition (they are what the library stores);
everything behind them is float64.  Shared by tests/test_denoise_live_host.py and tests/test_gpu_stream_denoise.py."""
import numpy as np

DEFAULTS = dict(mode=1, strength=0.9, n_std=3.0, knee_db=1.0, thresh_mult=1.0, slope=5.0, time_constant_s=2.0,
                fall_time_s=0.2, freq_smooth_hz=500.0, time_smooth_ms=50.0)
TINY = float(np.float32(1e-20))


def values(**kw):
    """the ten values, each rounded to float32 as the ABI carries them"""
    v = dict(DEFAULTS, **kw)
    v["mode"] = {"profile": 0, "adaptive": 1}.get(v["mode"], v["mode"])
    return {k: (int(x) if k == "mode" else float(np.float32(x))) for k, x in v.items()}


def geometry(sr):
    """(N, H, nb): the smallest power of two with 48 N >= sr, never below 512"""
    N = 512
    while 48 * N < sr:
        N *= 2
    return N, N // 4, N // 2 + 1


def window(N):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)


def frames(n, sr):
    """frames complete once n samples have arrived: frame t needs the samples below t H + N / 2"""
    N, H, _ = geometry(sr)
    return 0 if n < N // 2 else (n - N // 2) // H + 1


def half_widths(sr, freq_smooth_hz=500.0, time_smooth_ms=50.0):
    """(nf, nt)"""
    N, H, _ = geometry(sr)
    return (int(np.floor(float(np.float32(freq_smooth_hz)) * N / (2.0 * sr))),
            int(np.floor(float(np.float32(time_smooth_ms)) * sr / (1000.0 * H))))


def rms(a):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a)).astype(np.float64) ** 2)))


def rel(a, b):
    """relative RMS distance of a from b"""
    return rms(np.asarray(a) - np.asarray(b)) / max(rms(b), 1e-300)


# ---- analysis --------------------------------------------------------------------------------------------------------------------
def analysis(x, sr):
    """D in complex128, (T, nb): frame t centred at t H, x zero in front of sample 0, the frames complete in x only"""
    N, H, nb = geometry(sr)
    x = np.asarray(x, np.float64)
    T = frames(x.shape[0], sr)
    pad = np.concatenate([np.zeros(N // 2), x])
    w = window(N).astype(np.float64)
    D = np.zeros((T, nb), np.complex128)
    for t in range(T):
        D[t] = np.fft.rfft(w * pad[t * H:t * H + N])
    return D


def round_d(D):
    """the float32 pairs the library stores, as complex128"""
    return np.asarray(D).astype(np.complex64).astype(np.complex128)


def a2_of(D32):
    """A2 = fl(fl(re re) + fl(im im)) in float32, returned as float64"""
    re, im = np.real(D32).astype(np.float32), np.imag(D32).astype(np.float32)
    return (re * re + im * im).astype(np.float64)


# ---- smoothing -------------------------------------------------------------------------------------------------------------------
def smooth(A2, nf, nt):
    """S (T, nb): the frequency triangle over the bins inside the grid, then the time triangle over the past side, each
    divided by the weights of the indices it summed"""
    A2 = np.asarray(A2, np.float64)
    T, nb = A2.shape
    F = np.zeros_like(A2)
    wf = np.zeros(nb)
    for d in range(-nf, nf + 1):
        lo, hi = max(0, -d), min(nb, nb - d)
        F[:, lo:hi] += (nf + 1 - abs(d)) * A2[:, lo + d:hi + d]
        wf[lo:hi] += nf + 1 - abs(d)
    S = np.zeros_like(A2)
    for t in range(T):
        tot, wt = np.zeros(nb), 0.0
        for dt in range(-nt, 1):
            if t + dt >= 0:
                tot += (nt + 1 + dt) * F[t + dt]
                wt += nt + 1 + dt
        S[t] = tot / (wt * wf)
    return S


# ---- mode 0 ----------------------------------------------------------------------------------------------------------------------
def level(S):
    return 10.0 * np.log10(np.asarray(S, np.float64) + TINY)


def profile_stats(S_profile):
    l = level(S_profile)
    mu = l.mean(axis=0)
    return mu, np.sqrt(((l - mu) ** 2).mean(axis=0))


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def mask_profile(S, mu, sd, n_std, knee_db):
    return sigmoid((level(S) - (mu + n_std * sd)[None, :]) / knee_db)


# ---- mode 1 ----------------------------------------------------------------------------------------------------------------------
def floor_constants(sr, time_constant_s, fall_time_s):
    H = geometry(sr)[1]
    return float(np.exp(-H / (sr * float(time_constant_s)))), float(np.exp(-H / (sr * float(fall_time_s))))


def floor(S, c_up, c_dn):
    """f (T, nb): forward only, rising with c_up, falling with c_dn, f[-1] = A[0]"""
    A = np.sqrt(np.asarray(S, np.float64))
    f = np.zeros_like(A)
    prev = A[0].copy() if A.shape[0] else None
    for t in range(A.shape[0]):
        c = np.where(A[t] >= prev, c_up, c_dn)
        prev = (1.0 - c) * A[t] + c * prev
        f[t] = prev
    return f


def mask_adaptive(S, f, thresh_mult, slope):
    A = np.sqrt(np.asarray(S, np.float64))
    return sigmoid(((A - f) / (f + 1e-10) - thresh_mult) * slope)


# ---- synthesis -------------------------------------------------------------------------------------------------------------------
def synthesis(D, m, strength, n, sr):
    """what the stream has emitted after n samples: y (n) in float64, y[i + N] = the overlap-add at sample i"""
    N, H, nb = geometry(sr)
    T = D.shape[0]
    w = window(N).astype(np.float64)
    g = 1.0 - strength * (1.0 - np.asarray(m, np.float64))
    num = np.zeros(T * H + N)
    den = np.zeros(T * H + N)
    for t in range(T):
        num[t * H:t * H + N] += w * np.fft.irfft(g[t] * np.asarray(D[t], np.complex128), N)
        den[t * H:t * H + N] += w * w
    y = np.zeros(n)
    k = max(n - N, 0)                  # samples 0 .. n - N - 1 have left: every frame that covers them is among the T
    if k:
        y[N:] = num[N // 2:N // 2 + k] / den[N // 2:N // 2 + k]
    return y


# ---- the stage whole -------------------------------------------------------------------------------------------------------------
def smoothed(x, sr, v, D32=None):
    """(D32, S) of one signal"""
    if D32 is None:
        D32 = round_d(analysis(x, sr))
    nf, nt = half_widths(sr, v["freq_smooth_hz"], v["time_smooth_ms"])
    return D32, smooth(a2_of(D32), nf, nt)


def denoise_live(x, sr, noise=None, **kw):
    """stage 16 on one channel, the signal whole -> dict of D, S, f (mode 1) or mu, sd (mode 0), m and y (float64)"""
    v = values(**kw)
    x = np.asarray(x)
    n = x.shape[0]
    D32, S = smoothed(x, sr, v)
    out = dict(D=D32, S=S)
    if v["mode"] == 0:
        mu, sd = profile_stats(smoothed(noise, sr, v)[1])
        out.update(mu=mu, sd=sd)
        m = mask_profile(S, mu, sd, v["n_std"], v["knee_db"])
    else:
        f = floor(S, *floor_constants(sr, v["time_constant_s"], v["fall_time_s"]))
        out.update(f=f)
        m = mask_adaptive(S, f, v["thresh_mult"], v["slope"])
    N = geometry(sr)[0]
    if v["strength"] == 0.0:
        y = np.zeros(n)
        y[N:] = np.asarray(x, np.float64)[:max(n - N, 0)]
    else:
        y = synthesis(D32, m, v["strength"], n, sr)
    out.update(m=m, y=y)
    return out


# ---- what the two test files share: the behaviour signal and its measures ----------------------------------------------------------
def bursts_in_noise(sr, seconds=4.0, seed=0, tone=0.25, noise=0.01, gate=(0.25, 1.0)):
    """0.25 sin 440 Hz, on for the first 0.25 s of every second, + 0.01 white noise (stage 15's test signal)"""
    n = int(seconds * sr)
    t = np.arange(n) / sr
    clean = tone * np.sin(2 * np.pi * 440.0 * t) * ((t % gate[1]) < gate[0])
    hiss = noise * np.random.default_rng(seed).standard_normal(n)
    return clean + hiss


def db(a):
    return 20.0 * np.log10(max(float(a), 1e-300))


def behaviour(fn, sr, **kw):
    """(attenuation of the pauses in dB, level of the bursts out / in) after the first second, on fn(x, sr, **kw) -> y
    delayed by N"""
    x = bursts_in_noise(sr)
    N = geometry(sr)[0]
    y = np.asarray(fn(x.astype(np.float32), sr, **kw), np.float64)[N:]
    x = x[:x.shape[0] - N]
    t = (np.arange(x.shape[0]) / sr)
    late = t >= 1.0
    quiet, burst = late & ((t % 1.0) >= 0.45) & ((t % 1.0) < 0.9), late & ((t % 1.0) >= 0.05) & ((t % 1.0) < 0.2)
    return db(rms(x[quiet]) / rms(y[quiet])), rms(y[burst]) / rms(x[burst])
