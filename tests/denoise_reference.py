"""float64 restatement of include/rvcx.h stage 15 (noise reduction: a soft spectral gate, from a noise profile or adaptive)
in numpy, written from the definition alone, one function per sub-stage: numpy's rfft / irfft for the transforms, plain
loops over frames for the recurrences and the overlap-add.  Every function can start from its own analysis or from spectra,
smoothed powers, statistics, floors and masks that somebody else computed, so that a test can check the library link by
link.  D and A2 carry the float32 roundings of the definition (they are what the library stores); everything behind them is
float64.  Shared by tests/test_denoise_host.py and tests/test_gpu_denoise.py."""
import numpy as np

from stretch_reference import a2_of, geometry, pairs_to_complex, rms, round_d, window  # noqa: F401  (the tests reach through)

DEFAULTS = dict(mode=1, strength=0.7, n_std=3.0, knee_db=1.0, thresh_mult=1.0, slope=5.0, time_constant_s=2.0,
                freq_smooth_hz=500.0, time_smooth_ms=50.0)
TINY = float(np.float32(1e-20))


def values(**kw):
    """the nine values, each rounded to float32 as the ABI carries them"""
    v = dict(DEFAULTS, **kw)
    v["mode"] = {"profile": 0, "adaptive": 1}.get(v["mode"], v["mode"])
    return {k: (int(x) if k == "mode" else float(np.float32(x))) for k, x in v.items()}


def frames(n, sr):
    return n // geometry(sr)[1] + 1


def half_widths(sr, freq_smooth_hz=500.0, time_smooth_ms=50.0):
    """(nf, nt)"""
    N, H, _ = geometry(sr)
    return (int(np.floor(float(np.float32(freq_smooth_hz)) * N / (2.0 * sr))),
            int(np.floor(float(np.float32(time_smooth_ms)) * sr / (2000.0 * H))))


# ---- analysis --------------------------------------------------------------------------------------------------------------------
def analysis(x, sr):
    """D in complex128, (T, nb): frame t centred at t H, x zero outside the signal"""
    N, H, nb = geometry(sr)
    x = np.asarray(x, np.float64)
    T = x.shape[0] // H + 1
    pad = np.concatenate([np.zeros(N // 2), x, np.zeros(N + H)])
    w = window(N).astype(np.float64)
    D = np.zeros((T, nb), np.complex128)
    for t in range(T):
        D[t] = np.fft.rfft(w * pad[t * H:t * H + N])
    return D


# ---- smoothing -------------------------------------------------------------------------------------------------------------------
def _triangle(a, h, axis):
    """sum over |d| <= h of (h + 1 - |d|) a[i + d] along `axis`, indices inside the array only -> (sums, weight sums)"""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n = a.shape[0]
    out = np.zeros_like(a)
    wsum = np.zeros(n)
    for d in range(-h, h + 1):
        lo, hi = max(0, -d), min(n, n - d)          # i with 0 <= i + d < n
        if lo >= hi:
            continue
        out[lo:hi] += (h + 1 - abs(d)) * a[lo + d:hi + d]
        wsum[lo:hi] += h + 1 - abs(d)
    return np.moveaxis(out, 0, axis), wsum


def smooth(A2, nf, nt):
    """S (T, nb) in float64 from A2 (T, nb): the frequency triangle, then the time triangle, renormalised at the edges"""
    F, wf = _triangle(A2, nf, 1)
    G, wt = _triangle(F, nt, 0)
    return G / (wt[:, None] * wf[None, :])


# ---- mode 0 ----------------------------------------------------------------------------------------------------------------------
def level(S):
    return 10.0 * np.log10(np.asarray(S, np.float64) + TINY)


def profile_stats(S_profile):
    """(mu, sd) per bin: mean and population standard deviation of the level over the profile frames"""
    l = level(S_profile)
    mu = l.mean(axis=0)
    return mu, np.sqrt(((l - mu) ** 2).mean(axis=0))


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def mask_profile(S, mu, sd, n_std, knee_db):
    return sigmoid((level(S) - (mu + n_std * sd)[None, :]) / knee_db)


# ---- mode 1 ----------------------------------------------------------------------------------------------------------------------
def floor_constant(sr, time_constant_s):
    return float(np.exp(-geometry(sr)[1] / (sr * float(time_constant_s))))


def floor(S, c):
    """(f, b), each (T, nb): the forward follower of A = sqrt(S) and the backward follower of f"""
    A = np.sqrt(np.asarray(S, np.float64))
    T = A.shape[0]
    f, b = np.zeros_like(A), np.zeros_like(A)
    run = A[0]
    for t in range(T):
        run = (1.0 - c) * A[t] + c * run
        f[t] = run
    for t in range(T - 1, -1, -1):
        run = (1.0 - c) * f[t] + c * run
        b[t] = run
    return f, b


def mask_adaptive(S, b, thresh_mult, slope):
    A = np.sqrt(np.asarray(S, np.float64))
    return sigmoid(((A - b) / (b + 1e-10) - thresh_mult) * slope)


# ---- synthesis -------------------------------------------------------------------------------------------------------------------
def synthesis(D, m, strength, n, sr):
    """y (n) in float64 from D (T, nb complex) and the mask"""
    N, H, nb = geometry(sr)
    T = D.shape[0]
    w = window(N).astype(np.float64)
    g = 1.0 - strength * (1.0 - np.asarray(m, np.float64))
    num = np.zeros(T * H + N)
    den = np.zeros(T * H + N)
    for t in range(T):
        num[t * H:t * H + N] += w * np.fft.irfft(g[t] * np.asarray(D[t], np.complex128), N)
        den[t * H:t * H + N] += w * w
    num, den = num[N // 2:N // 2 + n], den[N // 2:N // 2 + n]
    y = np.zeros(n)
    ok = den > 1e-8
    y[ok] = num[ok] / den[ok]
    return y


# ---- the stage whole -------------------------------------------------------------------------------------------------------------
def smoothed(x, sr, v, D32=None):
    """(D32, S) of one signal"""
    if D32 is None:
        D32 = round_d(analysis(x, sr))
    nf, nt = half_widths(sr, v["freq_smooth_hz"], v["time_smooth_ms"])
    return D32, smooth(a2_of(D32), nf, nt)


def denoise(x, sr, noise=None, D32=None, S=None, S_profile=None, mu=None, sd=None, b=None, m=None, **kw):
    """stage 15 on one channel from x alone, or from whatever of D32 (T, nb complex64), S, S_profile, mu, sd, b and m is
    given -> dict of every intermediate and y (float64)"""
    v = values(**kw)
    n = np.asarray(x).shape[0]
    if D32 is None or S is None:
        D32, S0 = smoothed(x, sr, v, D32)
        S = S0 if S is None else S
    out = dict(D=D32, S=S)
    if m is None:
        if v["mode"] == 0:
            if mu is None or sd is None:
                if S_profile is None:
                    S_profile = S if noise is None else smoothed(noise, sr, v)[1]
                mu, sd = profile_stats(S_profile)
            out.update(mu=mu, sd=sd)
            m = mask_profile(S, mu, sd, v["n_std"], v["knee_db"])
        else:
            if b is None:
                b = floor(S, floor_constant(sr, v["time_constant_s"]))[1]
            out.update(b=b)
            m = mask_adaptive(S, b, v["thresh_mult"], v["slope"])
    out.update(m=m, y=synthesis(D32, m, v["strength"], n, sr))
    return out


# ---- what the two test files share: signals and measures -------------------------------------------------------------------------
def tone_in_noise(sr, seconds=4.0, seed=0, tone=0.25, noise=0.01, gate=None):
    """(x, clean, hiss): 440 Hz + white noise; gate = (on_seconds, period_seconds) switches the tone"""
    n = int(seconds * sr)
    t = np.arange(n) / sr
    clean = tone * np.sin(2 * np.pi * 440.0 * t)
    if gate is not None:
        clean = clean * ((t % gate[1]) < gate[0])
    hiss = noise * np.random.default_rng(seed).standard_normal(n)
    return clean + hiss, clean, hiss


def project(y, s):
    """(gain of s in y, what is left of y): y = a s + e with e orthogonal to s"""
    y, s = np.asarray(y, np.float64), np.asarray(s, np.float64)
    a = float(np.dot(y, s) / np.dot(s, s))
    return a, y - a * s


def db(a):
    return 20.0 * np.log10(max(float(a), 1e-300))


def behaviour(fn, sr):
    """The conditions of the issue, measured on `fn(x, sr, noise=None, **values)` -> y (strength 1, the defaults otherwise).
    Returns a dict of figures."""
    out = {}
    n = 4 * sr
    mid = slice(sr, 3 * sr)
    # mode 0 with a 1 s independent clip: level kept, SNR gained (middle 2 s)
    x, clean, hiss = tone_in_noise(sr, seed=0)
    clip = 0.01 * np.random.default_rng(1).standard_normal(sr)
    y = np.asarray(fn(x, sr, noise=clip, mode=0, strength=1.0), np.float64)
    a, e = project(y[mid], clean[mid])
    out["level"] = a
    out["snr_in_db"] = db(rms(clean[mid]) / rms(hiss[mid]))
    out["snr_out_db"] = db(a * rms(clean[mid]) / rms(e))
    # mode 0 on noise only
    y = np.asarray(fn(hiss, sr, noise=clip, mode=0, strength=1.0), np.float64)
    out["noise_only_db"] = db(rms(hiss[mid]) / rms(y[mid]))
    # mode 1 with the tone on for the first 0.25 s of every second
    x, clean, hiss = tone_in_noise(sr, seed=0, gate=(0.25, 1.0))
    y = np.asarray(fn(x, sr, mode=1, strength=1.0), np.float64)
    t = (np.arange(n) / sr) % 1.0
    quiet, burst = (t >= 0.45) & (t < 0.9), (t >= 0.05) & (t < 0.2)
    out["quiet_db"] = db(rms(x[quiet]) / rms(y[quiet]))
    out["burst"] = rms(y[burst]) / rms(x[burst])
    # mode 1 on a steady tone: it becomes the floor (the documented property of the mode)
    x, clean, hiss = tone_in_noise(sr, seed=0)
    y = np.asarray(fn(x, sr, mode=1, strength=1.0), np.float64)
    out["steady"] = rms(y[mid]) / rms(x[mid])
    return out


# the bars of the issue: conditions, not device tolerances
def check_behaviour(f):
    assert 0.99 <= f["level"] <= 1.01, f
    assert f["snr_out_db"] - f["snr_in_db"] >= 6.0, f
    assert f["noise_only_db"] >= 12.0, f
    assert f["quiet_db"] >= 30.0, f
    assert f["burst"] >= 0.7, f
    assert f["steady"] <= 0.05, f
