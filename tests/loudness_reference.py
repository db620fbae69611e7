"""float64 restatement of include/rvcx.h stages 9 - 12 (loudness, true peak, limiter) in numpy / scipy, written from the
definitions alone: scipy.signal.lfilter for the K-weighting filter, plain sums for blocks and gates, a direct convolution for
the interpolator.  Shared by tests/test_loudness_host.py and tests/test_gpu_loudness.py."""
import numpy as np
from scipy import signal, special

TABLE_48K = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                      1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])


def kweight_coeffs(sr):
    """{shelf b0, b1, b2, a1, a2, high-pass b0, b1, b2, a1, a2}"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp, np.float64)


def _planar(x):
    x = np.asarray(x, np.float64)
    return x[:, None] if x.ndim == 1 else x


def lufs_of(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def loudness(x, sr):
    """-> (L, momentary l[j]) in float64; L = -inf without a block or when none passes"""
    x = _planar(x)
    c = kweight_coeffs(sr)
    h = sr // 10
    nh = x.shape[0] // h
    nb = nh - 3
    if nb < 1:
        return -np.inf, np.zeros(0)
    y = signal.lfilter(c[0:3], [1.0, c[3], c[4]], x, axis=0)
    y = signal.lfilter(c[5:8], [1.0, c[8], c[9]], y, axis=0)
    hops = (y[:nh * h] ** 2).reshape(nh, h, -1).sum(axis=1)          # (nh, C)
    z = (hops[0:nb] + hops[1:nb + 1] + hops[2:nb + 2] + hops[3:nb + 3]).sum(axis=1) / (4.0 * h)
    l = lufs_of(z)
    keep = l > -70.0
    if not keep.any():
        return -np.inf, l
    gamma = lufs_of(z[keep].mean()) - 10.0
    keep &= l > gamma
    return (float(lufs_of(z[keep].mean())) if keep.any() else -np.inf), l


def interp_taps():
    """(4, 24) float64: row p holds h(m + p / 4) for m = -12 .. 11 (row 0: the unit sample at m = 0)"""
    m = np.arange(-12, 12, dtype=np.float64)
    rows = []
    for p in range(4):
        t = m + p / 4.0
        w = np.where(np.abs(t) < 12.0, special.i0(9.0 * np.sqrt(np.maximum(0.0, 1.0 - (t / 12.0) ** 2))) / special.i0(9.0), 0.0)
        rows.append(np.sinc(t) * w)
    return np.array(rows)


def oversample4(x):
    """x (n,) -> y (4 n,): y[4 n + p] = sum_m x[n - m] h(m + p / 4)"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    taps = interp_taps()
    y = np.zeros((n, 4))
    xp = np.concatenate([np.zeros(12), x, np.zeros(12)])
    for p in range(4):
        for k, m in enumerate(range(-12, 12)):
            y[:, p] += taps[p, k] * xp[12 - m:12 - m + n]
    return y.reshape(-1)


def true_peak(x):
    """-> (dBTP, p[n]) in float64"""
    x = _planar(x)
    p = np.zeros(x.shape[0])
    for c in range(x.shape[1]):
        p = np.maximum(p, np.abs(oversample4(x[:, c])).reshape(-1, 4).max(axis=1))
    top = p.max() if p.size else 0.0
    return (20.0 * np.log10(top) if top > 0 else -np.inf), p


def sine(freq, seconds, sr, dbfs, phase=0.0, channels=2):
    t = np.arange(int(round(seconds * sr)), dtype=np.float64) / sr
    s = 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t + phase)
    return np.stack([s] * channels, axis=1).astype(np.float32)


def ebu_case(k, sr=48000):
    """EBU Tech 3341 cases 1 - 5 from 1 kHz stereo sines -> (signal, expected LUFS)"""
    segs = {1: [(20, -23)], 2: [(20, -33)], 3: [(10, -36), (60, -23), (10, -36)],
            4: [(10, -72), (10, -36), (60, -23), (10, -36), (10, -72)], 5: [(20, -26), (20.1, -20), (20, -26)]}[k]
    return np.concatenate([sine(1000.0, s, sr, db) for s, db in segs]), (-33.0 if k == 2 else -23.0)


def limiter_signal(sr, seconds=1.0, seed=5):
    """noise plus a 220 Hz tone with planted spikes (one at n = 3, one in the last samples), mono float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    x = 0.2 * rng.standard_normal(n) + 0.4 * np.sin(2 * np.pi * 220.0 * t)
    for at, v in ((3, 1.7), (n // 3, -2.5), (n // 2, 1.2), (n // 2 + 5, -1.4), (n - 7, 1.9)):
        x[at] = v
    return x.astype(np.float32)
