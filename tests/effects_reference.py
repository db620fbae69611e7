"""Float64 numpy restatement of the post-production stages defined in include/rvcx.h ("post-production"): the yardstick of
tests/test_effects_host.py and tests/test_gpu_effects.py.  Every function works on one channel (1-D float64) unless it says
otherwise, takes the float32 coefficients the library uses (widened) where a test wants to separate coefficient rounding
from arithmetic, and keeps all state zero at sample 0.  test_effects_host.py pins the linear ones on scipy.signal.lfilter."""
import numpy as np
from scipy.signal import lfilter

COMB = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS = (556, 441, 341, 225)


def f32v(v):
    """the double a float32 argument of the C ABI carries"""
    return float(np.float32(v))


def cte(ms, sr):
    return 0.0 if ms < 1e-3 else float(np.exp(-2.0 * np.pi * 1000.0 / (ms * sr)))


def delay(sr, D):
    return int(sr) * int(D) // 44100


def highpass_coeffs(sr, fc=50.0):
    k = np.tan(np.pi * fc / sr)
    b0 = 1.0 / (k + 1.0)
    return np.array([b0, -b0, 0.0, (k - 1.0) / (k + 1.0), 0.0])


def shelf_coeffs(sr, gain_db, high, fc=440.0, Q=2.0 ** -0.5):
    A = 10.0 ** (gain_db / 40.0)
    w = 2.0 * np.pi * fc / sr
    cs, beta = np.cos(w), np.sin(w) * np.sqrt(A) / Q
    if not high:
        b = [A * ((A + 1) - (A - 1) * cs + beta), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - beta)]
        a = [(A + 1) + (A - 1) * cs + beta, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - beta]
    else:
        b = [A * ((A + 1) + (A - 1) * cs + beta), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - beta)]
        a = [(A + 1) - (A - 1) * cs + beta, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - beta]
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def biquad(x, c):
    """transposed direct form II with c = {b0, b1, b2, a1, a2}, sample by sample"""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    y = np.empty(len(x))
    s1 = s2 = 0.0
    for i, v in enumerate(np.asarray(x, np.float64)):
        o = b0 * v + s1
        s1 = b1 * v - a1 * o + s2
        s2 = b2 * v - a2 * o
        y[i] = o
    return y


def follower(x, c_att, c_rel, square=False, sqrt_out=False):
    a = np.asarray(x, np.float64)
    a = a * a if square else np.abs(a)
    out = np.empty(len(a))
    e = 0.0
    for i, v in enumerate(a.tolist()):
        e = v + (c_att if v > e else c_rel) * (e - v)
        out[i] = e
    return np.sqrt(out) if sqrt_out else out


def compressor(x, sr, ratio, thr_db, attack_ms=1.0, release_ms=100.0, c=None):
    """-> (y, envelope); c: (c_attack, c_release) to use instead of cte() (the library's float32 constants)"""
    x = np.asarray(x, np.float64)
    if ratio == 1:
        return x.copy(), np.zeros(len(x))
    ca, cr = c if c is not None else (cte(attack_ms, sr), cte(release_ms, sr))
    e = follower(x, ca, cr)
    thr = 10.0 ** (thr_db / 20.0)
    g = np.where(e < thr, 1.0, np.power(np.maximum(e, 1e-300) / thr, 1.0 / ratio - 1.0))
    return x * g, e


def gate(x, sr, thr_db, ratio, attack_ms, release_ms, c=None):
    """-> (y, envelope); c: (c0, c50, c_attack, c_release)"""
    x = np.asarray(x, np.float64)
    if ratio == 1:
        return x.copy(), np.zeros(len(x))
    c0, c50, ca, cr = c if c is not None else (cte(0.0, sr), cte(50.0, sr), cte(attack_ms, sr), cte(release_ms, sr))
    r = follower(x, c0, c50, square=True, sqrt_out=True)
    e = follower(r, ca, cr)
    thr = 10.0 ** (thr_db / 20.0)
    g = np.where(e > thr, 1.0, np.power(e / thr, ratio - 1.0))
    return x * g, e


def comb(x, D, fb, d):
    """o = buf[i]; last = o (1 - d) + last d; buf[i] = in + last fb -- block by block: inside a block of D samples o is known,
    `last` is the one-pole (1 - d) / (1 - d z^-1) over it (lfilter, carried across blocks), the writes are element-wise.
    test_effects_host.py pins the whole against the comb's own sparse transfer function."""
    x = np.asarray(x, np.float64)
    n = len(x)
    buf, out, zi = np.zeros(D), np.empty(n), np.zeros(1)
    for j in range(0, n, D):
        m = min(D, n - j)
        o = buf[:m].copy()
        ls, zi = lfilter([1.0 - d], [1.0, -d], o, zi=zi)
        buf[:m] = x[j:j + m] + ls * fb
        out[j:j + m] = o
    return out


def allpass(x, D):
    x = np.asarray(x, np.float64)
    n = len(x)
    buf, out = np.zeros(D), np.empty(n)
    for j in range(0, n, D):
        m = min(D, n - j)
        v = buf[:m].copy()
        buf[:m] = x[j:j + m] + 0.5 * v
        out[j:j + m] = v - x[j:j + m]
    return out


def reverb(x, sr, room, damping, wet, dry, width):
    """x (frames, 2) -> (frames, 2)"""
    x = np.asarray(x, np.float64)
    inp = 0.015 * (x[:, 0] + x[:, 1])
    fb, d = 0.28 * room + 0.7, 0.4 * damping
    o = []
    for side in range(2):
        acc = np.zeros(len(inp))
        for D in COMB:
            acc = acc + comb(inp, delay(sr, D + 23 * side), fb, d)
        for D in ALLPASS:
            acc = allpass(acc, delay(sr, D + 23 * side))
        o.append(acc)
    w1, w2 = 1.5 * wet * (1.0 + width), 1.5 * wet * (1.0 - width)
    return np.stack([o[0] * w1 + o[1] * w2 + 2.0 * dry * x[:, 0], o[1] * w1 + o[0] * w2 + 2.0 * dry * x[:, 1]], axis=1)


def chorus_tau(n, sr, rate, depth, centre_ms):
    return sr / 1000.0 * np.maximum(1.0, centre_ms + 10.0 * depth * np.sin(2.0 * np.pi * rate * n / sr))


def _tap(d, pos):
    i0 = np.floor(pos).astype(np.int64)
    fr = pos - i0
    d0 = np.where(i0 >= 0, d[np.maximum(i0, 0)], 0.0)
    d1 = np.where(i0 + 1 >= 0, d[np.maximum(i0 + 1, 0)], 0.0)
    return d0 + fr * (d1 - d0)


def chorus(x, sr, rate, depth, centre_ms, feedback, mix):
    x = np.asarray(x, np.float64)
    n = len(x)
    if mix == 0:
        return x.copy()
    idx = np.arange(n, dtype=np.float64)
    pos = idx - chorus_tau(idx, sr, rate, depth, centre_ms)
    if feedback == 0:
        w = _tap(x, pos)
    else:
        T = int(np.floor(sr / 1000.0 * max(1.0, centre_ms - abs(10.0 * depth)))) - 1
        d, w = np.zeros(n), np.empty(n)
        for j in range(0, n, T):
            k = min(j + T, n)
            w[j:k] = _tap(d, pos[j:k])
            d[j:k] = x[j:k] + feedback * w[j:k]
    return (1.0 - mix) * x + mix * w


def chain(x, sr, p):
    """the board on x (frames, 2); p: dict of the eighteen add_effects values (as the doubles the ABI's floats carry)"""
    x = np.asarray(x, np.float64)
    y = np.stack([biquad(x[:, c], highpass_coeffs(sr)) for c in range(2)], axis=1)
    y = np.stack([compressor(y[:, c], sr, p["compressor_ratio"], p["compressor_threshold"])[0] for c in range(2)], axis=1)
    y = np.stack([gate(y[:, c], sr, p["noise_gate_threshold"], p["noise_gate_ratio"], p["noise_gate_attack"],
                       p["noise_gate_release"])[0] for c in range(2)], axis=1)
    y = reverb(y, sr, p["reverb_rm_size"], p["reverb_damping"], p["reverb_wet"], p["reverb_dry"], p["reverb_width"])
    for key, high in (("low_shelf_gain", False), ("high_shelf_gain", True)):
        if p[key] != 0:
            y = np.stack([biquad(y[:, c], shelf_coeffs(sr, p[key], high)) for c in range(2)], axis=1)
    return np.stack([chorus(y[:, c], sr, p["chorus_rate_hz"], p["chorus_depth"], p["chorus_centre_delay_ms"],
                            p["chorus_feedback"], p["chorus_mix"]) for c in range(2)], axis=1)


def mix(vocal, inst, vocal_gain_db, inst_gain_db):
    """pydub: apply_gain is floor(s * 10^(dB / 20)) clipped to int16, overlay a saturating add over the vocal's length"""
    v, m = np.asarray(vocal, np.int64), np.asarray(inst, np.int64)
    pad = np.zeros_like(v)
    k = min(len(v), len(m))
    pad[:k] = m[:k]
    gv, gi = 10.0 ** (f32v(vocal_gain_db) / 20.0), 10.0 ** (f32v(inst_gain_db) / 20.0)
    a = np.clip(np.floor(v * gv), -32768, 32767).astype(np.int64)
    b = np.clip(np.floor(pad * gi), -32768, 32767).astype(np.int64)
    return np.clip(a + b, -32768, 32767).astype(np.int16)


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))
