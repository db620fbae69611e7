"""float64 restatement of include/rvcx.h stages 13 and 14 (time stretch by a phase-locked vocoder on integer phases, pitch
shift) in numpy, written from the definition alone, one function per sub-stage: numpy's rfft / irfft for the transforms,
plain loops over frames for the recurrence and the overlap-add, oracle.audio.resample_kaiser_hq for the resampler.  Every
function can start from its own analysis or from spectra, owners and phases that somebody else computed, so that a test can
check the library link by link.  Shared by tests/test_pitch_host.py and tests/test_gpu_pitch.py."""
import numpy as np


def geometry(sr):
    """(N, H, nb): N the smallest power of two with 24 N >= sr"""
    N = 2
    while 24 * N < sr:
        N *= 2
    return N, N // 4, N // 2 + 1


def window(N):
    """w in float32, formed in double and rounded once"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)


def stretch_len(n, P, Q):
    return (n * P + Q // 2) // Q


def frames(n, sr, P, Q):
    """(T, J)"""
    T = n // geometry(sr)[1] + 1
    return T, -(-T * P // Q)


def pitch_ratio(sr, s):
    return int(np.floor(sr * 2.0 ** (s / 12.0) + 0.5))


# ---- 13.1 ------------------------------------------------------------------------------------------------------------------
def analysis(x, sr):
    """D in complex128, (T + 2, nb): frames T and T + 1 are zero"""
    N, H, nb = geometry(sr)
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    T = n // H + 1
    pad = np.concatenate([np.zeros(N // 2), x, np.zeros(N + H)])
    w = window(N).astype(np.float64)
    D = np.zeros((T + 2, nb), np.complex128)
    for t in range(T):
        D[t] = np.fft.rfft(w * pad[t * H:t * H + N])
    return D


def round_d(D):
    """what the library stores: float32 pairs"""
    return np.asarray(D).astype(np.complex64)


def pairs_to_complex(Dp):
    """(.., nb, 2) float32 pairs -> complex64"""
    Dp = np.asarray(Dp, np.float32)
    return (Dp[..., 0] + 1j * Dp[..., 1]).astype(np.complex64)


# ---- 13.2 ------------------------------------------------------------------------------------------------------------------
def a2_of(D32):
    """A2 = fl(fl(re re) + fl(im im)) in float32: two products, one sum, each rounded"""
    re, im = np.real(D32).astype(np.float32), np.imag(D32).astype(np.float32)
    return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def th_of(D32, as_float32=True):
    """TH in units of 2^-32 turn (uint32) from float64 atan2 of the float32 D.  as_float32: the angle is rounded to float32
    first (what a correctly rounded atan2f returns), else kept in double"""
    re, im = np.real(D32).astype(np.float64), np.imag(D32).astype(np.float64)
    ang = np.arctan2(im, re)
    if as_float32:
        ang = ang.astype(np.float32).astype(np.float64)
    u = np.rint(ang * (2.0 ** 31 / np.pi)).astype(np.int64) % (1 << 32)
    return np.where(a2_of(D32) == 0, 0, u).astype(np.uint32)


def peaks_of(a2):
    """peak flags of one frame"""
    a2 = np.asarray(a2, np.float32)
    nb = a2.shape[0]
    big = np.full(nb + 4, -1.0, np.float64)                # a neighbour outside counts as smaller (A2 >= 0 > -1)
    big[2:nb + 2] = a2
    c = big[2:nb + 2]
    return (c > 0) & (c > big[1:nb + 1]) & (c > big[0:nb]) & (c >= big[3:nb + 3]) & (c >= big[4:nb + 4])


def own_of(a2):
    """own of one frame: the nearest peak, the lower one at equal distance; identity without a peak"""
    pk = np.flatnonzero(peaks_of(a2))
    k = np.arange(np.asarray(a2).shape[0])
    if pk.size == 0:
        return k.astype(np.int32)
    dist = np.abs(k[:, None] - pk[None, :])
    return pk[np.argmin(dist, axis=1)].astype(np.int32)      # argmin takes the first, that is the lower, of equal distances


def owners(D32):
    a2 = a2_of(D32)
    return np.stack([own_of(a2[t]) for t in range(a2.shape[0])])


# ---- 13.3 ------------------------------------------------------------------------------------------------------------------
def scan(own, TH, J, P, Q):
    """R (J, nb) in uint32 by the recurrence, frame after frame, on integers"""
    own = np.asarray(own, np.int64)
    TH = np.asarray(TH, np.int64)
    nb = own.shape[1]
    R = np.zeros((J, nb), np.int64)
    for j in range(J - 1):
        tj, tj1 = j * Q // P, (j + 1) * Q // P
        p = own[tj1]
        R[j + 1] = (R[j][own[tj][p]] + TH[tj + 1][p] - TH[tj1][p]) % (1 << 32)
    return R.astype(np.uint32)


# ---- 13.4 ------------------------------------------------------------------------------------------------------------------
def synthesis(A, TH, R, n, sr, P, Q):
    """y in float64 from A (T + 2, nb), TH and R"""
    N, H, nb = geometry(sr)
    J = R.shape[0]
    ns = stretch_len(n, P, Q)
    w = window(N).astype(np.float64)
    A = np.asarray(A, np.float64)
    num = np.zeros(J * H + N)
    den = np.zeros(J * H + N)
    for j in range(J):
        tj, f = j * Q // P, (j * Q % P) / P
        M = (1.0 - f) * A[tj] + f * A[tj + 1]
        phi = (np.asarray(R[j], np.int64) + np.asarray(TH[tj], np.int64)) % (1 << 32)
        ang = phi.astype(np.uint32).astype(np.int32).astype(np.float64) * (np.pi / 2.0 ** 31)
        fr = w * np.fft.irfft(M * np.exp(1j * ang), N)
        num[j * H:j * H + N] += fr
        den[j * H:j * H + N] += w * w
    num, den = num[N // 2:], den[N // 2:]
    y = np.zeros(ns)
    m = min(ns, num.shape[0])
    ok = den[:m] > 1e-8
    y[:m][ok] = num[:m][ok] / den[:m][ok]
    return y


# ---- the stages whole --------------------------------------------------------------------------------------------------------
def stretch(x, sr, P, Q, D32=None, own=None, TH=None, R=None):
    """stage 13 from x alone, or from whatever of D32 (T + 2, nb complex64), own, TH and R is given -> dict"""
    n = np.asarray(x).shape[0]
    T, J = frames(n, sr, P, Q)
    if D32 is None:
        D32 = round_d(analysis(x, sr))
    if own is None:
        own = owners(D32)
    if TH is None:
        TH = th_of(D32)
    if R is None:
        R = scan(own, TH, J, P, Q)
    A = np.sqrt(a2_of(D32))                                 # float32 square root of the float32 A2
    return dict(D=D32, own=own, TH=TH, R=R, y=synthesis(A, TH, R, n, sr, P, Q))


def pitch_shift(x, sr, s):
    """stage 14 in float64, one channel"""
    from oracle.audio import resample_kaiser_hq
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    P = pitch_ratio(sr, s)
    if P == sr:
        return x.copy()
    y = resample_kaiser_hq(stretch(x, sr, P, sr)["y"], P, sr)
    out = np.zeros(n)
    m = min(n, y.shape[0])
    out[:m] = y[:m]
    return out


# ---- what the two test files share: signals and measures ------------------------------------------------------------------------
def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def signal(n, seed, sr=8000):
    """a few partials with slow vibrato plus a little noise, peak 0.5"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * (f * t + 0.3 * np.sin(2 * np.pi * 3.0 * t)) + p)
            for f, a, p in zip(rng.uniform(100, 0.4 * sr, 5), rng.uniform(0.2, 1.0, 5), rng.uniform(0, 6.28, 5)))
    x = x + 0.01 * rng.standard_normal(n)
    return np.ascontiguousarray(0.5 * x / max(np.abs(x).max(), 1e-9), dtype=np.float32)


def tones(n=16000, sr=8000):
    t = np.arange(n) / sr
    return dict(sine=0.5 * np.sin(2 * np.pi * 440 * t),
                chord=0.2 * sum(np.sin(2 * np.pi * f * t) for f in (220.0, 277.18, 329.63, 440.0)),
                glide=0.5 * np.sin(2 * np.pi * (300 * t + 100 * t * t)))      # 300 -> 700 Hz in 2 s


def unit_diff(a, b):
    """|a - b| of two phase arrays, mod 2^32"""
    d = (np.asarray(a, np.int64) - np.asarray(b, np.int64)) % (1 << 32)
    return int(np.minimum(d, (1 << 32) - d).max())


def sine_peak_hz(y, sr):
    n = y.shape[0]
    spec = np.abs(np.fft.rfft(np.asarray(y, np.float64) * np.hanning(n), 8 * n))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1:k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * sr / (8 * n)
