"""Plain references of the operations csrc/ops.hip implements, for tests/test_gpu_ops.py: numpy / torch on the CPU, float64
wherever the arithmetic is floating point, exact integers elsewhere.  Written from the definitions of the operations (and from
what the reference model computes), not from the kernels; tests/test_ops_reference.py checks them on their own."""
import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------------- Philox4x32-10
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
RANDN_STREAM = 0x52564358          # third counter word of the library's noise stream
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """One block of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11) on Python ints:
    counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = (int(v) & _M32 for v in counter)
    k0, k1 = (int(v) & _M32 for v in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def _philox_blocks(ctr, seed):
    """the same on numpy uint64 arrays: 64-bit counters ctr (nq,) with the stream constant, key = the two halves of seed"""
    m = np.uint64(_M32)
    sh = np.uint64(32)
    c0, c1 = ctr & m, ctr >> sh
    c2 = np.full_like(ctr, RANDN_STREAM)
    c3 = np.zeros_like(ctr)
    k0, k1 = np.uint64(seed & _M32), np.uint64((seed >> 32) & _M32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m, (k1 + np.uint64(PHILOX_W1)) & m
    return c0, c1, c2, c3


def randn_words(n, seed, offset):
    """(ceil(n / 4), 4) uint32 words of the noise stream: block q has the counter (offset + q, RANDN_STREAM, 0)"""
    nq = (int(n) + 3) // 4
    ctr = (np.arange(nq, dtype=np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF))      # wraps mod 2^64
    return np.stack(_philox_blocks(ctr, int(seed)), 1).astype(np.uint32)


def randn(n, seed, offset=0):
    """n values: Box-Muller on the word pairs (c0, c1) and (c2, c3) of each block.  The uniforms u = (float32(c) + 0.5) 2^-32
    and the angle 6.2831853f * u are formed in float32 (they are part of the definition: a float32 angle is a different
    angle); log, sqrt, cos and sin are float64."""
    w = randn_words(n, seed, offset)
    u = (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    ang = (np.float32(6.2831853) * u[:, [1, 3]]).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[:, [0, 2]].astype(np.float64)))
    out = np.stack([r[:, 0] * np.cos(ang[:, 0]), r[:, 0] * np.sin(ang[:, 0]),
                    r[:, 1] * np.cos(ang[:, 1]), r[:, 1] * np.sin(ang[:, 1])], 1)
    return out.reshape(-1)[:int(n)]


# ---------------------------------------------------------------------------------------------------- NSF sine source
def sine_rad(f0, sr):
    """rad = (f0 / sr) % 1 in float32, as the reference model (a float32 module) computes it"""
    f0 = np.asarray(f0, np.float32)
    return np.fmod(f0 / np.float32(sr), np.float32(1.0)).astype(np.float32)


def sine_phase(rad, upp):
    """phase in cycles of sample jj of frame t: frac(upp * sum_{t' < t} rad[t'] + (jj + 1) rad[t]) -- what
    sin(2 pi cumsum(rad upsampled)) of the model sees, whole cycles dropped.  rad (B, T) -> (B, T, upp) float64.  The prefix is
    kept wrapped (only integers are removed), so float64 holds it to 1e-16 per frame."""
    rad = np.asarray(rad, np.float64)
    B, T = rad.shape
    pre = np.zeros((B, T))
    run = np.zeros(B)
    for t in range(T):
        pre[:, t] = run
        run = run + rad[:, t] * upp
        run -= np.floor(run)
    ph = pre[:, :, None] + np.arange(1, upp + 1)[None, None, :] * rad[:, :, None]
    return ph - np.floor(ph)


def sine_excitation(f0, noise, upp, sr, rad=None):
    """sine * uv + noise_amp * noise of SineGenerator (harmonic_num = 0): f0 (B, T), noise (B, T upp) -> (B, T upp) float64"""
    f0 = np.asarray(f0, np.float32)
    B, T = f0.shape
    rad = sine_rad(f0, sr) if rad is None else rad
    ph = sine_phase(rad, upp).reshape(B, T * upp)
    uv = np.repeat((f0 > 0).astype(np.float64), upp, 1)
    namp = uv * 0.003 + (1.0 - uv) * 0.1 / 3.0
    return 0.1 * np.sin(2.0 * np.pi * ph) * uv + namp * np.asarray(noise, np.float64)


def sine_source(f0, noise, lin_wb, upp, sr, lens=None):
    """har = tanh(w * excitation + b), zero in the frames behind lens[b]"""
    v = sine_excitation(f0, noise, upp, sr)
    har = np.tanh(float(np.float32(lin_wb[0])) * v + float(np.float32(lin_wb[1])))
    if lens is not None:
        for b, L in enumerate(lens):
            har[b, int(L) * upp:] = 0.0
    return har


# ---------------------------------------------------------------------------------------------------- GroupNorm + GELU
def groupnorm_gelu(x, gamma, beta, eps=1e-5, lens=None, dtype=torch.float64):
    """GroupNorm(C, C) + GELU (erf) of x (B, C, T), every item at its own length -> (y (B, C, T) with zeros behind lens[b],
    mean (B, C), rstd (B, C)); dtype float32 gives torch's own float32 answer (the yardstick of an ill-conditioned input)"""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    g, bt = torch.as_tensor(np.asarray(gamma)).to(dtype), torch.as_tensor(np.asarray(beta)).to(dtype)
    B, C, T = x.shape
    y = torch.zeros_like(x)
    mean, rstd = torch.zeros(B, C, dtype=dtype), torch.zeros(B, C, dtype=dtype)
    for b in range(B):
        L = T if lens is None else int(lens[b])
        xb = x[b:b + 1, :, :L]
        mean[b] = xb.mean(2)[0]
        rstd[b] = 1.0 / torch.sqrt(xb.var(2, unbiased=False)[0] + eps)
        if L > 1:
            y[b, :, :L] = F.gelu(F.group_norm(xb, C, g, bt, eps))[0]
        else:          # torch refuses one value per channel: the definition itself (the deviation is zero)
            y[b, :, :L] = F.gelu((xb[0] - mean[b][:, None]) * rstd[b][:, None] * g[:, None] + bt[:, None])
    return y.numpy(), mean.numpy(), rstd.numpy()


def hubert_conv0(wav, w, gamma, beta, stride, eps=1e-5, lens=None):
    """conv1d(wav (B, n), w (C, 1, K), stride) in float64, then the GroupNorm + GELU above"""
    x = F.conv1d(torch.as_tensor(np.asarray(wav)).double()[:, None], torch.as_tensor(np.asarray(w)).double(), stride=stride)
    return groupnorm_gelu(x.numpy(), gamma, beta, eps, lens)


# ---------------------------------------------------------------------------------------------------- index arithmetic
def reflect_pad(x, p, ns=None):
    """np.pad(x[b, :ns[b]], p, "reflect") per item, zeros behind it: x (B, n) -> (B, n + 2 p)"""
    x = np.asarray(x)
    B, n = x.shape
    y = np.zeros((B, n + 2 * p), x.dtype)
    for b in range(B):
        nb = n if ns is None else int(ns[b])
        y[b, :nb + 2 * p] = np.pad(x[b, :nb], p, mode="reflect")
    return y


def mel_post(mel, Tp, bn, fs=None, tps=None):
    """log(max(mel, 1e-5)) * sc + sh on the frames reflected as F.pad(.., "reflect"): mel (B, nmel, F) -> (B, Tp, nmel + 2)
    float64, zero pad columns, zero rows behind tps[b]"""
    mel = np.asarray(mel, np.float32)
    B, nmel, Fr = mel.shape
    out = np.zeros((B, Tp, nmel + 2))
    sc, sh = float(np.float32(bn[0])), float(np.float32(bn[1]))
    for b in range(B):
        Fb = Fr if fs is None else int(fs[b])
        Tb = Tp if tps is None else int(tps[b])
        m = torch.as_tensor(mel[b:b + 1, :, :Fb]).double()
        m = F.pad(m, (0, Tb - Fb), mode="reflect") if Tb > Fb else m[:, :, :Tb]
        lg = torch.log(torch.clamp(m, min=float(np.float32(1e-5)))) * sc + sh
        out[b, :Tb, 1:-1] = lg[0].numpy().T
    return out


CENTS_BASE = 1997.3794084376191


def decode_f0(sal, thred=0.03, f0_min=50.0, f0_max=1100.0):
    """to_local_average_cents + the gates of the F0 model's decoder, restated: sal (N, 360) float32 -> f0 (N,) float32.
    Arithmetic of the original: float32 salience times float64 cents, numpy sums, first-maximum argmax."""
    sal = np.asarray(sal, np.float32)
    cm = np.pad(20 * np.arange(360) + CENTS_BASE, (4, 4))
    center = np.argmax(sal, axis=1)
    salp = np.pad(sal, ((0, 0), (4, 4)))
    idx = center[:, None] + np.arange(9)[None, :]
    win = np.ascontiguousarray(np.take_along_axis(salp, idx, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        cents = np.sum(win * cm[idx], 1) / np.sum(win, 1)
    cents[np.max(sal, axis=1) <= np.float32(thred)] = 0
    f0 = 10 * (2 ** (cents / 1200))
    f0[f0 == 10] = 0
    f0[(f0 < float(np.float32(f0_min))) | (f0 > float(np.float32(f0_max)))] = 0
    return f0.astype(np.float32)


def avgpool2(x):
    """avg_pool2d(kernel 2) of dense planes (P, H, W) -> (P, H // 2, W // 2) float64"""
    x = np.asarray(x, np.float64)
    P, H, W = x.shape
    v = x[:, :H // 2 * 2, :W // 2 * 2].reshape(P, H // 2, 2, W // 2, 2)
    return v.sum((2, 4)) * 0.25


def gru_input(x):
    """row-padded (B, C, T, Wp) -> (B, C (Wp - 2), T): channel k = c (Wp - 2) + f holds column f + 1"""
    x = np.asarray(x)
    B, C, T, Wp = x.shape
    return np.ascontiguousarray(x[:, :, :, 1:-1].transpose(0, 1, 3, 2)).reshape(B, C * (Wp - 2), T)


def upsample_protect(feats, feats0, pitchf, p_len, protect, use_protect):
    """F.interpolate(scale_factor=2) (nearest) of feats (C, Th) cropped to p_len; with use_protect the frames whose pitchf < 1
    become feats * protect + feats0 * (1 - protect) -> (C, p_len) float64"""
    f = np.repeat(np.asarray(feats, np.float64), 2, 1)[:, :p_len]
    if not use_protect:
        return f
    f0 = np.repeat(np.asarray(feats0, np.float64), 2, 1)[:, :p_len]
    ff = np.where(np.asarray(pitchf, np.float32)[:p_len] < 1, float(np.float32(protect)), 1.0)[None, :]
    return f * ff + f0 * (1.0 - ff)
