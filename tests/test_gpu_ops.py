"""The normalisation, scan, noise and index kernels of csrc/ops.hip, each on its own (rvcx_op_*), against the plain float64 /
exact references of tests/ops_reference.py -- at the smallest shapes that reach every code path: the 4 x 512 unrolled sums
and their 512-stride tails, both statistics kernels of the fused first HuBERT layer, 64-lane scan segments of every
raggedness, the n % 4 tail of the noise stream, pads wider than the signal, clipped decoder windows.

Bars: integer / copy kernels exact; fp32 arithmetic within fp32 rounding (relative RMS < 2e-6, the bar of the conv and GEMM
tests) and finite; the entry points NaN-fill their outputs first, so an element no thread wrote fails the finite check."""
import functools

import numpy as np
import pytest

from conftest import rms

import ops_reference as R

pytestmark = pytest.mark.gpu

FP32_BAR = 2e-6
EPS = float(np.float32(1e-5))


def _rel(got, ref):
    return rms(np.asarray(got, np.float64) - ref) / max(rms(ref), 1e-300)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- GroupNorm + GELU
GN_B, GN_C = 3, 16


@functools.lru_cache(maxsize=None)
def _gn_case(T, ragged):
    g = np.random.default_rng(1000 + T)
    x = g.standard_normal((GN_B, GN_C, T)).astype(np.float32) * g.uniform(0.5, 2.0, (GN_B, GN_C, 1)).astype(np.float32)
    x += g.uniform(-0.5, 0.5, (GN_B, GN_C, 1)).astype(np.float32)
    gamma = (1 + 0.2 * g.standard_normal(GN_C)).astype(np.float32)
    beta = (0.2 * g.standard_normal(GN_C)).astype(np.float32)
    lens = [T, min(T, T // 2 + 3), 1] if ragged else None
    return x, gamma, beta, lens, R.groupnorm_gelu(x, gamma, beta, EPS, lens)


def _check_split(ys, y):
    """the split image holds hi = fp16(v) and lo = fp16((v - hi) * 256): 22 significant bits while lo is a normal fp16 number,
    and never worse than half a quantum of a subnormal lo, 2^-25 / 256 = 2^-33, absolute.  Asked for: 2^-19 relative."""
    assert np.isfinite(ys).all()
    d = np.abs(ys.astype(np.float64) - y.astype(np.float64))
    assert (d <= 2.0 ** -19 * np.abs(y.astype(np.float64)) + 2.0 ** -33).all(), d.max()


def _check_stats(st, mean, rstd):
    std = 1.0 / rstd
    assert np.isfinite(st).all()
    assert (np.abs(st[..., 0] - mean) <= FP32_BAR * np.maximum(np.abs(mean), std)).all()
    assert (np.abs(st[..., 1] / rstd - 1) <= FP32_BAR).all()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("T", [1, 511, 513, 2047, 2049, 4100])
def test_groupnorm_gelu(ctx, T, ragged):
    """T: tail only (1, 511), one thread with two tail frames (513), just short of / just past one unrolled trip (2047, 2049),
    two trips (4100); lens [T, T/2 + 3, 1]"""
    x, gamma, beta, lens, (ref, mean, rstd) = _gn_case(T, ragged)
    y, st, ys = ctx.groupnorm_gelu(x, gamma, beta, EPS, lens)
    e = _rel(y, ref)
    print(f"groupnorm_gelu T {T} lens {lens}: rel err {e:.2e}")
    assert np.isfinite(y).all() and e < FP32_BAR
    _check_stats(st, mean, rstd)
    _check_split(ys, y)
    if lens is None:
        return
    for b, L in enumerate(lens):
        assert not y[b, :, L:].any() and not ys[b, :, L:].any()
        y1, st1, ys1 = ctx.groupnorm_gelu(x[b:b + 1, :, :L], gamma, beta, EPS)          # the item alone, at its own length
        assert np.array_equal(_bits(y[b, :, :L]), _bits(y1[0]))
        assert np.array_equal(_bits(st[b]), _bits(st1[0]))
        assert np.array_equal(_bits(ys[b, :, :L]), _bits(ys1[0]))


def test_groupnorm_gelu_constant_rows(ctx):
    """var = 0: finite, rstd = 1 / sqrt(eps), y = gelu(beta)"""
    g = np.random.default_rng(7)
    x = np.repeat(g.uniform(-4, 4, (2, 16, 1)).astype(np.float32), 513, 2)
    gamma, beta = g.standard_normal(16).astype(np.float32), g.standard_normal(16).astype(np.float32)
    ref, mean, rstd = R.groupnorm_gelu(x, gamma, beta, EPS)
    y, st, ys = ctx.groupnorm_gelu(x, gamma, beta, EPS)
    assert np.isfinite(y).all() and np.isfinite(st).all()
    assert np.array_equal(st[..., 0], x[..., 0])
    assert (np.abs(st[..., 1] * np.sqrt(EPS) - 1) < FP32_BAR).all()
    assert _rel(y, ref) < FP32_BAR
    _check_split(ys, y)


# torch-CPU float32 group_norm + gelu against float64 on the input of the test below: relative RMS 5.65e-07 (measured on the
# CPU; seeds 89 / 90 give 3.8e-07 / 4.9e-07, the same input without the offset 8.9e-08).  The kernel rounds the mean to
# float32 once, as torch does, and differs in rounding direction and summation order only: 4 x.
GN_OFFSET_BAR = 4 * 5.65e-7


def test_groupnorm_gelu_offset_rows(ctx):
    """x = 8 + N(0, 1): the float32 mean (one ulp of 8 is 9.5e-7 of the unit deviation) limits any float32 implementation;
    torch-CPU float32 sits at 5.65e-07 relative RMS of float64 on this input, the bar is GN_OFFSET_BAR = 4 x that"""
    g = np.random.default_rng(88)
    x = (8 + g.standard_normal((3, 16, 2049))).astype(np.float32)
    gamma, beta = (1 + 0.1 * g.standard_normal(16)).astype(np.float32), (0.1 * g.standard_normal(16)).astype(np.float32)
    ref, mean, rstd = R.groupnorm_gelu(x, gamma, beta, EPS)
    y, st, ys = ctx.groupnorm_gelu(x, gamma, beta, EPS)
    e = _rel(y, ref)
    print(f"groupnorm_gelu 8 + N(0,1): rel err {e:.2e} (bar {GN_OFFSET_BAR:.2e})")
    assert np.isfinite(y).all() and e < GN_OFFSET_BAR
    _check_stats(st, mean, rstd)
    _check_split(ys, y)


# ---------------------------------------------------------------------------------------------------- fused first HuBERT layer
@pytest.mark.parametrize("B,C,T0,lens", [
    (1, 32, 100, None),                                        # the 4-channel statistics kernel, tail only
    (1, 32, 2049, None),                                       # ... one unrolled trip + tail
    (1, 32, 2049, [2040]),
    (8, 512, 600, [600, 599, 513, 512, 511, 300, 10, 1]),      # B * C / 16 = 256 blocks: the 16-channel kernel
])
def test_hubert_conv0_fused_equals_three_passes(ctx, B, C, T0, lens):
    K, stride = 10, 5
    n = stride * (T0 - 1) + K
    g = np.random.default_rng(B * 100000 + C * 100 + T0)
    wav = g.standard_normal((B, n)).astype(np.float32) * g.uniform(0.05, 1.0, (B, 1)).astype(np.float32)
    w = (g.standard_normal((C, 1, K)) / np.sqrt(K)).astype(np.float32)
    gamma, beta = (1 + 0.2 * g.standard_normal(C)).astype(np.float32), (0.2 * g.standard_normal(C)).astype(np.float32)
    st1, y1, raw1 = ctx.hubert_conv0(wav, w, gamma, beta, stride, EPS, lens, fused=True)
    st0, y0, raw0 = ctx.hubert_conv0(wav, w, gamma, beta, stride, EPS, lens, fused=False)
    assert np.isfinite(st1).all() and np.isfinite(y1).all()
    assert np.array_equal(_bits(st1), _bits(st0))
    assert np.array_equal(raw1, raw0)
    ref, mean, rstd = R.hubert_conv0(wav, w, gamma, beta, stride, EPS, lens)
    e = _rel(y1, ref)
    print(f"hubert_conv0 B {B} C {C} T0 {T0}: rel err {e:.2e}")
    assert e < FP32_BAR
    # statistics of fp32 conv outputs: held to float64 where the item is long enough for its deviation to dwarf the conv's own
    # rounding (a one-frame item has deviation 0 and a mean that is a single fp32 dot product)
    long_items = [b for b in range(B) if (lens is None or lens[b] >= 100)]
    _check_stats(st1[long_items], mean[long_items], rstd[long_items])
    if lens is not None:
        for b, L in enumerate(lens):
            assert not y1[b, :, L:].any()


# ---------------------------------------------------------------------------------------------------- NSF sine source
SINE_SR, SINE_B = 48000, 3
SINE_WB = (0.9, 0.05)


@functools.lru_cache(maxsize=None)
def _sine_case(T, upp):
    g = np.random.default_rng(31 * T + upp)
    t = np.arange(T)
    f0 = np.zeros((SINE_B, T), np.float32)
    f0[0] = 575 + 500 * np.sin(2 * np.pi * t / 97 + 1.0) + 20 * np.sin(2 * np.pi * t / 7)          # voiced throughout, 55 .. 1095 Hz
    for b in (1, 2):          # voiced runs (vibrato around a random pitch) between runs of zeros
        pos, voiced = 0, b == 1
        while pos < T:
            run = int(g.integers(1, 40))
            if voiced:
                c = g.uniform(80, 1000)
                f0[b, pos:pos + run] = np.clip(c * (1 + 0.05 * np.sin(2 * np.pi * t[pos:pos + run] / 11)), 50, 1100)
            pos, voiced = pos + run, not voiced
    noise = g.standard_normal((SINE_B, T * upp)).astype(np.float32)
    lens = [T, max(1, 2 * T // 3), max(1, T // 2)]
    return f0, noise, lens, R.sine_source(f0, noise, SINE_WB, upp, SINE_SR, lens)


@pytest.mark.parametrize("T,upp", [(1, 10), (63, 10), (64, 10), (65, 10), (130, 480), (4099, 480)])
def test_sine_source(ctx, T, upp):
    """T below, at and above the 64 lanes of the prefix scan, segments of 1, 2, 3 and 65 frames with an empty or short last
    lane; |tanh'| <= 1, so float32 arithmetic on |v| <= 0.2 (0.1 sine + 0.033 x noise) stays below 2e-6 absolute"""
    f0, noise, lens, ref = _sine_case(T, upp)
    har = ctx.sine_source(f0, noise, SINE_WB, upp, SINE_SR, lens)
    e = np.abs(har - ref).max()
    print(f"sine_source T {T} upp {upp}: max abs err {e:.2e}")
    assert np.isfinite(har).all() and e < 2e-6
    for b, L in enumerate(lens):
        assert not har[b, L * upp:].any()


def test_sine_source_phase_drift(ctx):
    """4099 frames x 480 samples: the kernel's own phase, recovered from a run without noise and with the identity Linear
    (har = tanh(0.1 sin(2 pi ph))) on samples away from the sine's extrema, stays within 1e-4 cycles of the reference over the
    last 100 frames of every item (a float32 running sum is off by more than 1e-3 cycles there)"""
    T, upp = 4099, 480
    f0, _, lens, _ = _sine_case(T, upp)
    har = ctx.sine_source(f0, np.zeros((SINE_B, T * upp), np.float32), (1.0, 0.0), upp, SINE_SR, lens)
    ph = R.sine_phase(R.sine_rad(f0, SINE_SR), upp)
    checked = 0
    for b, L in enumerate(lens):
        sl = slice(L - 100, L)
        s = np.arctanh(har[b].reshape(T, upp)[sl].astype(np.float64)) / float(np.float32(0.1))
        ok = (np.abs(s) < 0.9) & (f0[b, sl, None] > 0)
        a = np.arcsin(np.clip(s, -1, 1)) / (2 * np.pi)
        want = ph[b, sl]
        d1 = np.abs((a - want + 0.5) % 1 - 0.5)                  # rising branch
        d2 = np.abs((0.5 - a - want + 0.5) % 1 - 0.5)            # falling branch (0.14 cycles from the other where |s| < 0.9)
        err = np.minimum(d1, d2)[ok]
        checked += err.size
        print(f"sine phase item {b}: {err.size} samples, max {err.max() if err.size else 0:.2e} cycles")
        assert err.size == 0 or err.max() < 1e-4
        if b == 0:
            assert err.size > 100 * upp // 2
    assert checked > 0


# ---------------------------------------------------------------------------------------------------- Philox noise
RANDN_CASES = [(1, 0, 0), (2, 1, 0), (3, 1, 0), (5, 7, 0), (1025, (1 << 40) + 3, 0), (70001, 12345, (1 << 33) + 5),
               (18, 9, (1 << 32) - 2)]          # the last one: the counter carries into its high word after two blocks


@pytest.mark.parametrize("n,seed,offset", RANDN_CASES)
def test_randn_is_philox_box_muller(ctx, n, seed, offset):
    """|value| <= sqrt(-2 ln 2^-33) = 6.8 times the error of float32 log / sqrt / cos / sin (a few 1e-7): 1e-5"""
    got = ctx.randn(n, seed, offset)
    ref = R.randn(n, seed, offset)
    e = np.abs(got - ref).max()
    print(f"randn n {n} seed {seed} offset {offset}: max abs err {e:.2e}")
    assert got.shape == (n,) and np.isfinite(got).all() and e < 1e-5
    if n == 70001:
        assert abs(got.mean()) < 5 / np.sqrt(n) and abs(got.astype(np.float64).var() - 1) < 5 * np.sqrt(2 / n)


def test_randn_stream_continues(ctx):
    n, seed, off = 70001, 12345, (1 << 33) + 5
    a = ctx.randn(n, seed, off)
    for k in (1, 256, 4097):
        assert np.array_equal(_bits(a[4 * k:]), _bits(ctx.randn(n - 4 * k, seed, off + k))), k
    assert np.array_equal(_bits(a[:1023]), _bits(ctx.randn(1023, seed, off)))          # a shorter draw is a prefix
    assert not np.array_equal(a[:1025], ctx.randn(1025, seed + (1 << 32), off))         # the seed's high word counts
    assert not np.array_equal(a[:1025], ctx.randn(1025, seed, off - (1 << 33)))         # the offset's high word counts
    assert not np.array_equal(ctx.randn(1025, 3, 0), ctx.randn(1025, (1 << 40) + 3, 0))


# ---------------------------------------------------------------------------------------------------- index arithmetic
@pytest.mark.parametrize("n,p", [(1, 4), (2, 5), (5, 4), (5, 5), (5, 13), (400, 1000), (4000, 16)])
def test_reflect_pad(ctx, n, p):
    g = np.random.default_rng(n * 31 + p)
    x = g.standard_normal((3, n)).astype(np.float32)
    for ns in (None, [n, max(1, n // 2), 1]):
        got = ctx.reflect_pad(x, p, ns)
        assert np.array_equal(_bits(got), _bits(R.reflect_pad(x, p, ns))), ns
        if ns is not None:
            for b, nb in enumerate(ns):
                assert not got[b, nb + 2 * p:].any()


@pytest.mark.parametrize("F,Tp,fs", [(33, 64, [33, 20, 17]), (64, 64, [64, 33, 32]), (100, 128, [100, 65, 50])])
def test_mel_post(ctx, F, Tp, fs):
    """fs: item lengths whose pad to the next multiple of 32 rows is a single reflection (17 -> 32 is the shortest)"""
    nmel, B = 128, 3
    g = np.random.default_rng(F)
    mel = np.exp(3 * g.standard_normal((B, nmel, F))).astype(np.float32)
    mel[g.uniform(size=mel.shape) < 0.1] *= 1e-7          # below the 1e-5 floor
    mel[g.uniform(size=mel.shape) < 0.05] = 0
    bn = (0.37, -1.2)
    tps = [32 * ((f + 31) // 32) for f in fs]
    for a, b in ((None, None), (fs, tps)):
        got = ctx.mel_post(mel, Tp, bn, a, b)
        ref = R.mel_post(mel, Tp, bn, a, b)
        e = _rel(got, ref)
        print(f"mel_post F {F} Tp {Tp} ragged {a is not None}: rel err {e:.2e}")
        assert np.isfinite(got).all() and e < FP32_BAR
        assert not got[:, :, 0].any() and not got[:, :, -1].any()
        if b is not None:
            for i, tb in enumerate(b):
                assert not got[i, tb:].any()


def _decode_frames(T, ld):
    """B = 2 items of T frames: random frames, and in front of them as many of the hand-built ones as fit (all of them at
    T = 1001; a window of the list that moves with T otherwise).  Columns 360 .. ld hold large values nobody may read."""
    B = 2
    g = np.random.default_rng(T * 1000 + ld)
    sal = (g.uniform(0, 1, (B * T, ld)) ** 6).astype(np.float32)
    hand = []

    def frame(peaks, noise=0.02):
        f = (g.uniform(0, noise, 360)).astype(np.float32)
        for k, v in peaks:
            f[k] = v
        hand.append(f)

    for k in (0, 1, 3, 4, 180, 355, 356, 359):
        frame([(k, 0.9)])
        frame([(k, 0.9), (max(k - 1, 0), 0.9 if k == 0 else 0.6), (min(k + 2, 359), 0.9 if k == 359 else 0.5)])
    frame([(100, 0.5), (164, 0.5)])          # equal maxima in one lane's bins (100 and 164 are 64 apart): the lower bin wins
    frame([(100, 0.5), (137, 0.5)])          # ... in two lanes
    frame([(200, 0.7), (201, 0.7)])          # ... next to each other
    frame([(5, 0.25), (300, 0.25), (359, 0.25)], noise=0.0)
    frame([(180, np.float32(0.03))], noise=0.01)          # the maximum equals the threshold: unvoiced
    frame([(180, np.nextafter(np.float32(0.03), np.float32(1)))], noise=0.01)
    frame([(20, 0.9)], noise=0.0)            # 40 Hz: below f0_min
    frame([(250, 0.9)], noise=0.0)           # 570 Hz
    frame([(330, 0.9)], noise=0.0)           # 1436 Hz: above f0_max
    frame([], noise=0.0)                     # all zero
    m = min(len(hand), B * T)
    for i in range(m):
        sal[i, :360] = hand[(2 * T + i) % len(hand)]
    sal[:, 360:] = 9.0
    return sal.reshape(B, T, ld)


@pytest.mark.parametrize("ld", [360, 384])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 1001])
def test_decode_f0(ctx, T, ld):
    """four frames per block: T = 1 .. 5 leave waves of the last block without a frame; exact (the kernel promises numpy's bits)"""
    sal = _decode_frames(T, ld)
    for f0_min, f0_max in ((50.0, 1100.0), (20.0, 3000.0)):          # the second pair lets the clipped windows at bins 0 and 359 through
        got = ctx.decode_f0(sal, 0.03, f0_min, f0_max)
        ref = R.decode_f0(sal[:, :, :360].reshape(-1, 360), 0.03, f0_min, f0_max).reshape(2, T)
        bad = np.flatnonzero(_bits(got).ravel() != _bits(ref).ravel())
        assert bad.size == 0, (bad[:8], got.ravel()[bad[:8]], ref.ravel()[bad[:8]])
        if T == 1001 and f0_max == 1100.0:
            assert (ref > 0).sum() > 500 and (ref == 0).sum() > 100          # both sides of every gate occur


@pytest.mark.parametrize("Wp", [6, 130])
def test_avgpool2(ctx, Wp):
    planes, H = 3, 7          # odd H: the last row is dropped
    W, H2, W2 = Wp - 2, H // 2, (Wp - 2) // 2
    g = np.random.default_rng(Wp)
    x_ps, y_ps = H * Wp + 5, H2 * (W2 + 2) + 3
    dense = g.standard_normal((planes, H, W)).astype(np.float32)
    x = g.standard_normal((planes, x_ps)).astype(np.float32)          # the gap between planes holds values nobody may read
    rows = x[:, :H * Wp].reshape(planes, H, Wp)
    rows[:, :, 1:-1] = dense
    rows[:, :, 0] = rows[:, :, -1] = 0
    got = ctx.avgpool2(x, H, Wp, y_ps)
    out = got[:, :H2 * (W2 + 2)].reshape(planes, H2, W2 + 2)
    assert np.isnan(got[:, H2 * (W2 + 2):]).all()                     # and the gap behind a pooled plane is not written
    assert np.isfinite(out).all() and not out[:, :, 0].any() and not out[:, :, -1].any()
    assert _rel(out[:, :, 1:-1], R.avgpool2(dense)) < FP32_BAR


@pytest.mark.parametrize("Wp", [6, 130])
def test_gru_input(ctx, Wp):
    g = np.random.default_rng(Wp + 1)
    x = g.standard_normal((2, 3, 5, Wp)).astype(np.float32)           # pad columns non-zero: they must not travel
    assert np.array_equal(_bits(ctx.gru_input(x)), _bits(R.gru_input(x)))


@pytest.mark.parametrize("use_protect", [0, 1])
@pytest.mark.parametrize("Th,p_len,ld_in,ld_out", [(6, 11, 9, 14), (6, 7, 6, 7), (300, 599, 301, 640)])
def test_upsample_protect(ctx, Th, p_len, ld_in, ld_out, use_protect):
    Cc = 5
    g = np.random.default_rng(Th + p_len)
    feats = g.standard_normal((Cc, ld_in)).astype(np.float32)
    feats0 = g.standard_normal((Cc, ld_in)).astype(np.float32)
    pitchf = g.choice(np.array([0.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), 1.0, np.nextafter(np.float32(1), np.float32(2)),
                                100.0, 440.0], np.float32), p_len).astype(np.float32)
    pitchf[:5] = [0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 220.0, 0.5]
    got = ctx.upsample_protect(feats, feats0, pitchf, Th, p_len, 0.33, use_protect, ld_out)
    ref = R.upsample_protect(feats[:, :Th], feats0[:, :Th], pitchf, p_len, 0.33, use_protect)
    assert np.isnan(got[:, p_len:]).all()                             # columns behind p_len belong to somebody else
    out = got[:, :p_len]
    assert np.isfinite(out).all()
    if use_protect:
        assert _rel(out, ref) < FP32_BAR
        keep = pitchf >= 1
        assert np.array_equal(out[:, keep], ref[:, keep].astype(np.float32))          # factor 1: the feature itself
    else:
        assert np.array_equal(out, ref.astype(np.float32))
