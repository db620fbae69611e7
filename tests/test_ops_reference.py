"""CPU: the plain references of tests/ops_reference.py against published vectors, the oracle's own formulation and cases
worked by hand.  tests/test_gpu_ops.py holds the HIP kernels to these references."""
import numpy as np
import torch

import ops_reference as R


# counter, key -> output: the known-answer vectors of Random123 (kat_vectors, philox4x32 with 10 rounds)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        assert R.philox4x32_10(ctr, key) == want, [hex(v) for v in R.philox4x32_10(ctr, key)]


def test_philox_vectorised_equals_scalar():
    """the numpy uint64 form (what randn uses) against the Python-int form, high seed and offset words included"""
    for seed, off in [(0, 0), (7, 3), ((1 << 40) + 3, (1 << 33) + 5), ((1 << 64) - 1, (1 << 64) - 2)]:
        w = R.randn_words(13, seed, off)
        assert w.shape == (4, 4) and w.dtype == np.uint32
        for q in range(4):
            c = (off + q) & ((1 << 64) - 1)
            want = R.philox4x32_10((c & 0xffffffff, c >> 32, R.RANDN_STREAM, 0), (seed & 0xffffffff, seed >> 32))
            assert tuple(int(v) for v in w[q]) == want


def test_randn_reference_properties():
    a = R.randn(70001, 12345, (1 << 33) + 5)
    assert a.shape == (70001,) and a.dtype == np.float64 and np.isfinite(a).all()
    n = a.size
    assert abs(a.mean()) < 5 / np.sqrt(n) and abs(a.var() - 1) < 5 * np.sqrt(2 / n)
    # four values per counter step: a stream started k steps later continues the same sequence
    assert np.array_equal(a[4 * 256:], R.randn(n - 4 * 256, 12345, (1 << 33) + 5 + 256))
    assert np.array_equal(R.randn(5, 7)[:3], R.randn(3, 7))


def test_sine_reference_means_the_models_two_cumsums():
    """oracle.synth.sine_source (the reference model's interpolate / wrap / cumsum formulation) in float64 on the float32-rounded
    rad, against the closed form of ops_reference: the same signal to 1e-9"""
    from oracle import synth as OS
    T, upp, sr = 40, 10, 48000.0
    rng = np.random.default_rng(5)
    f0 = np.zeros((2, T), np.float32)
    f0[0] = 220 * 2 ** (rng.uniform(-1, 2, T))
    f0[1, 5:17] = rng.uniform(50, 1100, 12)
    f0[1, 25:] = rng.uniform(50, 1100, 15)
    noise = rng.standard_normal((2, T * upp))
    rad = R.sine_rad(f0, sr)
    assert rad.dtype == np.float32 and (rad[f0 > 0] > 0).all() and (rad[f0 == 0] == 0).all()
    # sr = 1: the oracle's (f0 / sr) % 1 is then rad itself, exactly, and its voiced flag (f0 > 0) is the track's
    want = OS.sine_source(torch.from_numpy(rad.astype(np.float64)), upp, 1.0, torch.from_numpy(noise)[:, :, None])[:, :, 0].numpy()
    got = R.sine_excitation(f0, noise, upp, sr)
    assert want.dtype == np.float64
    assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max()


def test_sine_reference_phase_is_exact():
    """the wrapped float64 prefix against exact rational arithmetic (float32 values are dyadic rationals)"""
    from fractions import Fraction
    rng = np.random.default_rng(6)
    f0 = rng.uniform(50, 1100, (1, 300)).astype(np.float32)
    rad = R.sine_rad(f0, 48000)
    ph = R.sine_phase(rad, 480)
    acc = Fraction(0)
    for t in range(300):
        r = Fraction(float(rad[0, t]))
        for jj in (0, 479):
            e = acc + (jj + 1) * r
            e -= e.numerator // e.denominator
            d = abs(float(e) - ph[0, t, jj])
            assert min(d, 1 - d) < 1e-12
        acc += 480 * r


def test_reflect_pad_hand_cases():
    assert np.array_equal(R.reflect_pad(np.array([[7.0]]), 4), np.full((1, 9), 7.0))          # n = 1: a constant
    x = np.array([[0.0, 1.0, 2.0]])
    # n = 3, p = 7: the triangle wave of period 4 through 0 1 2 1 | 0 1 2 1 ...
    assert np.array_equal(R.reflect_pad(x, 7)[0], [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1])
    # ragged: item 1 holds two samples, its padded signal is 2 + 2 p long and zeros follow
    y = R.reflect_pad(np.array([[0.0, 1.0, 2.0], [5.0, 6.0, 9.0]]), 2, ns=[3, 2])
    assert np.array_equal(y, [[2, 1, 0, 1, 2, 1, 0], [5, 6, 5, 6, 5, 6, 0]])


def _cents_to_f0(c):
    return np.float32(10 * 2 ** (c / 1200))


def test_decode_f0_hand_cases():
    base = R.CENTS_BASE
    sal = np.zeros((6, 360), np.float32)
    sal[0, 0] = 0.5                      # peak at bin 0: the window is clipped, the average is bin 0's cents
    sal[1, 100], sal[1, 200] = 0.5, 0.5  # two equal maxima: the lower bin wins
    sal[2, 180] = np.float32(0.03)       # maximum equal to the threshold: unvoiced
    sal[3, 359] = 0.9                    # bin 359 = 9177 cents = 2006 Hz: above f0_max
    sal[4, 59:62] = [0.25, 0.5, 0.25]    # symmetric neighbours: the centre's cents (20 * 60 + base)
    # row 5: all zero
    f0 = R.decode_f0(sal, f0_min=20.0)
    assert f0.dtype == np.float32
    assert f0[0] == _cents_to_f0(base)
    assert f0[1] == _cents_to_f0(20 * 100 + base)
    assert f0[2] == 0 and f0[3] == 0 and f0[5] == 0
    assert abs(float(f0[4]) - float(_cents_to_f0(20 * 60 + base))) < 1e-4
    assert R.decode_f0(sal, f0_max=3000.0)[3] == _cents_to_f0(20 * 359 + base)
    assert 31 < f0[0] < 32 and R.decode_f0(sal)[0] == 0          # bin 0 is 31.7 Hz: below the default f0_min = 50


def test_decode_f0_equals_the_oracle():
    from oracle import rmvpe as OR
    rng = np.random.default_rng(7)
    sal = rng.uniform(0, 1, (200, 360)).astype(np.float32) ** 4
    sal[::7] *= 0.01
    want = OR.decode_f0(sal.copy()).astype(np.float32)
    assert np.array_equal(R.decode_f0(sal), want)
    assert (want > 0).sum() > 50 and (want == 0).sum() > 10


def test_small_index_references():
    x = np.arange(2 * 5 * 6, dtype=np.float64).reshape(2, 5, 6)
    want = torch.nn.functional.avg_pool2d(torch.from_numpy(x), 2).numpy()
    assert np.array_equal(R.avgpool2(x), want) and want.shape == (2, 2, 3)
    g = np.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5)
    y = R.gru_input(g)
    assert y.shape == (2, 9, 4) and y[1, 2 * 3 + 1, 3] == g[1, 2, 3, 2]
    f, f0 = np.array([[1.0, 2.0, 3.0]]), np.array([[10.0, 20.0, 30.0]])
    out = R.upsample_protect(f, f0, np.array([0.0, 100.0, 100.0, 0.5, 1.0], np.float32), 5, 0.5, True)
    assert np.array_equal(out, [[5.5, 1.0, 2.0, 11.0, 3.0]])
    assert np.array_equal(R.upsample_protect(f, None, None, 5, 0.5, False), [[1, 1, 2, 2, 3]])
