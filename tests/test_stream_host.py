"""CPU: the host side of live streams -- head_from_rate (the reference's float32 `rate` arithmetic), the float64 SOLA
restatement the GPU tests measure against, and the argument checks of VC.stream_open that need no device."""
import numpy as np
import pytest


def test_head_from_rate_restates_the_reference():
    """int(T * (1.0 - rate.item())) for a float32 rate tensor (synthesizers.py:177): the values the reference produced"""
    from polgen_rvc_amd._lib import head_from_rate
    assert head_from_rate(40, 0.3) == 27            # float32(0.3) > 0.3: 40 * 0.69999998... = 27.99..., not 28
    assert head_from_rate(40, 0.25) == 30
    assert head_from_rate(40, 0.5) == 20
    assert head_from_rate(24, 0.375) == 15
    assert head_from_rate(40, np.float32(0.3)) == 27 and head_from_rate(40, 1.0) == 0


def test_sola_reference_on_a_hand_built_case():
    from polgen_rvc_amd._lib import sola_reference
    # Lx = 2, Ls = 2, Lb = 3.  windows of y: d=0 [0,0], d=1 [0,1], d=2 [1,2]; carry b = [3,6] is parallel to the last one
    y = np.array([0, 0, 1, 2, 5, 6, 7], np.float64)
    b = np.array([3, 6], np.float64)
    out, carry, d, scores, mags = sola_reference(y, b, 3, 2, 2)
    assert d == 2
    np.testing.assert_allclose(scores, [0.0, 6.0 / np.sqrt(1 + 1e-8), 15.0 / np.sqrt(5 + 1e-8)], rtol=1e-12)
    np.testing.assert_allclose(mags, np.abs(scores), rtol=1e-12)
    # fin = sin^2(pi/2 * i / (Lx - 1)) = [0, 1]: the first sample is the carry's, the second y's
    np.testing.assert_allclose(out, [3.0, 2.0, 5.0], atol=1e-15)
    np.testing.assert_array_equal(carry, [6.0, 7.0])
    # a forced offset; Lx > Lb cross-fades the min(Lx, Lb) samples there are
    out0, carry0, d0, _, _ = sola_reference(y, b, 3, 2, 2, offset=0)
    assert d0 == 0
    np.testing.assert_allclose(out0, [3.0, 0.0, 1.0], atol=1e-15)
    np.testing.assert_array_equal(carry0, [2.0, 5.0])
    y2 = np.arange(1.0, 8.0)
    o2, c2, _, _, _ = sola_reference(y2, np.array([1.0, 1.0, 1.0, 1.0]), 2, 4, 1, offset=1)
    fin = np.sin(0.5 * np.pi * np.arange(4) / 3) ** 2
    np.testing.assert_allclose(o2, y2[1:3] * fin[:2] + (1 - fin[:2]), rtol=1e-15)
    np.testing.assert_array_equal(c2, y2[3:7])


def test_sola_reference_ties_take_the_first_index():
    from polgen_rvc_amd._lib import sola_reference
    z = np.zeros(9)
    for b in (np.zeros(3), np.array([1.0, -2.0, 0.5])):
        out, carry, d, scores, _ = sola_reference(z, b, 4, 3, 2)
        assert d == 0 and not scores.any() and np.isfinite(out).all() and not carry.any()
    # the same window twice: equal scores, the first wins
    y = np.array([1.0, 2.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    assert sola_reference(y, np.array([1.0, 2.0]), 3, 2, 2)[2] == 0


def test_stream_open_argument_checks_need_no_device():
    from polgen_rvc_amd.infer import infer as I, pipeline as P

    class Net:
        input_dim, ctx, model_id = 768, object(), 0

    class Hub:
        ctx = object()
    vc = P.VC(48000, I.Config())
    geo = dict(block_ms=100, context_ms=2500, crossfade_ms=50, search_ms=10)
    args = (Hub(), Net(), [0], [0.0])
    with pytest.raises(ValueError, match="not implemented"):
        vc.stream_open(*args, "harvest", "", 0.0, "v2", 0.33, **geo)
    with pytest.raises(ValueError, match="mangio-crepe"):
        vc.stream_open(*args, "mangio-crepe", "", 0.0, "v2", 0.33, **geo)
    with pytest.raises(ValueError, match="does not match"):
        vc.stream_open(*args, "rmvpe", "", 0.0, "v1", 0.33, **geo)
    with pytest.raises(ValueError, match="unknown voice model version"):
        vc.stream_open(*args, "rmvpe", "", 0.0, "v3", 0.33, **geo)
    for bad in (dict(block_ms=0), dict(block_ms=105), dict(crossfade_ms=0), dict(search_ms=-10), dict(context_ms=12.5)):
        with pytest.raises(ValueError, match="multiple of 10 ms"):
            vc.stream_open(*args, "rmvpe", "", 0.0, "v2", 0.33, **{**geo, **bad})
    with pytest.raises(ValueError, match="per stream"):
        vc.stream_open(Hub(), Net(), [0, 1], [0.0], "rmvpe", "", 0.0, "v2", 0.33, **geo)
    with pytest.raises(ValueError, match="different rvcx contexts"):
        vc.stream_open(*args, "rmvpe", "", 0.0, "v2", 0.33, **geo)
    assert P.VC._stream_frames(100, 2500, 50, 10) == (10, 250, 5, 1)
