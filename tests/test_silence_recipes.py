"""The silence fixtures (tests/golden/pipeline_{tag}.npz, tools/gen_golden.py SILENCE_RECIPES) hold their input as a
recipe: rebuild it, and check on scipy's own filter that the stored cut points are the reference's, that every cut window
passes the conditioning check gen_golden.py asserts, and that the library's host filter -- the one the cut search runs
on -- is scipy.signal.filtfilt bit for bit.  No GPU."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TAGS = ["tiny_silent", "tiny_silent_env", "tiny_silent_cut", "tiny_gap_cut", "tiny_gap_cut_index", "tiny_lead_trail",
        "gap_real_geo"]
GAP_TAGS = ["tiny_gap_cut", "tiny_gap_cut_index", "gap_real_geo"]


def _recipe(tag):
    from polgen_rvc_amd import synthetic as S
    d = np.load(os.path.join(GOLD, f"pipeline_{tag}.npz"))
    audio = S.make_gapped_clip(int(d["clip"]), float(d["seconds"]), [tuple(s) for s in d["zero_spans"]])
    return d, audio


@pytest.mark.parametrize("tag", TAGS)
def test_recipe_gives_the_stored_cuts(tag):
    from oracle import pipeline as OP
    d, audio = _recipe(tag)
    filt = OP.highpass(audio.astype(np.float64))
    geo = OP.Geometry(48000, *[int(v) for v in d["geo"]])
    cuts = [int(t) for t in OP.chunk_points(filt, geo)]
    assert cuts == d["cuts"].tolist()
    assert int(d["n_chunks"]) == len(cuts) + 1
    margins = OP.cut_margins(filt, geo)
    print(f"{tag}: cuts {cuts}, margins {margins}")
    # all exact zeros (ties: the first index wins), or every other frame >= 1.01 x the minimum
    assert all(m is None or m >= 1.01 for m in margins), margins
    if int(d["clip"]) < 0:
        assert not filt.any() and all(m is None for m in margins)
        assert cuts == [t - geo.t_query for t in range(geo.t_center, len(audio), geo.t_center)]
    elif tag in GAP_TAGS:
        # every cut window overlaps a zero gap
        for t in range(geo.t_center, len(audio), geo.t_center):
            lo, hi = t - geo.t_query, t + geo.t_query
            assert any(a * 16000 < hi and b * 16000 > lo for a, b in d["zero_spans"]), t


@pytest.mark.parametrize("tag", TAGS)
def test_exact_highpass_is_scipy_bit_for_bit(tag):
    import polgen_rvc_amd  # noqa: F401
    from oracle import pipeline as OP
    from polgen_rvc_amd import _lib
    d, audio = _recipe(tag)
    for x in (audio.astype(np.float64), audio.astype(np.float64)[:int(0.6 * len(audio))]):
        ref = OP.highpass(x)
        got = _lib.highpass_exact(x)
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), np.abs(got - ref).max()


def test_exact_highpass_rejects_short_input():
    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd import _lib
    with pytest.raises(_lib.RvcxError):
        _lib.highpass_exact(np.ones(18))
    assert np.array_equal(_lib.highpass_exact(np.zeros(19)), np.zeros(19))
