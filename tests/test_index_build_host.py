"""CPU: the host side of index building -- the list-count rule, the index writer against the reader and against the
test-side faiss encoder, and the float64 restatement's own properties (tests/kmeans_reference.py)."""
import os

import numpy as np
import pytest

import faiss_writer as FW
import kmeans_reference as KR


def test_ivf_lists_rule():
    from polgen_rvc_amd.index_build import ivf_lists
    want = {38: 1, 39: 1, 4099: 105, 65536: 1680, 200000: 5128}
    for n, v in want.items():
        assert ivf_lists(n) == v == KR.ivf_lists(n), n
    assert ivf_lists(1) == 1


def _index(seed=0, n=300, d=32, nlist=7):
    rng = np.random.default_rng(seed)
    big = rng.standard_normal((n, d)).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    assign = rng.integers(0, nlist - 1, n).astype(np.int32)      # the last list stays empty
    assign[rng.permutation(n)[:5]] = 0
    return big, cent, assign


def test_write_index_is_the_inverse_of_read_index(tmp_path):
    from polgen_rvc_amd.index_io import index_bytes, read_index, write_index
    big, cent, assign = _index()
    assert (np.bincount(assign, minlength=len(cent)) == 0).any()
    p = os.path.join(tmp_path, "flat.index")
    write_index(p, big)
    ix = read_index(p)
    assert not ix.is_ivf and ix.vectors.dtype == np.float32 and np.array_equal(ix.vectors, big)
    assert open(p, "rb").read() == FW.flat_bytes(big)
    p = os.path.join(tmp_path, "ivf.index")
    write_index(p, big, cent, assign, nprobe=1)
    ix = read_index(p)
    assert ix.is_ivf and ix.nprobe == 1
    assert np.array_equal(ix.vectors, big) and np.array_equal(ix.centroids, cent) and np.array_equal(ix.assign, assign)
    # the test-side encoder lists the members of a list by np.where: ascending ids, the writer's order
    assert open(p, "rb").read() == FW.ivf_flat_bytes(big, cent, assign, nprobe=1)
    assert index_bytes(big, cent, assign, 1) == open(p, "rb").read()


def test_write_index_refuses_bad_lists():
    from polgen_rvc_amd.index_io import index_bytes
    big, cent, assign = _index()
    with pytest.raises(ValueError):
        index_bytes(big, cent, None)
    with pytest.raises(ValueError):
        index_bytes(big, None, assign)
    bad = assign.copy()
    bad[3] = len(cent)
    with pytest.raises(ValueError, match="out of range"):
        index_bytes(big, cent, bad)
    with pytest.raises(ValueError):
        index_bytes(big, cent, assign[:-1])


def test_build_index_refuses_a_width_that_is_not_the_versions():
    from polgen_rvc_amd.index_build import build_index
    with pytest.raises(ValueError, match="768 wide"):
        build_index(None, np.zeros((50, 256), np.float32), version="v2")
    with pytest.raises(ValueError, match="version"):
        build_index(None, np.zeros((50, 256), np.float32), version="v3")


def test_reference_split_rule_leaves_no_empty_cluster():
    X, init = KR.duplicate_init_case()
    steps = KR.run(X, init, 4)
    assert len(steps[0]["pairs"]) == 2 and [c for c, _ in steps[0]["pairs"]] == [40, 77]   # ties go to the smaller id: 7 wins
    assert (steps[3]["counts"] > 0).all()                     # no cluster is empty after iteration 3
    assert all(s["counts"].sum() == len(X) for s in steps)


def test_reference_objective_does_not_rise_without_a_split():
    rng = np.random.default_rng(1)
    X, _ = KR.blobs(rng, 1031, 64)
    steps = KR.run(X, X[rng.choice(1031, 37, replace=False)], 6)
    checked = 0
    for a, b in zip(steps, steps[1:]):
        if not a["pairs"]:
            assert b["objective"] <= a["objective"] * (1 + 1e-12)
            checked += 1
    assert checked >= 3
