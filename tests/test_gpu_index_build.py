"""GPU: index building (include/rvcx.h "index building"; csrc/kmeans.hip, index_build.py) against the float64 restatement
in tests/kmeans_reference.py, the writer / reader / IVF search round trip and the public path."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_reference as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, k, D): the real widths; n off every tile size; k below one tile, above one tile, off a tile
SHAPES = [(4099, 700, 768), (1031, 37, 256), (4099, 33, 768)]


@functools.lru_cache(maxsize=None)
def _assign_case(n, k, dim):
    X, C = KR.assign_case(n, k, dim)
    a, best, margin = KR.nearest(X, C)
    keep = margin > KR.margin_bound(X, C)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C, a, keep


@functools.lru_cache(maxsize=None)
def _dup_case():
    X, init = KR.duplicate_init_case()
    X.setflags(write=False)
    init.setflags(write=False)
    return X, init, KR.run(X, init, 3)


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("centroids", "assign", "counts", "objective", "splits"))


@pytest.mark.parametrize("shape", SHAPES)
def test_assign_step_vs_float64(ctx, shape):
    """1: the device's assignment equals the float64 argmin on every row whose float64 margin between best and second best
    exceeds 2^-15 (|x| max|c| + max|c|^2); at most 1 % of the rows are excluded."""
    X, C, ref, keep = _assign_case(*shape)
    r = ctx.kmeans(X, C, 1)
    excluded = 1.0 - keep.mean()
    wrong = int((r["assign"][keep] != ref[keep]).sum())
    print(f"assign {shape}: excluded {100 * excluded:.2f} %, wrong {wrong}, exhaustive {ctx.kmeans_exhaustive()} of {shape[0]}")
    assert excluded <= 0.01
    assert wrong == 0


_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import polgen_rvc_amd
from polgen_rvc_amd import _lib
import kmeans_reference as KR
ctx = _lib.Context(0)
out = {{}}
for i, (n, k, d, iters) in enumerate({cases!r}):
    X, C = KR.outlier_case(n) if isinstance(n, str) else KR.assign_case(n, k, d)
    r = ctx.kmeans(X, C, iters)
    for key, v in r.items():
        out[f"{{key}}_{{i}}"] = v
    out[f"exhaustive_{{i}}"] = np.int64(ctx.kmeans_exhaustive())
ctx.close()
np.savez({path!r}, **out)
"""


def test_same_bits_without_the_prefilter(ctx, tmp_path):
    """2: RVCX_KMEANS_PREFILTER=0 (read once per process: a fresh child) scans every row exactly and gives the same bits;
    the default run certified something on the first shape."""
    cases = [(4099, 700, 768, 2), (4099, 33, 768, 1)]
    path = str(tmp_path / "noprefilter.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)), cases=cases, path=path)
    env = dict(os.environ, RVCX_KMEANS_PREFILTER="0")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    d = np.load(path)
    for i, (n, k, dim, iters) in enumerate(cases):
        X, C = KR.assign_case(n, k, dim)
        r = ctx.kmeans(X, C, iters)
        ex = ctx.kmeans_exhaustive()
        print(f"prefilter {(n, k, dim)}: exhaustive rows {ex} of {n * iters} with the filter, {int(d[f'exhaustive_{i}'])} without")
        assert int(d[f"exhaustive_{i}"]) == n * iters > 0
        if i == 0:
            assert ex < n
        for key, v in r.items():
            assert np.array_equal(v, d[f"{key}_{i}"]), (i, key)


def test_values_beyond_fp16_range_are_demoted_to_the_scan(ctx, tmp_path):
    """2b: a row with a value the fp16 split cannot hold takes the exact scan (the others keep the filter); centroids beyond
    the split's range switch the filter off for the iteration.  Either way the bits are those of the run without the
    pre-filter, and the outlier's own row has the float64 argmin."""
    cases = [("row", 0, 0, 1), ("row", 0, 0, 2), ("centroid", 0, 0, 1)]
    path = str(tmp_path / "outliers.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)), cases=cases, path=path)
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RVCX_KMEANS_PREFILTER="0"), check=True, timeout=300)
    d = np.load(path)
    for i, (which, _, _, iters) in enumerate(cases):
        X, C = KR.outlier_case(which)
        n = len(X)
        r = ctx.kmeans(X, C, iters)
        ex = ctx.kmeans_exhaustive()
        print(f"outlier {which}, iters {iters}: exhaustive rows {ex} of {n * iters}")
        assert int(d[f"exhaustive_{i}"]) == n * iters
        if which == "row" and iters == 1:
            assert 1 <= ex < n                     # the marked row, and whoever else missed the certificate
            ref, _, margin = KR.nearest(X, C)
            assert margin[5] > KR.margin_bound(X, C)[5] and r["assign"][5] == ref[5]
        if which == "centroid":
            assert ex == n                         # no split image of the centroids: every row scanned
        for key, v in r.items():
            assert np.isfinite(v).all() and np.array_equal(v, d[f"{key}_{i}"]), (which, iters, key)


def _sequential_mean(X, members):
    """the device's update restated exactly: float64 sum in ascending row order, one division, one rounding"""
    acc = np.zeros(X.shape[1], np.float64)
    for m in members:
        acc += X[m].astype(np.float64)
    return (acc / len(members)).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_update_is_the_member_mean(ctx, shape):
    """3: given the device's own assignment, the centroids are the float64 member means within one rounding
    (2^-23 |ref| + 2^-40 max|x|), counts = bincount(assign), and a second call gives the same bits."""
    X, C, _, _ = _assign_case(*shape)
    r = ctx.kmeans(X, C, 1)
    k = C.shape[0]
    assert np.array_equal(r["counts"], np.bincount(r["assign"], minlength=k))
    assert r["counts"].sum() == len(X) and r["splits"][0] == int((r["counts"] == 0).sum())
    X64 = X.astype(np.float64)
    xmax = np.abs(X64).max()
    worst = 0.0
    treated = {c for pair in KR.split_pairs(r["counts"]) for c in pair}      # perturbed by the split: test 4 checks those
    for c in np.nonzero(r["counts"])[0]:
        if c in treated:
            continue
        ref = X64[r["assign"] == c].mean(0)
        tol = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * xmax
        err = np.abs(r["centroids"][c].astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
    print(f"update {shape}: worst error / tolerance {worst:.3f}")
    assert 0 < worst <= 1.0
    assert _same(r, ctx.kmeans(X, C, 1))


def test_empty_clusters_are_split_by_the_rule(ctx):
    """4: an init with three identical rows leaves two clusters empty; both are treated by the rule, bit for bit, with the
    float64 run's choice of the cluster to halve; nobody is empty after iteration 3."""
    X, init, ref = _dup_case()
    r = ctx.kmeans(X, init, 1)
    assert r["splits"][0] == 2 and np.array_equal(np.nonzero(r["counts"] == 0)[0], [40, 77])
    pairs = ref[0]["pairs"]
    assert pairs == KR.split_pairs(r["counts"]) and [c for c, _ in pairs] == [40, 77]
    want = r["centroids"].copy()
    for _, j in pairs:
        want[j] = _sequential_mean(X, np.nonzero(r["assign"] == j)[0])
    KR.apply_split(want, pairs)
    for c, j in pairs:
        assert np.array_equal(want[c].view(np.uint32), r["centroids"][c].view(np.uint32)), (c, j)
        assert np.array_equal(want[j].view(np.uint32), r["centroids"][j].view(np.uint32)), (c, j)
        assert not np.array_equal(r["centroids"][c], r["centroids"][j])
    r4 = ctx.kmeans(X, init, 4)
    assert r4["splits"][0] == 2 and (r4["counts"] > 0).all()


# Relative difference of objective[i] from the float64 trajectory, teacher-forced per step.  Worst case by derivation: every
# e within 2^-17 (|x||c| + |c|^2) of the float64 value, all errors of one sign, against |x|^2 + e >= 0.2 |x|^2 on this data:
# below 1e-4.  Measured at the first GPU run (LABNOTES 19): 1.15e-8, 1.98e-9, 3.11e-8 on the three steps; the bar is 3 x the
# largest.
OBJECTIVE_MEASURED = 3.11e-8
OBJECTIVE_WORST_CASE = 1e-4


def test_a_run_is_its_steps(ctx):
    """5: kmeans(iters = 3) equals three chained iters = 1 calls in every output bit; each step's objective follows the
    float64 trajectory when the device starts the step from the reference's float32-rounded centroids."""
    X, init, ref = _dup_case()
    r3 = ctx.kmeans(X, init, 3)
    cur, chain = init, []
    for i in range(3):
        chain.append(ctx.kmeans(X, cur, 1))
        cur = chain[-1]["centroids"]
    assert np.array_equal(r3["centroids"], chain[2]["centroids"]) and np.array_equal(r3["assign"], chain[2]["assign"])
    assert np.array_equal(r3["counts"], chain[2]["counts"])
    for i in range(3):
        assert r3["objective"][i] == chain[i]["objective"][0] and r3["splits"][i] == chain[i]["splits"][0], i
    rel = []
    for i in range(3):
        start = init if i == 0 else ref[i - 1]["centroids"]
        got = ctx.kmeans(X, start, 1)["objective"][0]
        rel.append(abs(got - ref[i]["objective"]) / ref[i]["objective"])
    print("objective: relative difference per teacher-forced step " + ", ".join(f"{v:.3e}" for v in rel))
    bar = 3 * OBJECTIVE_MEASURED
    assert bar <= OBJECTIVE_WORST_CASE and max(rel) <= bar, (rel, bar)


def test_fixed_point_on_separated_blobs(ctx):
    """6: 24 well separated blobs, init one row per blob: the assignment equals the labels after iteration 1 and stays."""
    rng = np.random.default_rng(3)
    X, lab = KR.blobs(rng, 1031, 256, ncen=24, scale=4.0, noise=0.3)
    init = X[[int(np.nonzero(lab == b)[0][0]) for b in range(24)]]
    r1, r3 = ctx.kmeans(X, init, 1), ctx.kmeans(X, init, 3)
    assert np.array_equal(r1["assign"], lab) and np.array_equal(r3["assign"], lab)
    assert r3["objective"][1] == r3["objective"][2] and r3["objective"][1] < r3["objective"][0]
    assert (r3["splits"] == 0).all()


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_ivf_assign_vs_float64(ctx, shape):
    """7: the filing equals the float64 nearest centroid outside the margin of test 1, with the same cap."""
    X, C, ref, keep = _assign_case(*shape)
    a = ctx.ivf_assign(X, C)
    assert a.dtype == np.int32 and 1.0 - keep.mean() <= 0.01
    assert np.array_equal(a[keep], ref[keep])


@functools.lru_cache(maxsize=None)
def _features_4099():
    X, _ = KR.blobs(np.random.default_rng(5), 4099, 256)
    X.setflags(write=False)
    return X


def test_build_index_end_to_end(ctx, tmp_path):
    """8: build_index writes added_IVF105_Flat_nprobe_1_*.index; read back and loaded, the IVF search returns the ids of the
    float64 oracle on the same centroids and lists, and stored rows find themselves."""
    from oracle import pipeline as OP
    from polgen_rvc_amd.index_build import build_index, ivf_lists
    from polgen_rvc_amd.index_io import read_index
    X = _features_4099()
    built = build_index(ctx, X, str(tmp_path), name="blobs", version="v1", niter=4)
    path = os.path.join(tmp_path, "added_IVF105_Flat_nprobe_1_blobs_v1.index")
    assert ivf_lists(4099) == 105 and built.path == path and os.path.exists(path)
    ix = read_index(path)
    assert ix.is_ivf and ix.nprobe == 1 and ix.centroids.shape == (105, 256)
    assert np.array_equal(ix.vectors, X) and np.array_equal(ix.assign, built.assign)
    assert np.array_equal(ix.centroids, built.centroids)
    try:
        ctx.load_index_ivf(ix.vectors, ix.centroids, ix.assign, ix.nprobe)
        rng = np.random.default_rng(9)
        fresh = (X[rng.choice(4099, 200, replace=False)] + 0.1 * rng.standard_normal((200, 256))).astype(np.float32)
        for name, q in (("fresh", fresh), ("stored", np.ascontiguousarray(X[:200]))):
            _, _, margin = KR.nearest(q, ix.centroids)
            keep = margin > KR.margin_bound(q, ix.centroids)
            assert 1.0 - keep.mean() <= 0.01, name
            q = np.ascontiguousarray(q[keep])
            for T in (1, len(q)):
                _, ids, _ = ctx.index_blend(q[:T], 1.0)
                _, want, _ = OP.index_blend_ivf(q[:T], ix.vectors, ix.centroids, ix.assign, 1.0)
                assert np.array_equal(ids, want), (name, T)
                if name == "stored":
                    assert np.array_equal(ids[:, 0], np.nonzero(keep)[0][:T])
    finally:
        from polgen_rvc_amd.infer import pipeline as P
        ctx.load_index(None)
        P._INDEX_RESIDENT[id(ctx)] = None       # what VC._load_index believes is resident


def test_build_index_reduces_large_feature_sets(ctx, tmp_path):
    """9: more rows than reduce_above are replaced by reduce_to k-means centres before the lists are trained."""
    from polgen_rvc_amd.index_build import build_index
    from polgen_rvc_amd.index_io import read_index
    path = str(tmp_path / "reduced.index")
    build_index(ctx, _features_4099(), path, version="v1", reduce_above=1000, reduce_to=256, niter=3)
    ix = read_index(path)
    assert ix.vectors.shape == (256, 256) and ix.centroids.shape == (6, 256)
    assert ix.assign.min() >= 0 and ix.assign.max() < 6 and np.isfinite(ix.vectors).all()


def test_built_index_through_vc_pipeline(ctx, tmp_path):
    """10: VC.pipeline with file_index = the built file converts, and equals the conversion with that index loaded by hand."""
    from polgen_rvc_amd import synthetic as S
    from polgen_rvc_amd.index_build import build_index, features_from_audio
    from polgen_rvc_amd.index_io import read_index
    from polgen_rvc_amd.infer import infer as I, pipeline as P
    cfgs = (S.HUBERT_CFG_TINY, S.RMVPE_CFG_TINY, S.SYNTH_CFG_TINY)
    I._CTX[0] = ctx
    hub = I.load_hubert("cuda:0", False, None, state=S.hubert_state(cfgs[0], 4), cfg=cfgs[0])
    I.load_rmvpe("cuda:0", state=S.rmvpe_state(cfgs[1], 4), cfg=cfgs[1])
    cpt = S.synth_checkpoint(cfgs[2], 4)
    cpt["weight"] = S.synth_state(cfgs[2], 4, input_dim=cfgs[0]["embed_dim"])
    cpt, version, net_g, tgt_sr, vc = I.get_vc("cuda:0", False, I.Config(), None, cpt=cpt)
    E = cfgs[0]["embed_dim"]
    feats = features_from_audio(ctx, [S.make_clip(20 + i, 2.0) for i in range(3)], "v2", width=E)
    assert feats.shape[1] == E and feats.shape[0] >= 3 * 90
    built = build_index(ctx, feats, str(tmp_path), name="tiny", version="v2", niter=3, width=E)
    audio = S.make_clip(12, 2.0)
    vc.seed = 21
    try:
        pcm = vc.pipeline(hub, net_g, 0, audio, "x.wav", 0.0, "rmvpe+", built.path, 0.75, 1, 3, tgt_sr, 0, 1.0, "v2", 0.33,
                          128, None, 50, 1100)
        plain = vc.pipeline(hub, net_g, 0, audio, "x.wav", 0.0, "rmvpe+", None, 0, 1, 3, tgt_sr, 0, 1.0, "v2", 0.33,
                            128, None, 50, 1100)
        assert pcm.dtype == np.int16 and len(pcm) == len(plain) and not np.array_equal(pcm, plain)
        ix = read_index(built.path)
        ctx.load_index_ivf(ix.vectors, ix.centroids, ix.assign, ix.nprobe)
        p = vc._params(0.0, 0.75, 1.0, 0.33, 50, 1100, 0, f0_method="rmvpe+", hop_length=128)
        by_hand = ctx.convert_batch(net_g.model_id, [audio], p)[0]
        assert np.array_equal(pcm, by_hand)
    finally:
        ctx.load_index(None)
        P._INDEX_RESIDENT[id(ctx)] = None


def test_build_index_cli_from_a_features_file(ctx, tmp_path, capsys):
    """tools/build_index.py --features: argument parsing, the resident context and its lock, build_index, the file name"""
    import importlib.util
    from polgen_rvc_amd.index_io import read_index
    from polgen_rvc_amd.infer import infer as I
    I._CTX[0] = ctx
    spec = importlib.util.spec_from_file_location("build_index_cli", os.path.join(ROOT, "tools", "build_index.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    X = _features_4099()[:1031]
    np.save(tmp_path / "total_fea.npy", X)
    rc = cli.main(["--features", str(tmp_path / "total_fea.npy"), "--out", str(tmp_path), "--name", "cli", "--version", "v1",
                   "--niter", "3"])
    path = os.path.join(tmp_path, "added_IVF26_Flat_nprobe_1_cli_v1.index")
    assert rc == 0 and os.path.exists(path) and "26 lists" in capsys.readouterr().out
    ix = read_index(path)
    assert np.array_equal(ix.vectors, X) and ix.centroids.shape == (26, 256) and ix.nprobe == 1
    with pytest.raises(ValueError, match="768 wide"):
        cli.main(["--features", str(tmp_path / "total_fea.npy"), "--out", str(tmp_path), "--version", "v2"])


def test_refusals_leave_the_context_usable(ctx):
    """11: k > n, a width that is no multiple of 16, and a v1 width passed as v2 are refused by name."""
    from polgen_rvc_amd import _lib
    from polgen_rvc_amd.index_build import build_index
    rng = np.random.default_rng(2)
    X = rng.standard_normal((64, 32)).astype(np.float32)
    with pytest.raises(_lib.RvcxError, match="exceeds"):
        ctx.kmeans(X[:10], X[:11], 1)
    with pytest.raises(_lib.RvcxError, match="multiple of 16"):
        ctx.kmeans(rng.standard_normal((50, 100)).astype(np.float32), rng.standard_normal((4, 100)).astype(np.float32), 1)
    with pytest.raises(_lib.RvcxError, match="dim above 1024"):
        ctx.kmeans(np.zeros((8, 1040), np.float32), np.zeros((2, 1040), np.float32), 1)
    with pytest.raises(ValueError, match="768 wide"):
        build_index(ctx, np.zeros((100, 256), np.float32), version="v2")
    r = ctx.kmeans(X, X[:4], 2)
    assert r["counts"].sum() == 64 and np.isfinite(r["centroids"]).all() and r["objective"][1] <= r["objective"][0]
