#!/usr/bin/env python3
"""Times of index building (rvcx_kmeans / build_index): per-iteration ms and the share of rows that took the exact scan for
C3's index (65 536 x 768, k = 1 680) and for the reduction step (1 000 000 x 768, k = 10 000), the wall time of build_index
on C3's rows, and one float32 numpy Lloyd step on this host for the first case -- the only comparison there is (the parent
has no such path, faiss is not installed).  Per-iteration time = (t(1 + iters) - t(1)) / iters, so the upload and the split
of the data matrix are not in it.  Not part of bench.py; no bar.

    python tools/bench_index_build.py [--iters 3] [--skip-large] [--out profiles/bench_index_build.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import polgen_rvc_amd  # noqa: E402,F401
from polgen_rvc_amd import _lib  # noqa: E402
from polgen_rvc_amd.index_build import build_index  # noqa: E402


def data(n, dim, seed=0):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((64, dim), dtype=np.float32)
    X = cen[rng.integers(0, 64, n)]
    X += 0.5 * rng.standard_normal((n, dim), dtype=np.float32)
    return X


def case(ctx, n, dim, k, iters):
    X = data(n, dim)
    init = X[np.random.default_rng(0).choice(n, k, replace=False)]
    t = []
    for it in (1, 1, 1 + iters):                              # the first call also grows the arena
        t0 = time.perf_counter()
        r = ctx.kmeans(X, init, it)
        t.append(time.perf_counter() - t0)
    ex = ctx.kmeans_exhaustive()
    return dict(n=n, dim=dim, k=k, iters=iters, ms_first_call=round(1e3 * t[0], 1), ms_one_iteration_call=round(1e3 * t[1], 1),
                ms_per_iteration=round(1e3 * (t[2] - t[1]) / iters, 2), exhaustive_share=round(ex / (n * (1 + iters)), 5),
                objective=[float(v) for v in r["objective"]], splits=r["splits"].tolist()), X, init


def numpy_step(X, C):
    t0 = time.perf_counter()
    e = (C * C).sum(1)[None, :] - 2.0 * (X @ C.T)
    a = e.argmin(1)
    sums = np.zeros_like(C)
    np.add.at(sums, a, X)
    cnt = np.bincount(a, minlength=len(C))
    _ = sums / np.maximum(cnt, 1)[:, None]
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_index_build.json"))
    a = ap.parse_args()
    ctx = _lib.Context(0)
    res = {}
    res["c3_index"], X, init = case(ctx, 65536, 768, 1680, a.iters)
    res["c3_index"]["numpy_f32_step_ms"] = round(numpy_step(X, init), 1)
    t0 = time.perf_counter()
    ix = build_index(ctx, X, None, version="v2")
    res["build_index_c3"] = dict(rows=len(X), lists=len(ix.centroids), niter=20, wall_s=round(time.perf_counter() - t0, 2))
    del X
    if not a.skip_large:
        res["reduction"], _, _ = case(ctx, 1_000_000, 768, 10_000, a.iters)
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
