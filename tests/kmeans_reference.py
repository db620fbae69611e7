"""float64 restatement of index building as include/rvcx.h defines it ("index building"): one Lloyd step with the
deterministic split of empty clusters, the list-count rule of the RVC UIs, a nearest-centroid search.  The yardstick of
tests/test_index_build_host.py and tests/test_gpu_index_build.py; never imported by the product."""
import math

import numpy as np

UP, DN = np.float32(1 + 2.0 ** -10), np.float32(1 - 2.0 ** -10)


def ivf_lists(n):
    return max(1, min(int(16 * math.sqrt(n)), n // 39))


def blobs(rng, n, dim, ncen=64, scale=1.0, noise=0.5):
    """the issue's test data: cen = scale N(0,1) (ncen, dim), X = cen[randint(ncen)] + noise N(0,1), float32"""
    cen = scale * rng.standard_normal((ncen, dim))
    lab = rng.integers(0, ncen, n)
    return (cen[lab] + noise * rng.standard_normal((n, dim))).astype(np.float32), lab


def duplicate_init_case():
    """n = 4099, k = 105, D = 256, an init with three identical rows (7, 40, 77): two clusters start empty"""
    rng = np.random.default_rng(0)
    X, _ = blobs(rng, 4099, 256)
    init = X[rng.choice(4099, 105, replace=False)].copy()
    init[40] = init[7]
    init[77] = init[7]
    return X, init


def assign_case(n, k, dim, seed=0):
    """X = blobs, centroids = k rows of X + 0.05 N(0,1) (float32)"""
    rng = np.random.default_rng(seed)
    X, _ = blobs(rng, n, dim)
    C = (X[rng.choice(n, k, replace=False)] + 0.05 * rng.standard_normal((k, dim))).astype(np.float32)
    return X, C


def outlier_case(which):
    """assign_case(1031, 37, 256) with one value beyond fp16 range: which = "row": X[5, 3] = 1e5 (that row cannot be split
    into fp16 halves); "centroid": C[2, 7] = 1e5 (the centroids get no split image: no pre-filter at all)"""
    X, C = assign_case(1031, 37, 256)
    if which == "row":
        X[5, 3] = 1e5
    else:
        C[2, 7] = 1e5
    return X, C


def pair_e(x, c):
    """e(x, c) = |c|^2 - 2 x.c for every pair, float64: (n, k)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def nearest(x, c):
    """(argmin, best e, margin to the second best e) per row; ties: the first (smallest id)"""
    e = pair_e(x, c)
    a = np.argmin(e, axis=1)
    best = e[np.arange(len(a)), a]
    if e.shape[1] > 1:
        e2 = e.copy()
        e2[np.arange(len(a)), a] = np.inf
        margin = e2.min(1) - best
    else:
        margin = np.full(len(a), np.inf)
    return a, best, margin


def margin_bound(x, c, scale=2.0 ** -15):
    """per row: scale (|x| max|c| + max|c|^2) -- a float32 evaluation may pick another centroid inside it"""
    xn = np.sqrt((np.asarray(x, np.float64) ** 2).sum(1))
    cm = np.sqrt((np.asarray(c, np.float64) ** 2).sum(1).max())
    return scale * (xn * cm + cm * cm)


def split_pairs(counts):
    """(empty cluster, cluster it halves) in treatment order, by the running bookkeeping of the header"""
    book = np.asarray(counts, np.int64).copy()
    pairs = []
    for c in np.nonzero(np.asarray(counts) == 0)[0]:
        j = int(np.argmax(book))                     # the first maximum: ties go to the smaller id
        pairs.append((int(c), j))
        book[c] = book[j] // 2
        book[j] -= book[c]
    return pairs


def apply_split(cent32, pairs):
    """the float32 perturbation, in place, in order"""
    even = (np.arange(cent32.shape[1]) % 2) == 0
    for c, j in pairs:
        v = cent32[j].copy()
        cent32[c] = v * np.where(even, UP, DN).astype(np.float32)
        cent32[j] = v * np.where(even, DN, UP).astype(np.float32)
    return cent32


def step(x, cent):
    """one iteration from the float32 centroids `cent`: dict(assign, counts, objective, centroids (float32, after the
    split), mean (float64 member means; empty clusters keep their centroid), pairs, margin)"""
    x64 = np.asarray(x, np.float64)
    a, best, margin = nearest(x, cent)
    k = cent.shape[0]
    counts = np.bincount(a, minlength=k)
    obj = float(((x64 * x64).sum(1) + best).sum())
    mean = np.asarray(cent, np.float64).copy()
    sums = np.zeros((k, x64.shape[1]))
    np.add.at(sums, a, x64)
    nz = counts > 0
    mean[nz] = sums[nz] / counts[nz, None]
    new = mean.astype(np.float32)
    pairs = split_pairs(counts)
    apply_split(new, pairs)
    return dict(assign=a, counts=counts, objective=obj, centroids=new, mean=mean, pairs=pairs, margin=margin)


def run(x, init, iters):
    cent, out = np.asarray(init, np.float32), []
    for _ in range(iters):
        out.append(step(x, cent))
        cent = out[-1]["centroids"]
    return out
