"""Build a retrieval index on the GPU: what the RVC UIs call "train index".

The UIs stack the voice's HuBERT features, reduce them to 10 000 k-means centres when there are more than 200 000, train
the coarse quantiser of a faiss ``IVF{n},Flat`` index on them, add the rows and write
``added_IVF{n}_Flat_nprobe_1_{name}_{version}.index``.  The reference tree ships no such trainer and neither faiss nor
scikit-learn is a dependency here: the clustering is the one ``include/rvcx.h`` defines ("index building":
``Context.kmeans``), the filing is the IVF search's own coarse quantiser (``Context.ivf_assign``), the file is written by
``index_io.write_index``.  Parity with faiss's k-means (random init with seed 1234, stochastic splitting) and with
``MiniBatchKMeans`` is unpinned: an index built here holds other centres than one built by a UI from the same features.
"""
from __future__ import annotations

import math
import os

import numpy as np

from .index_io import IndexFile, write_index

WIDTHS = {"v1": 256, "v2": 768}


def ivf_lists(n: int) -> int:
    """number of inverted lists the UIs choose for n stored rows: min(int(16 sqrt(n)), n // 39), at least 1"""
    n = int(n)
    return max(1, min(int(16 * math.sqrt(n)), n // 39))


def _width(version, width):
    if version not in WIDTHS:
        raise ValueError(f"version must be 'v1' or 'v2', got {version!r}")
    return WIDTHS[version] if width is None else int(width)


def features_from_audio(ctx, wavs16k, version="v2", *, width=None):
    """Stack the frames of 16 kHz mono clips as the conversion would see them: HuBERT layer 12 ("v2", the model's embed_dim:
    768) or final_proj of layer 9 ("v1", 256).  Clips are taken as given (no slicing, no normalisation).  ``width``: the
    feature width of a reduced-size HuBERT (its embed_dim / final_proj width) instead of the version's."""
    width = _width(version, width)
    rows = []
    for w in wavs16k:
        w = np.asarray(w, np.float32).ravel()
        rows.append(ctx.index_features(w, width)[0])
    if not rows:
        raise ValueError("features_from_audio: no clips")
    return np.ascontiguousarray(np.concatenate(rows, 0), np.float32)


def _train(ctx, x, k, niter, seed):
    """k centres of x: Lloyd's iterations from k distinct rows drawn by the seeded generator"""
    pick = np.random.default_rng(seed).choice(x.shape[0], k, replace=False)
    return ctx.kmeans(x, x[pick], niter)["centroids"]


def build_index(ctx, features, path=None, *, name="model", version="v2", reduce_above=200_000, reduce_to=10_000,
                niter=20, seed=0, width=None) -> IndexFile:
    """features (n, 768 | 256) -> an ``IVF{ivf_lists(n)},Flat`` index with nprobe = 1, as an ``IndexFile`` that
    ``ctx.load_index_ivf(ix.vectors, ix.centroids, ix.assign, ix.nprobe)`` takes as is.  More rows than ``reduce_above``
    are first replaced by ``reduce_to`` k-means centres.  ``path``: a file name, or a directory that receives
    ``added_IVF{nlist}_Flat_nprobe_1_{name}_{version}.index``; None writes nothing.  ``width``: see features_from_audio."""
    width = _width(version, width)
    x = np.ascontiguousarray(features, np.float32)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("build_index: features must be a non-empty (n, dim) matrix")
    if x.shape[1] != width:
        raise ValueError(f"build_index: {version} features are {width} wide, got {x.shape[1]}")
    if x.shape[0] > reduce_above:
        x = _train(ctx, x, int(reduce_to), niter, seed)
    n = x.shape[0]
    nlist = ivf_lists(n)
    centroids = _train(ctx, x, nlist, niter, seed)
    assign = ctx.ivf_assign(x, centroids)
    ix = IndexFile(x, centroids, assign, 1)
    if path is not None:
        if os.path.isdir(path):
            path = os.path.join(path, f"added_IVF{nlist}_Flat_nprobe_1_{name}_{version}.index")
        write_index(path, ix.vectors, ix.centroids, ix.assign, ix.nprobe)
        ix.path = path
    return ix
