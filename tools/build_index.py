#!/usr/bin/env python3
"""Build a retrieval index on the GPU ("train index" of the RVC UIs; polgen-rvc_amd/index_build.py): from stacked HuBERT
features, or from a directory of 16 kHz-able audio through the resident HuBERT.

    python tools/build_index.py --features total_fea.npy --out logs/voice [--name voice] [--version v2]
    python tools/build_index.py --audio DIR --hubert hubert_base.pt --out voice.index

--out: a file name, or a directory that receives added_IVF{n}_Flat_nprobe_1_{name}_{version}.index.  More than
--reduce-above rows are replaced by --reduce-to k-means centres first.  The clustering is the one include/rvcx.h defines,
not faiss's or scikit-learn's: the file holds other centres than one a UI builds from the same features."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

AUDIO_EXT = (".wav", ".flac")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", help="(n, 768 | 256) float32 .npy of stacked HuBERT features (total_fea.npy)")
    src.add_argument("--audio", help="directory of WAV / FLAC clips; read through load_audio (mono, 16 kHz)")
    ap.add_argument("--hubert", help="HuBERT checkpoint (with --audio)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="model")
    ap.add_argument("--version", default="v2", choices=["v1", "v2"])
    ap.add_argument("--reduce-above", type=int, default=200_000)
    ap.add_argument("--reduce-to", type=int, default=10_000)
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    import polgen_rvc_amd  # noqa: F401
    from polgen_rvc_amd.index_build import build_index, features_from_audio
    from polgen_rvc_amd.infer import infer as I
    ctx = I._context(a.device)
    t0 = time.perf_counter()
    if a.features:
        feats = np.load(a.features)
    else:
        if not a.hubert:
            ap.error("--audio needs --hubert")
        I.load_hubert(a.device, False, a.hubert)
        files = sorted(f for f in os.listdir(a.audio) if f.lower().endswith(AUDIO_EXT))
        if not files:
            ap.error(f"no WAV / FLAC files in {a.audio}")
        clips = [I.load_audio(os.path.join(a.audio, f), 16000) for f in files]      # mono 16 kHz (resampled on the GPU)
        with ctx.lock:
            feats = features_from_audio(ctx, clips, a.version)
    with ctx.lock:
        ix = build_index(ctx, feats, a.out, name=a.name, version=a.version, reduce_above=a.reduce_above,
                         reduce_to=a.reduce_to, niter=a.niter, seed=a.seed)
    sizes = np.bincount(ix.assign, minlength=len(ix.centroids))
    print(f"{ix.path}: {len(feats)} rows -> {len(ix.vectors)} vectors x {ix.vectors.shape[1]} in {len(ix.centroids)} lists "
          f"(sizes {sizes.min()} .. {sizes.max()}, {int((sizes == 0).sum())} empty), {time.perf_counter() - t0:.1f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
