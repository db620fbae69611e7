#!/usr/bin/env python3
"""Times of the noise reduction (rvcx_fx_denoise, include/rvcx.h stage 15): `--clips` stereo clips of `--seconds` s at `--rate`
Hz in ONE call (default 64 x 30 s at 48 kHz), one stereo clip and one mono clip, each in mode 0 (with a shared 1 s noise clip)
and mode 1; then the host twin on one mono clip.  One process; per case one warm-up call, then `--repeats` timed calls: wall
clock around the whole call (host arrays in, host arrays out) and the per-kernel device times of rvcx_last_timing, medians over
the repeats.  For the analysis, smoothing and synthesis kernels the bytes they have to move (the arrays they read and write
once, halos not counted) are set against their time.  Not part of bench.py; no bar is fixed in advance (LABNOTES 23 sets the
time per clip beside the effects chain's).

    python tools/bench_denoise.py [--clips 64] [--seconds 30] [--rate 48000] [--repeats 3] [--out profiles/bench_denoise.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import polgen_rvc_amd  # noqa: E402,F401
from polgen_rvc_amd import _lib, synthetic as S  # noqa: E402

NAMES = ["copies_in", "analysis", "smoothing", "stats_or_floor", "mask", "synthesis", "overlap_add", "copies_out", "total"]


def make_clips(clips, seconds, rate, seed, scale=0.5):
    n = int(round(seconds * rate))
    base = []
    for k in range(min(clips, 4)):
        a = S.make_clip(seed + k, min(seconds, 30.0) + 0.1)
        idx = ((np.arange(n, dtype=np.int64) * 16000) // rate) % a.shape[0]
        x = np.stack([a[idx], np.roll(a, 1234)[idx]], axis=1).astype(np.float32)
        base.append(np.ascontiguousarray(x * (scale / np.abs(x).max())))
    return [base[i % len(base)] for i in range(clips)]


def add_hiss(items, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(x + 0.01 * rng.standard_normal(x.shape).astype(np.float32)) for x in items]


def run(ctx, items, rate, mode, clip, repeats):
    ch = 1 if items[0].ndim == 1 else items[0].shape[1]
    p = _lib.FxDenoiseParams.make(rate, ch, mode=mode)
    ctx.fx_denoise(items, rate, p, noise=clip)                    # warm-up: the arena grows here
    wall, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ys = ctx.fx_denoise(items, rate, p, noise=clip)
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_denoise_timing()
        stages.append([tm[k] for k in NAMES])
    st = dict(zip(NAMES, np.median(np.asarray(stages), axis=0)))
    clips, n = len(items), items[0].shape[0]
    T, N, nf, nt = _lib.fx_denoise_frames(n, rate)
    bins = clips * ch * T * (N // 2 + 1)
    # bytes each kernel reads and writes once: x -> D + A2; A2 -> S; m + D -> windowed frames
    moved = dict(analysis=clips * ch * n * 4 + bins * 12, smoothing=bins * 8, synthesis=bins * 12 + clips * ch * T * N * 4)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))      # noqa: E731
    return dict(mode=mode, clips=clips, channels=ch, frames=T, N=N, nf=nf, nt=nt, lanes_of_the_floor=clips * ch * (N // 2 + 1),
                groups=ctx.fx_last_passes()[1], wall_ms_runs=[round(v, 2) for v in wall],
                wall_ms_median=round(float(np.median(wall)), 2), wall_ms_per_clip=round(float(np.median(wall)) / clips, 3),
                device_ms_per_clip=round(float(st["total"]) / clips, 3),
                kernel_ms_median={k: round(float(v), 3) for k, v in st.items()},
                kernel_ms_per_clip={k: round(float(v) / clips, 4) for k, v in st.items()},
                bytes_moved={k: int(v) for k, v in moved.items()},
                gb_per_s={k: round(v / max(float(st[k]), 1e-6) / 1e6, 1) for k, v in moved.items()},
                level_out_over_in=round(rms(ys[0]) / rms(items[0]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_denoise.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_denoise: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    name, _ = _lib.device_info(0)
    clips = add_hiss(make_clips(a.clips, a.seconds, a.rate, 400), 1)
    mono = [np.ascontiguousarray(clips[0][:, 0])]
    hiss = 0.01 * np.random.default_rng(2).standard_normal((a.rate, 2)).astype(np.float32)
    res = dict(metric="fx_denoise_ms", device=name, clips=a.clips, seconds=a.seconds, rate=a.rate, repeats=a.repeats,
               tiles=_lib.fx_denoise_tiles(), effects_chain_ms_per_clip=1.7, cases={})
    for mode in (0, 1):
        for tag, items in ((f"batch_{a.clips}", clips), ("single_stereo", clips[:1]), ("single_mono", mono)):
            clip = None if mode == 1 else (hiss if items[0].ndim == 2 else np.ascontiguousarray(hiss[:, 0]))
            key = f"{tag}_mode{mode}"
            res["cases"][key] = run(ctx, items, a.rate, mode, clip, a.repeats)
            print(f"  {key}: {res['cases'][key]}", flush=True)
    ctx.close()
    for mode in (0, 1):                                            # the host twin on one mono clip
        p = _lib.FxDenoiseParams.make(a.rate, 1, mode=mode)
        t0 = time.perf_counter()
        _lib.fx_denoise_host(mono[0], a.rate, p, noise=None if mode == 1 else np.ascontiguousarray(hiss[:, 0]))
        res["cases"][f"host_twin_mono_mode{mode}"] = dict(wall_ms=round(1e3 * (time.perf_counter() - t0), 1))
        print(f"  host twin, mode {mode}: {res['cases'][f'host_twin_mono_mode{mode}']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
