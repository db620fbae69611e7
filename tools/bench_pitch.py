#!/usr/bin/env python3
"""Times of the pitch shift (rvcx_fx_pitch_shift, include/rvcx.h stages 13 and 14): `--clips` stereo clips of `--seconds` s
at `--rate` Hz in ONE call (default 64 x 30 s at 48 kHz) and one item of `--long-seconds` s (default 180), each at s = +3 and
s = -5 semitones.  One process; per case one warm-up call, then `--repeats` timed calls: wall clock around the whole call
(host arrays in, host arrays out) and the per-kernel device times of rvcx_last_timing, medians over the repeats.  Not part of
bench.py; no bar is fixed in advance (LABNOTES 22 sets the time per clip beside the effects chain's and the master's).

    python tools/bench_pitch.py [--clips 64] [--seconds 30] [--long-seconds 180] [--rate 48000] [--repeats 3]
                                [--out profiles/bench_pitch.json]"""
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

NAMES = ["copies_in", "transforms", "owners", "scan", "inverse_transforms", "overlap_add", "resampler", "copies_out", "total"]


def make_clips(clips, seconds, rate, seed, scale=0.5):
    n = int(round(seconds * rate))
    base = []
    for k in range(min(clips, 4)):
        a = S.make_clip(seed + k, min(seconds, 30.0) + 0.1)
        idx = ((np.arange(n, dtype=np.int64) * 16000) // rate) % a.shape[0]
        x = np.stack([a[idx], np.roll(a, 1234)[idx]], axis=1).astype(np.float32)
        base.append(np.ascontiguousarray(x * (scale / np.abs(x).max())))
    return [base[i % len(base)] for i in range(clips)]


def run(ctx, items, rate, semitones, repeats):
    ctx.fx_pitch_shift(items, rate, semitones)                    # warm-up: the arena grows here
    wall, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ys = ctx.fx_pitch_shift(items, rate, semitones)
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_stretch_timing()
        stages.append([tm[k] for k in NAMES])
    st = np.median(np.asarray(stages), axis=0)
    clips, n = len(items), items[0].shape[0]
    T, J, N = _lib.fx_stretch_frames(n, rate, _lib.fx_pitch_ratio(rate, semitones), rate)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))      # noqa: E731
    return dict(semitones=semitones, P=_lib.fx_pitch_ratio(rate, semitones), clips=clips, frames_in=T, frames_out=J, N=N,
                groups=ctx.fx_last_passes()[1], wall_ms_runs=[round(v, 2) for v in wall],
                wall_ms_median=round(float(np.median(wall)), 2), wall_ms_per_clip=round(float(np.median(wall)) / clips, 3),
                device_ms_per_clip=round(float(st[-1]) / clips, 3),
                kernel_ms_median={k: round(float(v), 3) for k, v in zip(NAMES, st)},
                kernel_ms_per_clip={k: round(float(v) / clips, 4) for k, v in zip(NAMES, st)},
                level_out_over_in=round(rms(ys[0]) / rms(items[0]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--long-seconds", type=float, default=180.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pitch.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pitch: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    name, _ = _lib.device_info(0)
    clips = make_clips(a.clips, a.seconds, a.rate, 400)
    long_item = make_clips(1, a.long_seconds, a.rate, 440)
    res = dict(metric="fx_pitch_shift_ms", device=name, clips=a.clips, seconds=a.seconds, long_seconds=a.long_seconds,
               rate=a.rate, repeats=a.repeats, chunk_frames=_lib.fx_stretch_chunk(), cases={})
    for s in (3.0, -5.0):
        for tag, items in ((f"batch_{a.clips}", clips), ("single_clip", clips[:1]), ("long_item", long_item)):
            key = f"{tag}_s{s:+g}"
            res["cases"][key] = run(ctx, items, a.rate, s, a.repeats)
            print(f"  {key}: {res['cases'][key]}", flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
