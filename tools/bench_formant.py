#!/usr/bin/env python3
"""Times of the formant shift (rvcx_fx_formant, include/rvcx.h stage 17) and of the formant-preserving pitch shift
(rvcx_fx_pitch_shift_formant, stage 18): `--clips` stereo clips of `--seconds` s at `--rate` Hz in ONE call (default 64 x 30 s
at 48 kHz) and one stereo clip; stage 17 alone at +4 semitones, stage 17 with a source per item (the transfer stage 18 runs),
stage 18 at +3 semitones, and stage 14 alone beside it.  One process; per case one warm-up call, then `--repeats` timed calls:
wall clock around the whole call (host arrays in, host arrays out) and the device times of rvcx_last_timing, medians over the
repeats.  The frames kernel does 2 (iterations + 1) + 2 transforms of N points per frame (one more with a source); its rate is
given as transforms per second.  Not part of bench.py; no bar is fixed in advance (LABNOTES 25).

    python tools/bench_formant.py [--clips 64] [--seconds 30] [--rate 48000] [--repeats 3] [--out profiles/bench_formant.json]"""
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

NAMES = ["copies_in", "frames", "overlap_add", "copies_out", "pitch_shift", "total"]


def make_clips(clips, seconds, rate, seed, scale=0.5):
    n = int(round(seconds * rate))
    base = []
    for k in range(min(clips, 4)):
        a = S.make_clip(seed + k, min(seconds, 30.0) + 0.1)
        idx = ((np.arange(n, dtype=np.int64) * 16000) // rate) % a.shape[0]
        x = np.stack([a[idx], np.roll(a, 1234)[idx]], axis=1).astype(np.float32)
        base.append(np.ascontiguousarray(x * (scale / np.abs(x).max())))
    return [base[i % len(base)] for i in range(clips)]


def run(ctx, call, items, rate, repeats, transforms_per_frame):
    call()                                                           # warm-up: the arena grows here
    wall, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ys = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_formant_timing() if transforms_per_frame else dict(ctx.fx_stretch_timing(), frames=0.0, pitch_shift=0.0)
        stages.append([tm.get(k, 0.0) for k in NAMES])
    st = dict(zip(NAMES, np.median(np.asarray(stages), axis=0)))
    clips, n, ch = len(items), items[0].shape[0], items[0].shape[1]
    T, N, nc = _lib.fx_formant_frames(n, rate)
    frames = clips * ch * T
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))      # noqa: E731
    out = dict(clips=clips, channels=ch, frames_per_row=T, N=N, nc=nc, groups=ctx.fx_last_passes()[1],
               wall_ms_runs=[round(v, 2) for v in wall], wall_ms_median=round(float(np.median(wall)), 2),
               wall_ms_per_clip=round(float(np.median(wall)) / clips, 3), device_ms_per_clip=round(float(st["total"]) / clips, 3),
               device_ms_median={k: round(float(v), 3) for k, v in st.items()},
               level_out_over_in=round(rms(ys[0]) / rms(items[0]), 4))
    if transforms_per_frame and st["frames"] > 0:
        out.update(transforms_per_frame=transforms_per_frame,
                   transforms_per_s=round(frames * transforms_per_frame / (float(st["frames"]) * 1e-3), 0),
                   frames_kernel_us_per_frame=round(1e3 * float(st["frames"]) / frames, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_formant.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_formant: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    name, _ = _lib.device_info(0)
    clips = make_clips(a.clips, a.seconds, a.rate, 400)
    others = make_clips(a.clips, a.seconds, a.rate, 500)
    p = _lib.FxFormantParams.make(a.rate, 2, semitones=4.0)
    p1 = _lib.FxFormantParams.make(a.rate, 2)
    lifts = 2 * (p.iterations + 1)
    res = dict(metric="fx_formant_ms", device=name, clips=a.clips, seconds=a.seconds, rate=a.rate, repeats=a.repeats,
               iterations=p.iterations, cases={})
    for tag, items, srcs in ((f"batch_{a.clips}", clips, others), ("single_stereo", clips[:1], others[:1])):
        cases = (("stage17_shift", lambda: ctx.fx_formant(items, a.rate, p), lifts + 2),
                 ("stage17_transfer", lambda: ctx.fx_formant(items, a.rate, p1, source=srcs), lifts + 3),
                 ("stage18", lambda: ctx.fx_pitch_shift(items, a.rate, 3.0, preserve_formants=True), lifts + 3),
                 ("stage14_alone", lambda: ctx.fx_pitch_shift(items, a.rate, 3.0), 0))
        for what, call, per_frame in cases:
            key = f"{tag}_{what}"
            res["cases"][key] = run(ctx, call, items, a.rate, a.repeats, per_frame)
            print(f"  {key}: {res['cases'][key]}", flush=True)
    ctx.close()
    mono = np.ascontiguousarray(clips[0][:, 0])                     # the host twin on one mono clip
    t0 = time.perf_counter()
    _lib.fx_formant_host(mono, a.rate, _lib.FxFormantParams.make(a.rate, 1, semitones=4.0))
    res["cases"]["host_twin_mono_stage17_shift"] = dict(wall_ms=round(1e3 * (time.perf_counter() - t0), 1))
    print(f"  host twin: {res['cases']['host_twin_mono_stage17_shift']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
