#!/usr/bin/env python3
"""Times of loudness metering (rvcx_fx_loudness) and of the loudness-matched master (rvcx_fx_master): 1 clip and `--clips`
stereo clips of `--seconds` s at `--rate` Hz (default 64 x 30 s at 48 kHz), each in ONE call; the master at -16 LUFS (the
limiter has nothing to do on these clips) and once more at -6 LUFS, where it works on every item.  One process; per case one
warm-up call, then `--repeats` timed calls: wall clock around the whole call (host arrays in, host arrays out) and the
per-stage device times of rvcx_last_timing, medians over the repeats.  Beside every stage stands the number of passes it
makes over the signal (reads + writes of a float32 sample of one channel, counted from the kernels) and the bytes per second
that count amounts to at the measured time.  Not part of bench.py; no bar is fixed in advance (LABNOTES 21 sets the metering
time per clip beside the effects chain's).

    python tools/bench_loudness.py [--clips 64] [--seconds 30] [--rate 48000] [--repeats 3] [--out profiles/bench_loudness.json]"""
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

# float32 passes over one channel's samples per stage (a read or a write of every sample counts one; the per-item gain rows
# p, u, e, s count one half each on stereo; the limiter gain at one relaxation pass of its follower).
METER_PASSES = {"copies_in": 3.0, "chunk_states": 1.0, "carry": 0.0, "kweight_energy": 1.0, "gates": 0.0, "true_peak": 1.0}
MASTER_PASSES = {"stem_loudness": 4.0, "mix": 3.0, "mix_loudness": 2.0, "scale_true_peak": 3.5, "limiter_gain": 3.0,
                 "gain_int16": 3.0, "result_meters": 3.0}


def make_clips(clips, seconds, rate, seed, scale):
    n = int(round(seconds * rate))
    base = []
    for k in range(min(clips, 4)):
        a = S.make_clip(seed + k, seconds + 0.1)
        idx = (np.arange(n, dtype=np.int64) * 16000) // rate
        x = np.stack([a[idx], np.roll(a, 1234)[idx]], axis=1).astype(np.float32)
        base.append(np.ascontiguousarray(x * (scale / np.abs(x).max())))
    return [base[i % len(base)] for i in range(clips)]


def summarise(wall, stages, names, passes, samples, clips):
    st = np.median(np.asarray(stages), axis=0)
    res = dict(wall_ms_runs=[round(v, 2) for v in wall], wall_ms_median=round(float(np.median(wall)), 2),
               wall_ms_per_clip=round(float(np.median(wall)) / clips, 3), device_ms_per_clip=round(float(st[-1]) / clips, 3),
               stage_ms_median={k: round(float(v), 3) for k, v in zip(names, st)}, stages={})
    for k, v in zip(names, st):
        if k in passes:
            gb = passes[k] * samples * 4 / 1e9
            res["stages"][k] = dict(ms=round(float(v), 3), passes=passes[k], gbytes=round(gb, 3),
                                    gbytes_per_s=round(gb / (float(v) * 1e-3), 1) if v > 0 and gb > 0 else None)
    return res


def run_meter(ctx, items, rate, repeats):
    ctx.fx_loudness(items, rate)                               # warm-up: the arena grows here
    names = ["copies_in", "chunk_states", "carry", "kweight_energy", "gates", "true_peak", "copies_out", "unused", "total"]
    wall, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = ctx.fx_loudness(items, rate)
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_loudness_timing()
        stages.append([tm[k] for k in names])
    res = summarise(wall, stages, names, METER_PASSES, sum(x.size for x in items), len(items))
    res["first_item"] = dict(lufs=round(got[0][0], 3), dbtp=round(got[0][1], 3))
    return res


def run_master(ctx, vocals, insts, rate, repeats, target=-16.0):
    ctx.fx_master(vocals, insts, rate, target, 0.0, -1.0)
    names = ["stem_loudness", "mix", "mix_loudness", "scale_true_peak", "limiter_gain", "gain_int16", "result_meters", "copies",
             "total"]
    wall, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, reps = ctx.fx_master(vocals, insts, rate, target, 0.0, -1.0)
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_master_timing()
        stages.append([tm[k] for k in names])
    res = summarise(wall, stages, names, MASTER_PASSES, sum(x.size for x in vocals), len(vocals))
    res["target_lufs"] = target
    res["limited_items"] = sum(r["min_gain"] < 1.0 for r in reps)
    res["follower_passes"] = ctx.fx_last_passes()[0][0] if res["limited_items"] else 0
    res["first_item"] = {k: round(v, 3) for k, v in reps[0].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_loudness.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loudness: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    name, _ = _lib.device_info(0)
    vocals = make_clips(a.clips, a.seconds, a.rate, 300, 0.5)
    insts = make_clips(a.clips, a.seconds, a.rate, 340, 0.2)
    res = dict(metric="fx_loudness_ms", device=name, clips=a.clips, seconds=a.seconds, rate=a.rate, repeats=a.repeats,
               chunk=_lib.fx_chunk(), cases={})
    for B in sorted({1, a.clips}):
        res["cases"][f"meter_{B}"] = run_meter(ctx, vocals[:B], a.rate, a.repeats)
        print(f"  meter_{B}: {res['cases'][f'meter_{B}']}", flush=True)
        res["cases"][f"master_{B}"] = run_master(ctx, vocals[:B], insts[:B], a.rate, a.repeats)
        print(f"  master_{B}: {res['cases'][f'master_{B}']}", flush=True)
    # a target the peaks do not fit under: the limiter works on every item
    res["cases"][f"master_{a.clips}_limited"] = run_master(ctx, vocals, insts, a.rate, a.repeats, target=-6.0)
    print(f"  master_{a.clips}_limited: {res['cases'][f'master_{a.clips}_limited']}", flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
