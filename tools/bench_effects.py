#!/usr/bin/env python3
"""Times of the post-production chain (rvcx_fx_chain): `--clips` stereo clips of `--seconds` s at `--rate` Hz (default: the
C3-sized job, 64 x 30 s at 48 kHz) in ONE call, under two settings: the processing tab's defaults (chorus off, shelves flat)
and the same with the chorus on.  One process; per setting one warm-up call, then `--repeats` timed calls: wall clock around
the whole call (host arrays in, host arrays out), the per-stage device times of rvcx_last_timing and the relaxation passes
the envelope followers took.  Medians over the repeats.  Not part of bench.py; no bar is fixed in advance (LABNOTES 17 sets
the per-clip time beside C3's per-clip conversion time).

    python tools/bench_effects.py [--clips 64] [--seconds 30] [--rate 48000] [--repeats 3] [--out profiles/bench_effects.json]"""
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

CHORUS_ON = dict(chorus_rate_hz=1.5, chorus_depth=0.25, chorus_centre_delay_ms=7.0, chorus_feedback=0.3, chorus_mix=0.5)
STAGES = ["highpass", "compressor", "gate", "reverb", "low_shelf", "high_shelf", "chorus", "copies", "total"]


def make_clips(clips, seconds, rate):
    """stereo voices at +-0.5: a few distinct 16 kHz recipes held to the rate (the times do not depend on the values, the
    followers' pass counts do -- so real envelopes, not noise)"""
    n = int(round(seconds * rate))
    base = []
    for k in range(min(clips, 4)):
        a = S.make_clip(300 + k, seconds + 0.1)
        idx = (np.arange(n, dtype=np.int64) * 16000) // rate
        x = np.stack([a[idx], np.roll(a, 1234)[idx]], axis=1).astype(np.float32)
        base.append(np.ascontiguousarray(x * (0.5 / np.abs(x).max())))
    return [base[i % len(base)] for i in range(clips)]


def run(ctx, items, rate, values, repeats):
    p = _lib.FxParams.make(values, rate, 2)
    ctx.fx_chain(items, p)                                    # warm-up: the arena grows here
    wall, stage, passes = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = ctx.fx_chain(items, p)
        wall.append(1e3 * (time.perf_counter() - t0))
        tm = ctx.fx_last_timing()
        stage.append([tm[k] for k in STAGES])
        ps, groups = ctx.fx_last_passes()
        passes.append(ps)
    assert all(np.isfinite(y).all() for y in out[:2]) and out[0].any()
    st = np.median(np.asarray(stage), axis=0)
    res = dict(wall_ms_runs=[round(v, 2) for v in wall], wall_ms_median=round(float(np.median(wall)), 2),
               wall_ms_per_clip=round(float(np.median(wall)) / len(items), 3),
               device_ms_per_clip=round(float(st[-1]) / len(items), 3),
               stage_ms_median={k: round(float(v), 3) for k, v in zip(STAGES, st)},
               follower_passes=dict(zip(["compressor", "gate_square", "gate_peak"], np.max(np.asarray(passes), axis=0).tolist())),
               groups=groups)
    res["dominant_stage"] = max(STAGES[:-1], key=lambda k: res["stage_ms_median"][k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_effects.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_effects: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    name, _ = _lib.device_info(0)
    items = make_clips(a.clips, a.seconds, a.rate)
    res = dict(metric="fx_chain_ms", device=name, clips=a.clips, seconds=a.seconds, rate=a.rate, repeats=a.repeats,
               chunk=_lib.fx_chunk(), settings={})
    for label, extra in (("ui_defaults", {}), ("chorus_on", CHORUS_ON)):
        values = dict(_lib.FX_UI_DEFAULTS)
        values.update(extra)
        res["settings"][label] = run(ctx, items, a.rate, values, a.repeats)
        print(f"  {label}: {res['settings'][label]}", flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
