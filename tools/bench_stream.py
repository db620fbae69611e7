#!/usr/bin/env python3
"""Step times of live-stream sessions (rvcx_stream_step): full-size 48 k voice model, HuBERT-base, RMVPE, synthetic weights;
block 100 ms, context 2.5 s, cross-fade 50 ms, search 10 ms; S lock-step streams.  For every S: `--warmup` steps, then
`--repeats` runs of `--steps` timed steps (wall clock around the whole call: host blocks in, host blocks out), median and
p99 per run, and the per-stage device times of rvcx_last_timing.  Then the same step with the synthesizer run whole
(RVCX_STREAM_FULL_SYNTH=1: skip_head = 0, SOLA on the tail of the output): what the tail-only path saves.

The one criterion that can be derived is real time itself: a step must take less than the block it converts.  The result
records, per S, whether the median and the p99 do, and the largest S whose p99 does.  Not part of bench.py.

    python tools/bench_stream.py [--streams 1,4,16,32] [--steps 200] [--warmup 20] [--repeats 3] [--out profiles/bench_stream.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from polgen_rvc_amd import _lib, synthetic as S  # noqa: E402

BLOCK_MS, CONTEXT_MS, CROSSFADE_MS, SEARCH_MS = 100, 2500, 50, 10
STAGES = ["f0", "hubert", "blend_mix", "enc_p", "flow", "decoder", "sola_copies", "total"]


def run(ctx, mid, n_streams, steps, warmup, repeats, full_synth):
    os.environ["RVCX_STREAM_FULL_SYNTH"] = "1" if full_synth else "0"      # read when the session opens
    p = bench.make_params(seed=1)
    Fb, Fc, Fx, Fs = BLOCK_MS // 10, CONTEXT_MS // 10, CROSSFADE_MS // 10, SEARCH_MS // 10
    need = (warmup + steps) * Fb * 160
    clips = np.stack([S.make_clip(100 + s, need / 16000.0 + 0.1)[:need] for s in range(n_streams)]).astype(np.float32)
    runs, stage_ms = [], []
    with ctx.stream_open(mid, p, [0] * n_streams, [float(s % 5 - 2) for s in range(n_streams)], Fb, Fc, Fx, Fs) as se:
        geo = dict(ring_frames=Fc + Fx + Fs + Fb, frames=se.frames, skip_head=se.skip_head, block_out=se.block_out)
        for r in range(repeats):
            se.reset()
            ms = []
            for k in range(warmup + steps):
                blk = np.ascontiguousarray(clips[:, k * Fb * 160:(k + 1) * Fb * 160])
                t0 = time.perf_counter()
                out = se.step(blk)
                dt = time.perf_counter() - t0
                if k >= warmup:
                    ms.append(1e3 * dt)
                    tm = ctx.last_timing()
                    stage_ms.append([tm[n] for n in ("rmvpe", "hubert", "index", "enc_p", "flow", "decoder", "post", "total")])
            assert np.isfinite(out).all() and out.any()
            ms = np.asarray(ms)
            runs.append(dict(median_ms=round(float(np.median(ms)), 3), p99_ms=round(float(np.percentile(ms, 99)), 3),
                             max_ms=round(float(ms.max()), 3)))
            print(f"  S={n_streams} full_synth={int(full_synth)} run {r}: {runs[-1]}", flush=True)
    st = np.median(np.asarray(stage_ms), axis=0)
    return dict(geometry=geo, runs=runs, median_ms=round(float(np.median([r["median_ms"] for r in runs])), 3),
                p99_ms=round(float(np.max([r["p99_ms"] for r in runs])), 3),
                stage_ms_median={n: round(float(v), 3) for n, v in zip(STAGES, st)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=60, help="timed steps of the skip_head = 0 comparison (one run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_stream.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stream: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    mid = bench.load_models(ctx)
    name, _ = _lib.device_info(0)
    res = dict(metric="stream_step_ms", device=name, block_ms=BLOCK_MS, context_ms=CONTEXT_MS, crossfade_ms=CROSSFADE_MS,
               search_ms=SEARCH_MS, steps=a.steps, warmup=a.warmup, repeats=a.repeats, streams={})
    for n_streams in [int(v) for v in a.streams.split(",")]:
        r = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False)
        full = run(ctx, mid, n_streams, a.ab_steps, a.warmup, 1, True)
        r["real_time_median"] = bool(r["median_ms"] < BLOCK_MS)
        r["real_time_p99"] = bool(r["p99_ms"] < BLOCK_MS)
        r["skip_head_0"] = dict(median_ms=full["median_ms"], p99_ms=full["p99_ms"], stage_ms_median=full["stage_ms_median"])
        r["tail_only_saves_ms"] = round(full["median_ms"] - r["median_ms"], 3)
        res["streams"][str(n_streams)] = r
    ok = [int(k) for k, v in res["streams"].items() if v["real_time_p99"]]
    res["largest_streams_real_time_p99"] = max(ok) if ok else 0
    res["fast_path"] = {"fp32_layers": ctx.fp32_layers(), "fp32_reruns": ctx.fp32_reruns(), "gru_fallbacks": ctx.gru_fallbacks()}
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
