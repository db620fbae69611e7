#!/usr/bin/env python3
"""Step times of live-stream sessions (rvcx_stream_step): full-size 48 k voice model, HuBERT-base, RMVPE, synthetic weights;
block 100 ms, context 2.5 s, cross-fade 50 ms, search 10 ms; S lock-step streams.  For every S: `--warmup` steps, then
`--repeats` runs of `--steps` timed steps (wall clock around the whole call: host blocks in, host blocks out), median and
p99 per run, and the per-stage device times of rvcx_last_timing.  Then the same step with the synthesizer run whole
(RVCX_STREAM_FULL_SYNTH=1: skip_head = 0, SOLA on the tail of the output): what the tail-only path saves.

With `--in-rate` / `--in-channels` / `--out-rate` every S is measured a second time as a rate session (rvcx_stream_open_io:
the blocks arrive at the sound card's rate and leave at `--out-rate`), on the same model and the same audio, so the step with
and without the two resamplers stands side by side; the result gains the delays and the difference.  `--model 40k` measures
on the 40 k voice model (48 kHz out of it is a real conversion; out of the 48 k model it is none).  A rate session is then
measured a third and fourth time with the effects board inside the step (rvcx_stream_open_fx): at the processing tab's defaults,
and with the chorus and both shelves on; the result gains the board's cost beside the rate session without it and the per-stage
device times of rvcx_stream_last_fx_ms.  `--no-effects` leaves these out.

With `--denoise` every S is measured three more times with live noise reduction (rvcx_stream_open_dn, stage 16 at its
defaults) on the input side, on the output side and on both, next to the plain session of the same run: step time with and
without each side, and the sides' own device times (rvcx_stream_last_dn_ms).  The plain session is launch for launch what a
session without noise reduction always was, so it is the comparison.  Write that run to profiles/bench_stream_denoise.json
(`--out`).

With `--formant` every S is measured three more times with the live formant shift (rvcx_stream_open_fm, stage 19 at its
defaults, +4 semitones) on the input side, on the output side and on both, next to the plain session of the same run: step time
with and without each side, and the sides' own device times (rvcx_stream_last_fm_ms).  No bar is set on these times.  Write that
run to profiles/bench_stream_formant.json (`--out`).

The one criterion that can be derived is real time itself: a step must take less than the block it converts.  The result
records, per S, whether the median and the p99 do, and the largest S whose p99 does.  Not part of bench.py.

    python tools/bench_stream.py [--streams 1,4,16,32] [--steps 200] [--warmup 20] [--repeats 3] [--model 48k|40k]
                                 [--in-rate 48000 --in-channels 2 --out-rate 48000] [--out profiles/bench_stream.json]
    python tools/bench_stream.py --denoise --ab-steps 0 --out profiles/bench_stream_denoise.json
    python tools/bench_stream.py --formant --ab-steps 0 --out profiles/bench_stream_formant.json"""
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
FX_CASES = {"ui_defaults": {},
            "chorus_and_shelves": dict(low_shelf_gain=3.0, high_shelf_gain=-2.0, chorus_rate_hz=1.5, chorus_depth=0.25,
                                       chorus_centre_delay_ms=7.0, chorus_feedback=0.3, chorus_mix=0.5)}


def mic_blocks(clips, in_rate, in_channels):
    """the 16 kHz clips as a sound card would deliver them: (S, frames at in_rate[, channels]); sample-and-hold is enough for a
    timing run (the step does not depend on the values)"""
    if in_rate in (0, 16000) and in_channels == 1:
        return clips
    rate = in_rate or 16000
    idx = (np.arange(clips.shape[1] * rate // 16000) * 16000) // rate
    x = clips[:, idx]
    return x if in_channels == 1 else np.ascontiguousarray(np.repeat(x[:, :, None], in_channels, axis=2))


DN_CASES = {"in": dict(denoise_in={}), "out": dict(denoise_out={}), "both": dict(denoise_in={}, denoise_out={})}


FM = dict(semitones=4.0)
FM_CASES = {"in": dict(formant_in=FM), "out": dict(formant_out=FM), "both": dict(formant_in=FM, formant_out=FM)}


def run(ctx, mid, n_streams, steps, warmup, repeats, full_synth, io=None, effects=None, denoise=None, formant=None):
    os.environ["RVCX_STREAM_FULL_SYNTH"] = "1" if full_synth else "0"      # read when the session opens
    p = bench.make_params(seed=1)
    io = io or {}
    Fb, Fc, Fx, Fs = BLOCK_MS // 10, CONTEXT_MS // 10, CROSSFADE_MS // 10, SEARCH_MS // 10
    need = (warmup + steps) * Fb * 160
    clips = np.stack([S.make_clip(100 + s, need / 16000.0 + 0.1)[:need] for s in range(n_streams)]).astype(np.float32)
    clips = mic_blocks(clips, io.get("in_rate", 0), io.get("in_channels", 1))
    runs, stage_ms, fx_ms, dn_ms, fm_ms = [], [], [], [], []
    with ctx.stream_open(mid, p, [0] * n_streams, [float(s % 5 - 2) for s in range(n_streams)], Fb, Fc, Fx, Fs, effects=effects,
                         **io, **(denoise or {}), **(formant or {})) as se:
        geo = dict(ring_frames=Fc + Fx + Fs + Fb, frames=se.frames, skip_head=se.skip_head, block_in=se.block_in,
                   block_out=se.block_out, in_delay=se.in_delay, out_delay=se.out_delay, latency_ms=round(se.latency_ms, 3))
        for r in range(repeats):
            se.reset()
            ms = []
            for k in range(warmup + steps):
                blk = np.ascontiguousarray(clips[:, k * se.block_in:(k + 1) * se.block_in])
                t0 = time.perf_counter()
                out = se.step(blk)
                dt = time.perf_counter() - t0
                if k >= warmup:
                    ms.append(1e3 * dt)
                    tm = ctx.last_timing()
                    stage_ms.append([tm[n] for n in ("rmvpe", "hubert", "index", "enc_p", "flow", "decoder", "post", "total")])
                    if effects is not None:
                        fx_ms.append(list(se.last_fx_ms().values()))
                    if denoise:
                        dn_ms.append(se.last_dn_ms())
                    if formant:
                        fm_ms.append(se.last_fm_ms())
            assert np.isfinite(out).all() and out.any()
            ms = np.asarray(ms)
            runs.append(dict(median_ms=round(float(np.median(ms)), 3), p99_ms=round(float(np.percentile(ms, 99)), 3),
                             max_ms=round(float(ms.max()), 3)))
            print(f"  S={n_streams} full_synth={int(full_synth)} io={io} effects={effects is not None} "
                  f"denoise={sorted(denoise or {})} formant={sorted(formant or {})} run {r}: {runs[-1]}", flush=True)
    st = np.median(np.asarray(stage_ms), axis=0)
    res = dict(geometry=geo, runs=runs, median_ms=round(float(np.median([r["median_ms"] for r in runs])), 3),
               p99_ms=round(float(np.max([r["p99_ms"] for r in runs])), 3),
               stage_ms_median={n: round(float(v), 3) for n, v in zip(STAGES, st)})
    if effects is not None:
        names = ["highpass", "compressor", "gate", "reverb", "low_shelf", "high_shelf", "chorus", "total"]
        res["fx_ms_median"] = {n: round(float(v), 4) for n, v in zip(names, np.median(np.asarray(fx_ms), axis=0))}
    if denoise:
        res["dn_ms_median"] = {n: round(float(v), 4) for n, v in zip(("in", "out"), np.median(np.asarray(dn_ms), axis=0))}
    if formant:
        res["fm_ms_median"] = {n: round(float(v), 4) for n, v in zip(("in", "out"), np.median(np.asarray(fm_ms), axis=0))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16,32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=60, help="timed steps of the skip_head = 0 comparison (one run)")
    ap.add_argument("--model", default="48k", choices=["48k", "40k"], help="the voice model the sessions run on")
    ap.add_argument("--in-rate", type=int, default=0, help="Hz of the blocks a rate session takes (0: 16 kHz)")
    ap.add_argument("--in-channels", type=int, default=1)
    ap.add_argument("--out-rate", type=int, default=0, help="Hz of the blocks a rate session returns (0: the model's rate)")
    ap.add_argument("--no-effects", action="store_true", help="skip the rate session with the effects board inside the step")
    ap.add_argument("--denoise", action="store_true", help="also measure sessions with live noise reduction on either side")
    ap.add_argument("--formant", action="store_true", help="also measure sessions with the live formant shift on either side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_stream.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stream: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    mid = bench.load_models(ctx, also_40k=True)[1] if a.model == "40k" else bench.load_models(ctx)
    name, _ = _lib.device_info(0)
    io = dict(in_rate=a.in_rate, in_channels=a.in_channels, out_rate=a.out_rate)
    rates = io != dict(in_rate=0, in_channels=1, out_rate=0)
    res = dict(metric="stream_step_ms", device=name, model=a.model, block_ms=BLOCK_MS, context_ms=CONTEXT_MS,
               crossfade_ms=CROSSFADE_MS, search_ms=SEARCH_MS, steps=a.steps, warmup=a.warmup, repeats=a.repeats, streams={})
    if rates:
        res["io"] = io
    for n_streams in [int(v) for v in a.streams.split(",")]:
        r = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False)
        if a.ab_steps > 0:
            full = run(ctx, mid, n_streams, a.ab_steps, a.warmup, 1, True)
            r["skip_head_0"] = dict(median_ms=full["median_ms"], p99_ms=full["p99_ms"], stage_ms_median=full["stage_ms_median"])
            r["tail_only_saves_ms"] = round(full["median_ms"] - r["median_ms"], 3)
        r["real_time_median"] = bool(r["median_ms"] < BLOCK_MS)
        r["real_time_p99"] = bool(r["p99_ms"] < BLOCK_MS)
        if rates:     # the same S, model and audio through the two resamplers: the step with and without, side by side
            q = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False, io)
            r["rates"] = dict(geometry=q["geometry"], runs=q["runs"], median_ms=q["median_ms"], p99_ms=q["p99_ms"],
                              stage_ms_median=q["stage_ms_median"], real_time_p99=bool(q["p99_ms"] < BLOCK_MS),
                              resampling_costs_ms=round(q["median_ms"] - r["median_ms"], 3),
                              resampling_costs_device_ms=round(q["stage_ms_median"]["total"] - r["stage_ms_median"]["total"], 3))
            if not a.no_effects:      # and with the board behind the output resampler, in the same process
                r["effects"] = {}
                for name, fx in FX_CASES.items():
                    e = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False, io, effects=fx)
                    r["effects"][name] = dict(values=fx, runs=e["runs"], median_ms=e["median_ms"], p99_ms=e["p99_ms"],
                                              stage_ms_median=e["stage_ms_median"], fx_ms_median=e["fx_ms_median"],
                                              real_time_p99=bool(e["p99_ms"] < BLOCK_MS),
                                              board_costs_ms=round(e["median_ms"] - q["median_ms"], 3),
                                              board_costs_device_ms=round(e["stage_ms_median"]["total"]
                                                                          - q["stage_ms_median"]["total"], 3))
        if a.denoise:     # the same S, model, audio and rates with stage 16 on the input side, the output side and both
            base = r["rates"] if rates else r
            r["denoise"] = {}
            for name, dn in DN_CASES.items():
                e = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False, io if rates else None, denoise=dn)
                r["denoise"][name] = dict(geometry=e["geometry"], runs=e["runs"], median_ms=e["median_ms"], p99_ms=e["p99_ms"],
                                          stage_ms_median=e["stage_ms_median"], dn_ms_median=e["dn_ms_median"],
                                          real_time_p99=bool(e["p99_ms"] < BLOCK_MS),
                                          plain_median_ms=base["median_ms"],
                                          denoise_costs_ms=round(e["median_ms"] - base["median_ms"], 3),
                                          denoise_costs_device_ms=round(e["stage_ms_median"]["total"]
                                                                        - base["stage_ms_median"]["total"], 3))
        if a.formant:     # the same S, model, audio and rates with stage 19 on the input side, the output side and both
            base = r["rates"] if rates else r
            r["formant"] = {}
            for name, fm in FM_CASES.items():
                e = run(ctx, mid, n_streams, a.steps, a.warmup, a.repeats, False, io if rates else None, formant=fm)
                r["formant"][name] = dict(geometry=e["geometry"], runs=e["runs"], median_ms=e["median_ms"], p99_ms=e["p99_ms"],
                                          stage_ms_median=e["stage_ms_median"], fm_ms_median=e["fm_ms_median"],
                                          real_time_p99=bool(e["p99_ms"] < BLOCK_MS),
                                          plain_median_ms=base["median_ms"],
                                          formant_costs_ms=round(e["median_ms"] - base["median_ms"], 3),
                                          formant_costs_device_ms=round(e["stage_ms_median"]["total"]
                                                                        - base["stage_ms_median"]["total"], 3))
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
