#!/usr/bin/env python3
"""Synchronous single-clip calls against conversion tickets with two in flight, on the headline workload of bench.py (C2:
one 30 s / 16 kHz clip per request, v2 48 k, rmvpe+, full-size synthetic weights, pinned host buffers, H2D and D2H inside
the timed region).  One process alternates, ROUNDS times each, (a) a loop of N synchronous rvcx_convert_batch calls and (b)
the same N clips through rvcx_convert_submit / rvcx_convert_wait with two tickets in flight, and prints one JSON line.

(a) is the path a caller had before tickets existed and is the baseline; the in-batch figure (bench.py --workload c3) is the
ceiling.  No GPU, no result: there is no fallback.

    python tools/bench_pipelined.py [--n 20] [--rounds 5] [--distinct 4]
    RVCX_TICKET_GATE=0 python tools/bench_pipelined.py     # the HuBERT-gate A/B (one process per setting)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20, help="requests per loop (>= 20)")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two loops (>= 5)")
    ap.add_argument("--distinct", type=int, default=4, help="different clips the N requests cycle through")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pipelined: no GPU visible (there is no CPU path)")
    ctx = _lib.Context(0)
    mid = bench.load_models(ctx)
    params = bench.make_params()
    secs = bench.CLIP_SECONDS
    clips = [S.make_clip(i, secs) for i in range(a.distinct)]
    wavs = [torch.from_numpy(c).pin_memory() for c in clips]
    n = clips[0].shape[0]
    cap = ctx.out_capacity(mid, n, params)
    out_a = [torch.zeros(cap, dtype=torch.int16).pin_memory() for _ in range(a.n)]
    out_b = [torch.zeros(cap, dtype=torch.int16).pin_memory() for _ in range(a.n)]

    def sync_loop():
        return [ctx.convert_batch_raw(mid, [wavs[i % a.distinct].data_ptr()], [n], params, [out_a[i].data_ptr()])[0]
                for i in range(a.n)]

    leads = []

    def ticket_loop():
        got, pending = [], []
        for i in range(a.n):
            pending.append(ctx.convert_submit_raw(mid, [wavs[i % a.distinct].data_ptr()], [n], params, [out_b[i].data_ptr()]))
            if len(pending) == 2:
                t = pending.pop(0)
                got.append(t.wait()[0])
                leads.append(t.lead_ms)
        for t in pending:
            got.append(t.wait()[0])
            leads.append(t.lead_ms)
        return got

    for _ in range(2):                      # every shape once (and the arenas at their final size) before anything is timed
        sync_loop()
        ticket_loop()
    leads.clear()
    torch.cuda.synchronize()
    t_a, t_b = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        na = sync_loop()
        t_a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        nb = ticket_loop()
        t_b.append(time.perf_counter() - t0)
    equal = na == nb and all(torch.equal(x[:k], y[:k]) for x, y, k in zip(out_a, out_b, na)) and bool(out_a[0][:na[0]].any())
    rtf_a = [a.n * secs / t for t in t_a]
    rtf_b = [a.n * secs / t for t in t_b]

    def spread(v):
        return (max(v) - min(v)) / 2.0 / (sum(v) / len(v))

    mean_a, mean_b = sum(rtf_a) / len(rtf_a), sum(rtf_b) / len(rtf_b)
    ratio = mean_b / mean_a
    sp = max(spread(rtf_a), spread(rtf_b))
    later = [v for i, v in enumerate(leads) if i % a.n != 0]        # the first ticket of a loop enters an idle context
    print(json.dumps({
        "metric": "real_time_factor_c2_sync_vs_tickets", "n": a.n, "rounds": a.rounds, "clip_seconds": secs,
        "sync_rtf": [round(v, 1) for v in rtf_a], "ticket_rtf": [round(v, 1) for v in rtf_b],
        "sync_rtf_mean": round(mean_a, 1), "ticket_rtf_mean": round(mean_b, 1),
        "sync_ms_per_clip": round(1e3 * secs / mean_a, 3), "ticket_ms_per_clip": round(1e3 * secs / mean_b, 3),
        "spread_sync": round(spread(rtf_a), 4), "spread_tickets": round(spread(rtf_b), 4),
        "ratio": round(ratio, 4), "beats_twice_the_spread": bool(ratio - 1.0 > 2.0 * sp),
        "ticket_lead_ms_mean": round(float(np.mean(later)), 3), "ticket_lead_ms_min": round(float(np.min(later)), 3),
        "fast_path": {"fp32_layers": ctx.fp32_layers(), "fp32_reruns": ctx.fp32_reruns(), "gru_fallbacks": ctx.gru_fallbacks()},
        "outputs_byte_equal": bool(equal),
        "ticket_gate": os.environ.get("RVCX_TICKET_GATE", "default"),
    }))
    ctx.close()


if __name__ == "__main__":
    main()
