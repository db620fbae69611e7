"""bench.py's plain run and --dump-outputs: the PCM of the last timed step as float32 .npy files within 64 MB, and a
plain run that carries only the headline (children, sustained loop, roofline and CPU baseline are --full's)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_arrays_whole_when_they_fit_and_a_seeded_sample_when_not():
    B = _bench_module()
    g = np.random.Generator(np.random.PCG64(0))
    pcms = [g.integers(-32768, 32768, n, dtype=np.int16) for n in (1000, 2500, 40)]
    whole = B.dump_arrays(pcms, [0, 1, 2])
    assert set(whole) == {"pcm_lengths", "pcm_000", "pcm_001", "pcm_002"}
    assert whole["pcm_lengths"].tolist() == [1000, 2500, 40]
    for i, p in enumerate(pcms):
        a = whole[f"pcm_{i:03d}"]
        assert a.dtype == np.float32 and np.array_equal(a, p.astype(np.float32))

    budget = 8 << 10
    s1, s2 = B.dump_arrays(pcms, [5, 7, 9], budget), B.dump_arrays(pcms, [5, 7, 9], budget)
    assert sum(a.nbytes + 128 for a in s1.values()) <= budget
    for i, p in zip((5, 7, 9), pcms):
        at = s1[f"pcm_{i:03d}_at"]
        assert at.dtype == np.float64 and np.all(np.diff(at) > 0) and 0 < at.size < p.size
        assert np.array_equal(s1[f"pcm_{i:03d}"], p[at.astype(np.int64)].astype(np.float32))
        assert np.array_equal(at, s2[f"pcm_{i:03d}_at"])            # the same positions on every run


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_times_the_steps_asked_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert d[k]
    # what --full adds stays out of a plain run
    assert d["roofline"] is None and d["sustained"] is None and d["cpu_baseline"] is None
    assert not any(k in d for k in ("exact_fp32", "c3", "c5", "long_clip", "full_decoder"))
    files = sorted(os.listdir(out))
    assert files == ["pcm_000.npy", "pcm_lengths.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    pcm = np.load(out / "pcm_000.npy")
    assert pcm.dtype == np.float32 and pcm.shape == (d["config"]["out_samples"],)
    assert np.load(out / "pcm_lengths.npy").tolist() == [pcm.shape[0]]
    assert np.array_equal(pcm, np.round(pcm)) and np.abs(pcm).max() <= 32768 and np.any(pcm != 0)
