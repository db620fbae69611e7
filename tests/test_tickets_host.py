"""CPU: conversion tickets on the host-side sanitizer builds.  tools/host_tickets.sh builds the HOST pass of every csrc/*.hip
against tools/hipstub (the HIP runtime on host memory, kernel launches are no-ops) and runs tools/host_tickets_driver.py on
it: submit / wait / poll from four threads sharing one context for a few hundred tickets, the third-submit rule, interleaved
loads and unloads, every misuse path, destroy with tickets in flight, out_n / last_cuts / last_micro_batches of each ticket
against the synchronous call's -- once under AddressSanitizer + UBSan (make host-asan) and once under ThreadSanitizer (make
host-tsan; tools/tsan.supp silences reports that lie entirely inside the interpreter).  CPU container only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(mode):
    if not (os.path.exists(CLANG) and shutil.which("hipcc") and shutil.which("make")):
        pytest.skip("no ROCm clang / hipcc / make here")
    rt = subprocess.run([CLANG, f"-print-file-name=libclang_rt.{mode}-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.exists(rt):
        pytest.skip(f"no shared {mode} runtime: this half is not run")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_tickets.sh"), mode], capture_output=True, text=True,
                       timeout=1800, cwd=ROOT)
    tail = r.stdout[-2000:] + "\n" + r.stderr[-6000:]
    assert r.returncode == 0 and "HOST_TICKETS_OK" in r.stdout, tail
    return r, tail


def test_tickets_host_code_is_clean_under_asan_and_ubsan():
    r, tail = _run("asan")
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail


def test_tickets_host_code_is_clean_under_tsan():
    r, tail = _run("tsan")
    assert "WARNING: ThreadSanitizer" not in r.stderr, tail
