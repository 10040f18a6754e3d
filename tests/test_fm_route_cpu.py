"""The FM handle's per-stream routing (csrc/sdrfm_fm_route.h: windows, counter sets, the threshold, the back-off, the stream list, which event a kernel
carries and what a window's close records and waits for) on the CPU under UBSan, driven by tests/native/fm_route_check.cpp against an emulated device whose
read-backs arrive when the test says: known answers (the fixed calls tests/test_route_gpu.py holds on hardware), properties over a seeded sweep of call
sequences with resets and masks at any point."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fm_route_bookkeeping_clean_under_ubsan(tmp_path):
    exe = str(tmp_path / "fm_route_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests/native/fm_route_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
