"""Design Q's stage-aligned run count for overlapped calls (csrc/sdrfm_fm_call.h: fm_q_runs' trailing inputs) on the CPU under UBSan, driven by
tests/native/fm_runs_check.cpp: known answers worked by hand from the kernel's dealing rule, properties over a seeded sweep.  No GPU test sees this
arithmetic: design Q gives the same bits however a stream is cut into runs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fm_runs_arithmetic_clean_under_ubsan(tmp_path):
    exe = str(tmp_path / "fm_runs_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests/native/fm_runs_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
