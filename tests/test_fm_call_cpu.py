"""The FM call path's host arithmetic (csrc/sdrfm_fm_call.h: which design serves a call, the split of the machine's wave slots, segments, waves and
runs, the counts, the buffer-overlap test) on the CPU under UBSan, driven by tests/native/fm_call_check.cpp: known answers from DESIGN.md, properties
over a seeded sweep, fm_rows_overlap against byte sets.  No GPU test sees this arithmetic: every cut of a stream gives the same bits."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fm_call_arithmetic_clean_under_ubsan(tmp_path):
    exe = str(tmp_path / "fm_call_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests/native/fm_call_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
