"""The FM handle's carried state and overlap joins (csrc/sdrfm_fm_carry.h: whether a call may overlap and which term refuses it, when y[-1] is recomputed and
hist_q refilled, the slots, what each of the three joins records and waits for, what a reset keeps) on the CPU under UBSan, driven by
tests/native/fm_carry_check.cpp in enqueue()'s order against two emulated internal streams: known answers (every sequence of fm_shape_cases.overlap_cases(),
each row collision alone, the joins on a six-call script), properties over a seeded sweep of call sequences with joins, assignments and resets in between."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fm_carry_bookkeeping_clean_under_ubsan(tmp_path):
    exe = str(tmp_path / "fm_carry_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests/native/fm_carry_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
