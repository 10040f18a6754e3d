"""The blend and gain ramps of csrc/sdrfm_audio_ctl.h on the CPU: tests/native/audio_ctl_check.cpp, a program of its own
built with ASan and UBSan, holds the header's closed form to the one-output-at-a-time iteration, to its own composition and to the
saturated count; then tests/audio_ref.py, the Python reference the GPU tests use, is held to the same iteration."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import audio_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLEWS = (1, 2, 3, 7, 40, 32767, 32768)
VALUES = (0, 1, 2, 6, 7, 8, 16383, 32767, 32768)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ramp_header_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "audio_ctl_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests/native/audio_ctl_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


def test_python_reference_ramp_is_the_iteration():
    for slew in SLEWS:
        for x0 in VALUES:
            for xt in VALUES:
                end = -(-abs(xt - x0) // slew)
                ns = sorted(set([0, 1, 2, end - 1, end, end + 1, end + 7, 65536, 1 << 20]) | set(range(0, end + 1, max(1, end // 50))))
                x, at = x0, {}
                for n in range(end + 8):
                    at[n] = x
                    x = min(x + slew, xt) if x < xt else max(x - slew, xt)
                for n in ns:
                    if n >= 0:
                        assert ar.ramp(x0, xt, slew, n) == at.get(n, xt), (slew, x0, xt, n)
                got = ar.ramp_outputs(x0, xt, slew, 3, end + 4)
                assert [int(v) for v in got] == [at.get(3 + j + 1, xt) for j in range(end + 4)], (slew, x0, xt)


def test_python_reference_blend_is_fp32_faithful():
    """the formula's five roundings, one by one, against exact rational arithmetic on a few values"""
    from fractions import Fraction

    from conftest import round_f32
    rng = np.random.default_rng(5)
    am, as_ = rng.standard_normal(40).astype(np.float32), rng.standard_normal(40).astype(np.float32)
    b, v = rng.integers(0, 32769, 40), rng.integers(0, 32769, 40)
    L, R = ar.blend(am, as_, b, v)
    assert L.dtype == R.dtype == np.float32
    for k in range(40):
        beta, mu = Fraction(int(b[k]), 32768), Fraction(int(v[k]), 32768)
        t = round_f32(beta * Fraction(float(as_[k])))
        lw = round_f32(mu * Fraction(float(round_f32(Fraction(float(am[k])) + Fraction(float(t))))))
        rw = round_f32(mu * Fraction(float(round_f32(Fraction(float(am[k])) - Fraction(float(t))))))
        assert L[k] == lw and R[k] == rw, (k, L[k], lw, R[k], rw)
    ones = np.full(40, 32768)
    L, R = ar.blend(am, as_, ones, ones)
    assert np.array_equal(L, am + as_) and np.array_equal(R, am - as_)
    L, R = ar.blend(am, as_, 0 * ones, ones)
    assert np.array_equal(L, am) and np.array_equal(R, am)
