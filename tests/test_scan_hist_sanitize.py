"""ASan and UBSan over the histogram side of csrc/scan.c on the CPU: tests/native/scan_hist_sanity.c is a program of its own that calls
sdrfm_scan_hist_add and sdrfm_scan_hist_report on edge rows; it is compiled with the sanitizers and run as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_scan_hist_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "scan_hist_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/scan_hist_sanity.c", "stm32f7-rtlsdr_amd/csrc/scan.c")]
    cmd = ["gcc", "-O1", "-g", "-std=c99", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr
