"""UBSan (undefined behaviour, array bounds) over the plain-C RDS decoder csrc/rds.c on the CPU, driven by tests/native/rds_sanity.c at
every sample rate the decoder accepts: its rings and histogram are sized by the rate."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_rds_decoder_clean_under_ubsan(tmp_path):
    exe = str(tmp_path / "rds_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/rds_sanity.c", "stm32f7-rtlsdr_amd/csrc/rds.c")]
    cmd = ["gcc", "-O1", "-g", "-std=c99", "-Wall", "-fsanitize=undefined,bounds", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr
