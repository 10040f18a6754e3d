"""The (L, R) row checks of csrc/sdrfm_pcm_rows.h on the CPU: tests/native/pcm_rows_check.cpp, a program of its own built with
ASan and UBSan and run as a program.  It holds pcm_rows_refusal to the order the limiter's, the mix bus's and the rate matcher's entries have
always had (every combination of the nine defects, on host and on device rows), the single-row stride exemption, the mix bus's overlap test to a
walk over the bytes, and stage_cap at 0, 1, 1023, 1024, 1025, every handle's maximum and where its uint32 sum wraps.  The header has no HIP in it:
the same file compiles as C."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
HEADER = os.path.join(ROOT, "stm32f7-rtlsdr_amd", "csrc", "sdrfm_pcm_rows.h")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_row_checks_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pcm_rows_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/pcm_rows_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_header_is_plain_c_without_hip(tmp_path):
    src = tmp_path / "rows.c"
    src.write_text('#include "%s"\nint main(void) { return pcm_rows_capacity(1, 0, 2) && stage_cap(1, 1024u) == 1024u ? 0 : 1; }\n' % HEADER)
    exe = str(tmp_path / "rows")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-o", exe, str(src)], check=True, capture_output=True, text=True)
    assert subprocess.run([exe], timeout=60).returncode == 0
    assert "#include <hip" not in open(HEADER).read()
