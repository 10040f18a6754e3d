"""The true-peak meter on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
truepeak_check.cpp holds the lane arithmetic of csrc/sdrfm_truepeak.h (packing, odd and even alignment, half-rows, key reduction, join) to the
definition over every table shape, tests/native/truepeak_sanity.c walks the plain-C host side (csrc/truepeak.c) over its edges.  Then the
default table against the integers and the figures the issue quotes, the bound's edges, the C routine through the library against the numpy
restatement of the definition (tests/truepeak_ref.py) — integer equality of all eight fields — and the Python helpers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import truepeak_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_arithmetic_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "truepeak_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/truepeak_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "truepeak_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/truepeak_sanity.c", "stm32f7-rtlsdr_amd/csrc/truepeak.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _agree(pkg, pcm, coef=None, limit=ref.LIMIT_M1, tag=None):
    """the C routine on this PCM == the reference on it, records and histories; returns the records"""
    c = ref.BS1770 if coef is None else coef
    want, wh = ref.records(pcm, c, limit)
    got, gh = pkg.pcm_truepeak_host(pcm, limit, coef)
    assert ref.same(got, want), (tag, ref.diff(got, want))
    assert np.array_equal(gh, wh), tag
    return got


def test_default_table_is_the_annex_2_filter(pkg):
    """the integers of the issue, the symmetries, and the figures it quotes — re-derived from the table THE LIBRARY returns, which guards the
    transcription in csrc/truepeak.c"""
    c = pkg.truepeak_default_coef()
    assert c.dtype == np.int16 and c.shape == (4, 12)
    assert np.array_equal(c, ref.BS1770) and not (c % 4).any()
    assert np.array_equal(c[0] // 4, ref.PHASE0) and np.array_equal(c[1] // 4, ref.PHASE1)
    assert np.array_equal(c[2], c[1][::-1]) and np.array_equal(c[3], c[0][::-1])
    assert pkg.load_library().sdrfm_truepeak_check_coef(c.ctypes.data, 4, 12) == 0
    a = np.abs(c.astype(np.int64))
    assert a[:, :6].sum(axis=1).tolist() == [8596, 27228, 39056, 38400] and a[:, 6:].sum(axis=1).tolist() == [38400, 39056, 27228, 8596]
    assert a.sum(axis=1).max() == 66284 and 66284 * 32768 > 2 ** 31                          # a whole row can pass 2^31: two half-rows
    assert np.round(c.sum(axis=1) / 32768.0, 4).tolist() == [1.0016, 0.9730, 0.9730, 1.0016]
    # the interleaved 48-tap prototype h[4k + p] = coef[p][k] at 192 kHz
    h = np.zeros(48)
    for p in range(4):
        h[p::4] = c[p]
    f = np.arange(0.0, 96000.5, 100.0)
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(48)) / 192000.0) @ h) / (4 * 32768.0)
    db = 20.0 * np.log10(np.maximum(H, 1e-12))
    assert np.abs(db[f <= 20000.0]).max() <= 0.111
    assert abs(db[f == 24000.0][0] + 6.2) < 0.05
    assert db[f >= 28000.0].max() <= -39.0


def test_check_coef_edges(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    chk = lambda c: lib.sdrfm_truepeak_check_coef(c.ctypes.data, c.shape[0], c.shape[1])
    assert lib.sdrfm_truepeak_check_coef(None, 4, 12) == E
    for P in range(0, 10):
        for NT in range(0, 70):
            ok = P in (2, 4, 8) and 4 <= NT <= 64 and NT % 4 == 0
            assert lib.sdrfm_truepeak_check_coef(np.zeros(max(P * NT, 1), np.int16).ctypes.data, P, NT) == (0 if ok else E), (P, NT)
    for P, NT in ((2, 4), (4, 12), (8, 64)):
        for row in (0, P - 1):
            for half in (0, 1):
                c = np.zeros((P, NT), np.int16)
                c[row, half * (NT // 2)] = -32768
                c[row, half * (NT // 2) + NT // 2 - 1] = 32766
                assert chk(c) == 0                                                          # 65534
                c[row, half * (NT // 2) + NT // 2 - 1] = 32767
                assert chk(c) == 0                                                          # 65535: taken
                if NT > 4:
                    c[row, half * (NT // 2) + 1] = -1
                    assert chk(c) == E                                                      # 65536: refused
                    c[row, half * (NT // 2) + 1] = 0
                c[row, half * (NT // 2)] = -32768
                c[row, half * (NT // 2) + NT // 2 - 1] = -32768
                assert chk(c) == E                                                          # 65536 from two taps
                _agree(pkg, np.full((1, 2 * (NT + 3)), -32768, np.int16), c, 0, "over the bound")   # the host routine does not need the bound
    for P in (2, 4, 8):
        for NT in (4, 12, 16, 64):
            assert chk(ref.bound_table(P, NT)) == 0 and chk(pkg.truepeak_coef(P, NT)) == 0


@pytest.mark.parametrize("n", [0, 1, 10, 11, 12, 13, 4800])
def test_host_routine_against_the_numpy_reference(pkg, n):
    rng = np.random.default_rng(2300 + n)
    L, R = ref.random_full_range(rng, 3, n) if n else (np.zeros((3, 0), np.int64), np.zeros((3, 0), np.int64))
    got = _agree(pkg, ref.interleave(L, R), tag=n)
    assert (got["n"] == n).all() and not got["reserved"].any()
    if n >= 12:
        assert (got["peak_l"] > 0).all() and (got["over_l"] > 0).any()


def test_any_cut_into_calls_gives_the_one_call_record(pkg):
    """3 x 4800 pairs: calls of 1 and of 11 pairs — shorter than the history — among the cuts; records and histories after every call equal the
    reference on the prefix, and the per-call records, each from zero with the history carried, join to it"""
    rng = np.random.default_rng(2400)
    L, R = ref.random_full_range(rng, 2, 3 * 4800)
    pcm = ref.interleave(L, R)
    whole = _agree(pkg, pcm, tag="whole")
    for cuts in ((1, 11, 12, 4800, 7, 4788, 4781), (4800, 4800, 4800), (11, 1, 1, 14387), (14399, 1), (5, 5, 5, 14385)):
        assert sum(cuts) == 3 * 4800
        acc, hist, joined, at = None, None, np.zeros(2, pkg.TRUEPEAK_DTYPE), 0
        for k in cuts:
            piece = pcm[:, 2 * at:2 * (at + k)]
            part, _ = pkg.pcm_truepeak_host(piece, ref.LIMIT_M1, None, hist)
            acc, hist = pkg.pcm_truepeak_host(piece, ref.LIMIT_M1, None, hist, acc)
            at += k
            want, wh = ref.records(pcm[:, :2 * at])
            assert ref.same(acc, want) and np.array_equal(hist, wh), (cuts, at, ref.diff(acc, want))
            pkg.truepeak_add(joined, part)
            assert ref.same(joined, want), (cuts, at)
        assert ref.same(acc, whole)


def test_join_is_associative_with_the_zero_record_as_identity(pkg):
    rng = np.random.default_rng(2500)
    zero = np.zeros(1, pkg.TRUEPEAK_DTYPE)
    for _ in range(300):
        r = np.zeros(3, pkg.TRUEPEAK_DTYPE)
        r["n"] = rng.integers(0, 50, 3)
        for c in "lr":
            r["peak_" + c] = np.where(r["n"] > 0, rng.integers(0, 4, 3), 0)                 # small: ties are common
            r["at_" + c] = np.where(r["peak_" + c] > 0, rng.integers(0, 50, 3) % np.maximum(r["n"], 1), 0)
            r["over_" + c] = rng.integers(0, 9, 3)
        a, b, c_ = r[0:1].copy(), r[1:2].copy(), r[2:3].copy()
        left = pkg.truepeak_add(pkg.truepeak_add(a.copy(), b), c_)
        right = pkg.truepeak_add(a.copy(), pkg.truepeak_add(b.copy(), c_))
        assert ref.same(left, right)
        assert ref.same(left[0], ref.join(ref.join(a[0], b[0]), c_[0]))
        assert ref.same(pkg.truepeak_add(zero.copy(), a), a) and ref.same(pkg.truepeak_add(a.copy(), zero), a)


def test_at_ties_resolve_to_the_earlier_pair(pkg):
    """the same burst twice, 100 pairs apart and across a call boundary: the peak is attained twice and at_* names the first"""
    burst = np.array([3000, -20000, 30000, -20000, 3000])
    L = np.zeros(300, np.int64)
    L[50:55] = burst
    L[150:155] = burst
    pcm = ref.interleave(L, -L)[None, :]
    got = _agree(pkg, pcm)
    first, _ = ref.record(pcm[0, :200])
    assert int(got["at_l"][0]) == int(first["at_l"]) < 100 and int(got["peak_l"][0]) == int(first["peak_l"]) and int(got["at_r"][0]) == int(got["at_l"][0])
    a, h = pkg.pcm_truepeak_host(pcm[:, :200])
    b, _ = pkg.pcm_truepeak_host(pcm[:, 200:], hist=h)
    assert int(b["peak_l"][0]) == int(a["peak_l"][0])                                        # the second call attains it too
    assert ref.same(pkg.truepeak_add(a, b), got)


def test_quarter_rate_tone_reads_three_db_over_its_sample_peak(pkg):
    """fs / 4 sampled at 45 degrees: every sample is 16384 and the reconstruction peaks at 16384 sqrt(2)"""
    L = 16384 * np.tile([1, 1, -1, -1], 64)
    pcm = ref.interleave(L, np.zeros_like(L))
    got = _agree(pkg, pcm)
    assert int(got["peak_l"][0]) == 766509056 == 23392 << 15 and int(got["peak_r"][0]) == 0 and int(got["at_r"][0]) == 0
    rep = pkg.truepeak_report(got)
    assert abs(rep["dbtp_l"][0] - 20.0 * np.log10(16384 / 32768) - 3.01) <= 0.1              # the filter's own passband ripple, +-0.11 dB
    assert rep["dbtp_r"][0] == -np.inf and rep["dbtp"][0] == rep["dbtp_l"][0]


def test_32_bit_trap(pkg):
    """phase 1's row lined up with matching signs at the rails: the whole-row sum passes 2^31 - 1"""
    L, R = ref.trap_row(64)
    assert L[:12].tolist() == [32767 if ref.BS1770[1][11 - i] >= 0 else -32768 for i in range(12)] and not L[12:].any()
    got = _agree(pkg, ref.interleave(L, R), limit=0x7FFFFFFF)
    assert int(got["peak_l"][0]) == 2171945028 > 2 ** 31 - 1 and int(got["at_l"][0]) == 11 and int(got["over_l"][0]) >= 1


def test_limit_report_alarms_and_headroom(pkg):
    assert pkg.truepeak_limit(0.0) == 1 << 30 and pkg.truepeak_limit(-1.0) == ref.LIMIT_M1 and pkg.truepeak_limit(float("nan")) == 0
    assert pkg.truepeak_limit(1000.0) == 0xFFFFFFFF and pkg.truepeak_limit(-1000.0) == 0 and pkg.truepeak_limit(float("-inf")) == 0
    for d in (-60.0, -23.0, -6.0, -0.5, 3.0, 12.0):
        assert pkg.truepeak_limit(d) == int(np.floor(2.0 ** 30 * 10.0 ** (d / 20.0)))
    r = np.zeros(4, pkg.TRUEPEAK_DTYPE)
    r["n"] = (4800, 4800, 4800, 0)
    r["peak_l"] = (1 << 30, 1 << 29, 0, 0)
    r["peak_r"] = (1 << 29, 3 << 29, 0, 0)
    r["at_l"], r["over_r"] = (48, 0, 0, 0), (0, 96, 0, 0)
    rep = pkg.truepeak_report(r, 4, 48000.0)
    assert rep["dbtp_l"][0] == 0.0 and abs(rep["dbtp_r"][0] + 6.0206) < 1e-4 and rep["dbtp"][0] == 0.0 and rep["at_seconds_l"][0] == 0.001
    assert abs(rep["dbtp"][1] - 3.5218) < 1e-4 and rep["over_frac_r"][1] == 96 / 19200 and rep["dbtp"][2] == -np.inf and np.isnan(rep["dbtp"][3])
    al = pkg.truepeak_alarms(rep)
    assert al[0] == dict(over=True, over_l=True, over_r=False, overshoot=False) and al[1] == dict(over=True, over_l=False, over_r=True, overshoot=True)
    assert not any(al[2].values()) and not any(al[3].values())
    assert not pkg.truepeak_alarms(rep, max_dbtp=4.0)[1]["over"]
    g = pkg.headroom_gain_q15(rep, -1.0)
    assert g.dtype == np.uint16 and g.tolist() == [int(np.floor(32768 * 10 ** (-1 / 20))), int(np.floor(32768 * 10 ** (-(rep["dbtp"][1] + 1) / 20))), 32768, 32768]
    assert pkg.headroom_gain_q15(rep, 6.0).tolist() == [32768] * 4
    for s in range(2):                                                                       # the scaled peak is at or under the target
        assert rep["dbtp"][s] + 20 * np.log10(g[s] / 32768.0) <= -1.0
    with pytest.raises(pkg.SdrfmError):
        pkg.truepeak_report(r, 3)
    with pytest.raises(pkg.SdrfmError):
        pkg.pcm_truepeak_host(np.zeros(8, np.int16), 1 << 32)


def test_designed_tables(pkg):
    """taps.truepeak_coef: inside the bound, rows that sum to 32768, row P - 1 - p is row p reversed, and it interpolates — a slow sine's true
    peak is its amplitude within the table's ripple"""
    for P in (2, 4, 8):
        for NT in (4, 12, 16, 64):
            c = pkg.truepeak_coef(P, NT)
            assert c.dtype == np.int16 and c.shape == (P, NT) and (c.astype(np.int64).sum(axis=1) == 32768).all()
            assert np.array_equal(c[::-1, ::-1], c)
            a = np.abs(c.astype(np.int64))
            assert a[:, :NT // 2].sum(axis=1).max() <= 65535 and a[:, NT // 2:].sum(axis=1).max() <= 65535
            t = np.arange(2000)
            L = np.rint(20000 * np.sin(2 * np.pi * 0.013 * t + 0.3)).astype(np.int64)
            got = _agree(pkg, ref.interleave(L, L), c, 0, (P, NT))
            assert abs(int(got["peak_l"][0]) / 32768.0 / 20000.0 - 1.0) < (0.02 if NT >= 12 else 0.2), (P, NT)
    for bad in ((3, 12), (4, 10), (4, 68), (4, 0)):
        with pytest.raises(ValueError):
            pkg.truepeak_coef(*bad)
