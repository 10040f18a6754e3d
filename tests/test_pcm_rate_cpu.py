"""The PCM rate matcher on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
pcm_rate_check.cpp holds the count, advance and span arithmetic of csrc/sdrfm_pcm_rate.h to naive 128-bit arithmetic, tests/native/pcm_rate_sanity.c
walks the plain-C host side (csrc/pcm_rate.c) over its edges.  Then the C routine through the library against tests/pcm_rate_ref.py (the int64
numpy restatement the GPU tests use), the quality of the default table on tones, and ClockServo against a simulated consumer.  Every comparison
of samples, counts, pos and hist is integer equality; the only tolerance is the SNR test's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_rate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ONE = 1 << 32


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_header_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pcm_rate_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/pcm_rate_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pcm_rate_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/pcm_rate_sanity.c", "stm32f7-rtlsdr_amd/csrc/pcm_rate.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _same(got, want):
    return got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("step", ref.STEPS)
def test_c_routine_is_the_definition(pkg, step):
    rng = np.random.default_rng(21)
    for nt, logph in ((32, 8), (4, 4), (64, 4), (8, 6)):
        coef = pkg.rate_coef(nt, logph, step=step) if nt >= 32 else ref.small_table(nt, logph)
        x = ref.random_full_range(rng, 2 * 700)
        got, want = pkg.pcm_rate_host(x, coef, step), ref.process(x, coef, step)
        assert _same(got, want), (step, nt, logph)
        assert got[0].size // 2 == -((-700 * ONE) // step)
        got2, want2 = pkg.pcm_rate_host(x[:600], coef, step, got[1], got[2]), ref.process(x[:600], coef, step, want[1], want[2])   # from a carried state
        assert _same(got2, want2), (step, nt, logph)


def test_cut_invariance_over_ragged_cuts(pkg):
    """any cut of a row into calls, 0-length and sub-NT pieces included, gives the row's outputs, pos and hist"""
    rng = np.random.default_rng(22)
    cuts = [1, 0, 2, 30, 31, 32, 1, 1, 1, 257, 64, 0, 3, 700, 5]
    n = sum(cuts)
    x = ref.random_full_range(rng, 2 * n)
    rails = 0
    coef = pkg.rate_coef(32, 8, 0.9)                                   # one table at every step: what is checked here is the arithmetic
    for step in ref.STEPS:
        whole = pkg.pcm_rate_host(x, coef, step)
        assert _same(whole, ref.process(x, coef, step))
        r_out, r_pos, r_hist = ref.run(x, coef, step, cuts)
        pos, hist, at, outs = 0, None, 0, []
        for k, c in enumerate(cuts):
            o, pos, hist = pkg.pcm_rate_host(x[2 * at:2 * (at + c)], coef, step, pos, hist)
            assert pos == r_pos[k] and np.array_equal(o, r_out[k]), (step, k)
            outs.append(o)
            at += c
        assert pos == whole[1] and np.array_equal(hist, whole[2]) and np.array_equal(hist, r_hist) and np.array_equal(np.concatenate(outs), whole[0]), step
        rails += int((whole[0] == -32768).sum() > 0) + int((whole[0] == 32767).sum() > 0)
    assert rails == 2 * len(ref.STEPS)                                 # full-range noise overshoots: both rails at every step


def test_the_vectorised_reference_is_the_reference(pkg):
    """ref.process_fast — what tests/test_pcm_rate_tables_gpu.py holds calls of 2^20 pairs to — against ref.process, at every step, from reset and
    from a carried state, with chunks smaller than a call so that their seams are crossed; and once against the C routine on a call of 2^17 pairs"""
    rng = np.random.default_rng(25)
    x = ref.random_full_range(rng, 2 * 1500)
    for nt, logph in ((4, 4), (12, 5), (64, 8)):
        coef = ref.small_table(nt, logph, overshoot=True)
        for step in ref.STEPS:
            a, b = ref.process(x[:2000], coef, step), ref.process_fast(x[:2000], coef, step, chunk=97)
            assert _same(a, b), (nt, step)
            assert _same(ref.process(x[2000:], coef, step, a[1], a[2]), ref.process_fast(x[2000:], coef, step, b[1], b[2], chunk=64)), (nt, step)
            assert _same(ref.process(x[:2], coef, step, a[1], a[2]), ref.process_fast(x[:2], coef, step, b[1], b[2])), (nt, step)   # often no output at all
    coef = ref.small_table(4, 4, overshoot=True)
    big = ref.random_full_range(rng, 2 * (1 << 17))
    for step in (1 << 30, (1 << 34) - 1):
        assert _same(pkg.pcm_rate_host(big, coef, step), ref.process_fast(big, coef, step)), step


def test_a_constant_comes_out_as_itself(pkg):
    for step in ref.STEPS:
        for nt, logph, cutoff in ((32, 8, None), (48, 8, 0.9), (16, 4, 0.5)):
            coef = pkg.rate_coef(nt, logph, cutoff, step=step)
            assert (coef.astype(np.int64).sum(axis=1) == 32768).all()
            for c in (-32768, -1, 0, 1, 12345, 32767):
                x = np.tile(np.array([c, -c if c != -32768 else 7], np.int16), 300)
                out, _, _ = pkg.pcm_rate_host(x, coef, step, 0, np.tile(x[:2], nt - 1))   # the history holds the constant as well
                assert out.size and (out[0::2] == x[0]).all() and (out[1::2] == x[1]).all(), (step, nt, c)


def test_phase_edges_read_the_rows_they_should(pkg):
    """f = 0 uses row 0 only; p = NPH - 1 with mu = 255 reads row NPH"""
    nt, logph = 8, 4
    rng = np.random.default_rng(23)
    x = ref.random_full_range(rng, 2 * 40)
    base = ref.small_table(nt, logph)
    # step 2^32 from pos 0: every f is 0 — rows 1 .. NPH may hold anything
    other = base.copy()
    other[1:] = ref.small_table(nt, logph, np.random.default_rng(99))[1:]
    a, b = pkg.pcm_rate_host(x, base, ONE), pkg.pcm_rate_host(x, other, ONE)
    assert np.array_equal(a[0], b[0]) and a[0].size == 80 and _same(a, ref.process(x, base, ONE))
    want = np.clip(((base[0].astype(np.int64)[None, :, None] * np.concatenate([np.zeros((nt - 1, 2), np.int64), x.reshape(-1, 2)])[
        np.arange(40)[:, None] + np.arange(nt)[None, :]]).sum(axis=1) * 256 + (1 << 22)) >> 23, -32768, 32767)
    assert np.array_equal(a[0].reshape(-1, 2), want)
    # pos = 2^32 - 1: p = NPH - 1, mu = 255 — a change of row NPH changes the output, a change of rows 0 .. NPH - 2 does not
    pos = ONE - 1
    first = pkg.pcm_rate_host(x, base, ONE, pos)
    assert _same(first, ref.process(x, base, ONE, pos))
    moved = base.copy()
    moved[-1] = -base[-1] - 1
    assert not np.array_equal(pkg.pcm_rate_host(x, moved, ONE, pos)[0], first[0]) and _same(pkg.pcm_rate_host(x, moved, ONE, pos), ref.process(x, moved, ONE, pos))
    low = base.copy()
    low[:-2] = other[2:]
    assert np.array_equal(pkg.pcm_rate_host(x, low, ONE, pos)[0], first[0])


def test_both_rails_on_a_table_with_overshoot(pkg):
    nt, logph = 16, 4
    coef = ref.small_table(nt, logph, overshoot=True)
    a = np.abs(coef.astype(np.int64))
    assert (a[:, :nt // 2].sum(axis=1) == 65535).all() and (a[:, nt // 2:].sum(axis=1) == 65535).all()
    assert pkg.load_library().sdrfm_pcm_rate_check_coef(coef.ctypes.data, nt, logph) == 0
    # the input that drives row 0 to its extremes: x = +-32768 sign(coef) around pair 100 and 200 — the sums reach -+65535 * 32768 per half
    x = np.zeros((400, 2), np.int16)
    sgn = np.where(coef[0] >= 0, 1, -1)
    x[100 - nt + 1:101, 0] = np.where(sgn > 0, 32767, -32768)
    x[100 - nt + 1:101, 1] = np.where(sgn > 0, -32768, 32767)
    got, want = pkg.pcm_rate_host(x.reshape(-1), coef, ONE), ref.process(x.reshape(-1), coef, ONE)
    assert _same(got, want)
    assert got[0][2 * 100] == 32767 and got[0][2 * 100 + 1] == -32768
    noise = ref.random_full_range(np.random.default_rng(24), 2 * 2000)
    for step in ref.STEPS:
        got = pkg.pcm_rate_host(noise, coef, step)
        assert _same(got, ref.process(noise, coef, step)) and (got[0] == 32767).any() and (got[0] == -32768).any()


def test_check_coef_is_exact_at_the_bound(pkg):
    lib = pkg.load_library()
    for nt, logph in ((4, 4), (32, 8), (64, 8)):
        rows, half = (1 << logph) + 1, nt // 2
        for p in (0, rows // 2, rows - 1):
            for h in range(2):
                coef = np.zeros((rows, nt), np.int16)
                coef[p, h * half], coef[p, h * half + 1] = 32767, -32768                  # 65535
                assert lib.sdrfm_pcm_rate_check_coef(coef.ctypes.data, nt, logph) == 0, (nt, p, h)
                coef[p, (1 - h) * half], coef[p, (1 - h) * half + 1] = -32768, 32767      # ... and the other half its own 65535
                assert lib.sdrfm_pcm_rate_check_coef(coef.ctypes.data, nt, logph) == 0, (nt, p, h)
                coef[p, h * half] = -32768                                                # 65536
                assert lib.sdrfm_pcm_rate_check_coef(coef.ctypes.data, nt, logph) == pkg.lib.EINVAL, (nt, p, h)
    assert lib.sdrfm_pcm_rate_check_coef(pkg.rate_coef(48, 8, 0.9).ctypes.data, 48, 8) == 0     # over 65535 for the whole row, legal per half
    assert int(np.abs(pkg.rate_coef(48, 8, 0.9).astype(np.int64)).sum(axis=1).max()) > 65535
    assert int(np.abs(pkg.rate_coef(32, 8, 0.9).astype(np.int64)).sum(axis=1).max()) == 64268


def test_step_for_rounds_exactly(pkg):
    from fractions import Fraction
    assert pkg.step_for(48000, 48000) == ONE and pkg.step_for(48000, 44100) == round(Fraction(480, 441) * ONE) == ref.STEPS[4]
    assert pkg.step_for(48000, 48000, 100) == ONE + 429497 and pkg.step_for(48000, 48000, -100) == ONE - 429497
    assert pkg.step_for(48000, 32000) == 3 * ONE // 2 and pkg.step_for(48000, 192000) == 1 << 30 and pkg.step_for(48000, 12000) == 1 << 34
    for fs_in, fs_out in ((48000, 11025), (48000, 200000)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.step_for(fs_in, fs_out)
        assert e.value.status == pkg.lib.EINVAL


def _snr_db(pkg, freq, step, cutoff):
    """a 1 s tone of amplitude 30000 through the host routine against the float64 tone at the defined output instants"""
    nt, fs, n = 32, 48000.0, 48000
    coef = pkg.rate_coef(nt, 8, cutoff)
    t = np.arange(n)
    tone = np.rint(30000.0 * np.sin(2 * np.pi * freq * t / fs)).astype(np.int16)
    out, _, _ = pkg.pcm_rate_host(np.repeat(tone, 2), coef, step)
    y = out[0::2].astype(np.float64)
    assert np.array_equal(out[0::2], out[1::2])
    j = np.arange(y.size, dtype=object)
    P = j * step                                                       # exact: Python integers
    at = np.array([(int(v) >> 32) - nt // 2 + (int(v) & 0xFFFFFFFF) / ONE for v in P], np.float64)   # input time of output j, in input pairs
    want = 30000.0 * np.sin(2 * np.pi * freq * at / fs)
    keep = slice(4 * nt, y.size - 4 * nt)
    err = y[keep] - want[keep]
    return 10 * np.log10((want[keep] ** 2).mean() / (err ** 2).mean())


@pytest.mark.parametrize("freq", [1000.0, 10000.0, 15000.0])
def test_default_table_quality(pkg, freq):
    """SNR >= 80 dB for tones at 1, 10 and 15 kHz through the default table: drift-locked at +-100 ppm with cutoff 0.9, and to 44.1 kHz with cutoff
    0.9 * 44.1 / 48.  (The numpy restatement of the definition gives 83.1 - 85.9 dB.)"""
    for step, cutoff in ((ONE + 429497, 0.9), (ONE - 429497, 0.9), (ref.STEPS[4], 0.9 * 44.1 / 48)):
        snr = _snr_db(pkg, freq, step, cutoff)
        print("tone %.0f Hz, step %d: %.1f dB" % (freq, step, snr))
        assert snr >= 80.0, (freq, step, snr)


@pytest.mark.parametrize("ppm", [-200, -50, 0, 50, 200])
def test_clock_servo_holds_the_ring(pkg, ppm):
    """a consumer at 48000 (1 + ppm / 1e6) pairs/s empties a 0.5 s ring that starts half full; the producer is pcm_rate_host in calls of 4800 pairs
    (0.1 s of the dongle's clock) at the servo's step: over 10 simulated minutes the ring neither empties nor fills, and the mean step over the
    last minute is within 5 ppm of the true ratio"""
    ring, call = 24000, 4800
    servo = pkg.ClockServo(ring // 2, ring)
    coef = ref.small_table(4, 4)                                       # the counts do not depend on the table: the smallest one
    x = np.zeros(2 * call, np.int16)
    fill, pos, hist, step = ring // 2, 0, None, servo.step
    taken, steps = 0, []
    for k in range(6000):
        out, pos, hist = pkg.pcm_rate_host(x, coef, step, pos, hist)
        fill += out.size // 2
        due = (48000 * (1000000 + ppm) * (k + 1)) // (10 * 1000000)   # the pairs the consumer has played after k + 1 tenths of a second
        fill -= due - taken
        taken = due
        assert 0 < fill < ring, (k, fill)
        step = servo.update(fill)
        steps.append(step)
    mean = sum(steps[-600:]) / 600.0
    true = ONE / (1.0 + ppm * 1e-6)
    assert abs(mean / true - 1.0) <= 5e-6, (ppm, (mean / true - 1.0) * 1e6)
    assert abs(fill - ring // 2) <= ring // 50                         # ... and the ring is back at its target
