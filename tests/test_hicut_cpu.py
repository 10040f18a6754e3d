"""CPU: the host routine of the stereo PCM sink's ramped high-cut, sdrfm_pcm_deemph_stereo_hicut_s16 (csrc/pcm_sink.c; include/sdrfm.h,
DESIGN.md §4.17) — the reference of the device sink's conditioned forms — held to tests/hicut_ref.py, the definition in numpy fp32 with
the ramp in Python ints: bit for bit over the slews, both directions and per-stream pairs; h = 32768 is the plain routine; any cut into
calls is the one call; the saturated count; every refusal.  tests/native/hicut_check.c exercises it at edge sizes as a program of its own
under ASan and UBSan.  The ramp of hicut_ref.py is held to the one-sample-at-a-time iteration first."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import hicut_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLEWS = (1, 7, 40, 32768)
VALUES = (1024, 1025, 8192, 32767, 32768)
PAIRS = [(a, b) for a in VALUES for b in VALUES]                  # both directions and the flat ones
GAIN = float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(ns, n, seed=11):
    rng = np.random.default_rng(seed)
    left = (rng.standard_normal((ns, n)) * 1.5).astype(np.float32)
    right = (rng.standard_normal((ns, n)) * 1.5).astype(np.float32)
    head = np.array([9.0, -9.0, 0.0, 1e-30, 0.5, -0.5], np.float32)[: min(6, n)]
    left[0, : head.size], right[0, : head.size] = head, -head                   # row 0 saturates both channels
    return left, right


def _host(pkg, left, right, alpha, gain, h0, ht, slew, J=0, state=None):
    ns = left.shape[0]
    pcm = np.zeros((ns, 2 * left.shape[1]), np.int16)
    st = np.zeros((ns, 2), np.float32)
    for s in range(ns):
        pcm[s], st[s] = pkg.pcm_deemph_stereo_hicut_s16_host(left[s], right[s], alpha, gain, h0[s], ht[s], slew, J,
                                                             (0.0, 0.0) if state is None else tuple(state[s]))
    return pcm, st


def test_reference_ramp_is_the_iteration():
    for slew in (1, 2, 7, 40, 32767, 32768):
        for h0, ht in PAIRS:
            end = -(-abs(ht - h0) // slew)
            x, at = h0, {}
            for n in range(end + 8):
                at[n] = x
                x = min(x + slew, ht) if x < ht else max(x - slew, ht)
            for n in sorted({0, 1, 2, max(end - 1, 0), end, end + 1, end + 7, 65535, 65536, 1 << 20} | set(range(0, end + 1, max(1, end // 40)))):
                assert hr.ramp(h0, ht, slew, n) == at.get(n, ht), (slew, h0, ht, n)
            got = hr.ramp_samples(h0, ht, slew, 3, min(end + 4, 50))
            assert [int(v) for v in got] == [at.get(3 + i + 1, ht) for i in range(got.size)]


def test_reference_fma_is_correctly_rounded():
    """fma32 against exact rational arithmetic, on draws and on sums that sit on a float32 tie only the exact residual can break"""
    from fractions import Fraction

    from conftest import round_f32
    rng = np.random.default_rng(3)
    a = rng.standard_normal(60).astype(np.float32)
    b = rng.standard_normal(60).astype(np.float32)
    c = rng.standard_normal(60).astype(np.float32)
    a[:3], b[:3], c[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), [np.float32(2.0 ** -24), np.float32(-2.0 ** -24), np.float32(2.0 ** 30)]
    a[3], b[3], c[3] = np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1.0), np.float32(1.0)      # 1 + half an ulp + a little: up
    got = hr.fma32(a, b, c)
    for k in range(60):
        assert got[k] == round_f32(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))), k


@pytest.mark.parametrize("aname", ["75us", "50us"])
@pytest.mark.parametrize("slew", SLEWS)
def test_host_routine_is_the_definition_bit_for_bit(pkg, slew, aname):
    """one stream per (h0, ht) pair of VALUES x VALUES — 25 streams, both directions, the flat ones —, 700 samples: at slew 40 the longest
    ramp ends inside (794 samples would; so J = 150 starts it in mid-ramp), at 1 and 7 it runs throughout, at 32768 it is a jump"""
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, float(aname[:-2]) * 1e-6))
    h0, ht = np.array([p[0] for p in PAIRS[::-1]]), np.array([p[1] for p in PAIRS[::-1]])     # (row 0, whose head saturates: a flat 32768)
    left, right = _inputs(len(PAIRS), 700)
    for J in (0, 150):
        want, st = hr.hicut_ref(left, right, alpha, GAIN, h0, ht, slew, J)
        got, st_host = _host(pkg, left, right, alpha, GAIN, h0, ht, slew, J)
        assert np.array_equal(got, want), (slew, J, np.argwhere(got != want)[:4])
        assert np.array_equal(_bits(st_host), _bits(st)), (slew, J)
    assert want[0, 0::2].max() == 32767 and want[0, 1::2].min() == -32768


@pytest.mark.parametrize("alpha", [1.0, 0.05, 0.5])
def test_host_routine_is_the_definition_at_other_alphas(pkg, alpha):
    h0, ht = np.array([1024, 32768, 2622, 8192]), np.array([32768, 1024, 2622, 32767])
    left, right = _inputs(4, 300, seed=12)
    for slew in (7, 32768):
        want, st = hr.hicut_ref(left, right, alpha, -GAIN, h0, ht, slew, 5)
        got, st_host = _host(pkg, left, right, alpha, -GAIN, h0, ht, slew, 5)
        assert np.array_equal(got, want) and np.array_equal(_bits(st_host), _bits(st)), (alpha, slew)


def test_a_flat_32768_is_the_plain_routine_bit_for_bit(pkg):
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    left, right = _inputs(3, 500, seed=13)
    for s in range(3):
        want, st = pkg.pcm_deemph_stereo_s16_host(left[s], right[s], alpha, GAIN, (0.125, -0.25))
        for slew, J in ((1, 0), (32768, 77), (40, 1 << 31)):
            got, st_h = pkg.pcm_deemph_stereo_hicut_s16_host(left[s], right[s], alpha, GAIN, 32768, 32768, slew, J, (0.125, -0.25))
            assert np.array_equal(got, want) and np.array_equal(_bits(st_h), _bits(st)), (s, slew, J)
    # ... and a ramp that has arrived at 32768 long ago
    got, st_h = pkg.pcm_deemph_stereo_hicut_s16_host(left[0], right[0], alpha, GAIN, 1024, 32768, 1, 65536)
    want, st = pkg.pcm_deemph_stereo_s16_host(left[0], right[0], alpha, GAIN)
    assert np.array_equal(got, want) and np.array_equal(_bits(st_h), _bits(st))


@pytest.mark.parametrize("cuts", [(0, 1, 18, 19, 20, 500), (500, 20, 19, 18, 1, 0), (1, 1, 0, 0, 556), (558,)])
def test_any_cut_into_calls_gives_the_one_call(pkg, cuts):
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 50e-6))
    n = sum(cuts)
    assert n == 558
    left, right = _inputs(2, n, seed=14)
    for (h0, ht), slew in itertools.product([(1024, 32768), (32768, 1025)], (7, 40)):
        for s in range(2):
            want, st = pkg.pcm_deemph_stereo_hicut_s16_host(left[s], right[s], alpha, GAIN, h0, ht, slew, 9)
            J, at, state, parts = 9, 0, (0.0, 0.0), []
            for c in cuts:
                p, state = pkg.pcm_deemph_stereo_hicut_s16_host(left[s, at:at + c], right[s, at:at + c], alpha, GAIN, h0, ht, slew, J, state)
                parts.append(p)
                J, at = min(J + c, 65536), at + c
            assert np.array_equal(np.concatenate(parts), want) and np.array_equal(_bits(state), _bits(st)), (h0, ht, slew, s)
            assert hr.ramp(h0, ht, slew, 9 + n) != ht                                                       # the ramp was still running at every cut


def test_a_saturated_count_is_a_completed_ramp(pkg):
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    left, right = _inputs(1, 200, seed=15)
    flat, st = pkg.pcm_deemph_stereo_hicut_s16_host(left[0], right[0], alpha, GAIN, 8192, 8192, 1, 0)
    for J in (65536, 65537, 0xFFFFFFFF):
        got, st_j = pkg.pcm_deemph_stereo_hicut_s16_host(left[0], right[0], alpha, GAIN, 32768, 8192, 1, J)
        assert np.array_equal(got, flat) and np.array_equal(_bits(st_j), _bits(st)), J
    # one sample before the longest ramp's end (slew 1: 24576 samples) the last step is still to come
    got, _ = pkg.pcm_deemph_stereo_hicut_s16_host(left[0], right[0], alpha, GAIN, 32768, 8192, 1, 24574)
    assert not np.array_equal(got, flat)
    # a count near the top of 32 bits does not wrap
    got, _ = pkg.pcm_deemph_stereo_hicut_s16_host(left[0], right[0], alpha, GAIN, 32768, 8192, 1, 0xFFFFFFFF - 3)
    assert np.array_equal(got, flat)


def test_every_refusal(pkg):
    lib = pkg.load_library()
    E = pkg.lib.EINVAL
    x = np.arange(4, dtype=np.float32)
    pcm = np.full(8, 0x5555, np.int16)
    st = (C.c_float * 2)(0.5, 0.5)
    call = lambda l, r, n, a, h0, ht, slew, s, p: lib.sdrfm_pcm_deemph_stereo_hicut_s16(l, r, n, a, 1.0, h0, ht, slew, 0, s, p)
    xp, pp = x.ctypes.data, pcm.ctypes.data
    assert call(None, xp, 4, 0.25, 32768, 32768, 1, st, pp) == E
    assert call(xp, None, 4, 0.25, 32768, 32768, 1, st, pp) == E
    assert call(xp, xp, 4, 0.25, 32768, 32768, 1, st, None) == E
    assert call(xp, xp, 4, 0.25, 32768, 32768, 1, None, pp) == E
    for a in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        assert call(xp, xp, 4, a, 32768, 32768, 1, st, pp) == E, a
    for h in (0, 1023, 32769, 65535):
        assert call(xp, xp, 4, 0.25, h, 32768, 1, st, pp) == E, h
        assert call(xp, xp, 4, 0.25, 32768, h, 1, st, pp) == E, h
    for slew in (0, 32769, 0xFFFFFFFF):
        assert call(xp, xp, 4, 0.25, 32768, 32768, slew, st, pp) == E, slew
    assert (pcm == 0x5555).all() and st[0] == 0.5 and st[1] == 0.5
    assert call(None, None, 0, 0.25, 1024, 32768, 32768, st, None) == 0                       # n == 0: nothing is read or written
    assert call(xp, xp, 4, 1.0, 1024, 1024, 32768, st, pp) == 0                                # the smallest value, the largest alpha and slew
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_deemph_stereo_hicut_s16_host(x, x, 0.25, 1.0, 1023, 32768, 1)
    assert e.value.status == E
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_deemph_stereo_hicut_s16_host(x, x, 0.25, 1.0, 70000, 32768, 1)
    assert e.value.status == E


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_routine_clean_under_asan_and_ubsan(tmp_path):
    """csrc/pcm_sink.c with its own flags and tests/native/hicut_check.c, one program, nothing loaded into Python"""
    exe = str(tmp_path / "hicut_check")
    cmd = ["gcc", "-O1", "-g", "-std=c99", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests/native/hicut_check.c"),
           os.path.join(ROOT, "stm32f7-rtlsdr_amd/csrc/pcm_sink.c"), "-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr
