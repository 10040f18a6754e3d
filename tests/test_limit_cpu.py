"""The look-ahead PCM limiter on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
limit_check.cpp holds the arithmetic of csrc/sdrfm_limit.h — the (min, +) maps, the scan in the kernel's order, the doubling windows, the record
join — to one-pair-at-a-time iteration, tests/native/limit_sanity.c walks the plain-C host side (csrc/limit.c) over its edges.  Then the C routine
through the library against tests/limit_ref.py (the int64 numpy restatement of the definition).  Every comparison is integer equality of PCM, all
4 D state words and all four record fields."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import limit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LWS = [2, 3, 6, 8]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_header_arithmetic_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "limit_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/limit_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "limit_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/limit_sanity.c", "stm32f7-rtlsdr_amd/csrc/limit.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _params(corner):
    C, G, delta = corner
    return (C, delta, G, G)


def _same(pkg, got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1][0], want[1]) and ref.rec_tuple(got[2][0]) == want[2]


@pytest.mark.parametrize("lw", LWS)
@pytest.mark.parametrize("corner", ref.CORNERS)
def test_c_routine_is_the_definition_and_the_ceiling_holds(pkg, lw, corner):
    rng = np.random.default_rng(41)
    par = _params(corner)
    x = ref.random_full_range(rng, 2 * 700)
    got, want = pkg.pcm_limit_host(x, lw, 1, 0, par), ref.process(x, lw, 1, 0, par)
    assert _same(pkg, got, want), (lw, corner)
    assert int(np.abs(got[0].astype(np.int64)).max()) <= corner[0]
    got2 = pkg.pcm_limit_host(x[:600], lw, 1, 0, par, got[1], got[2])     # from a carried state, joined onto the first record
    want2 = ref.process(x[:600], lw, 1, 0, par, want[1])
    assert np.array_equal(got2[0], want2[0]) and np.array_equal(got2[1][0], want2[1]) and ref.rec_tuple(got2[2][0]) == ref.join(want[2], want2[2])
    assert int(np.abs(got2[0].astype(np.int64)).max()) <= corner[0]
    if corner[1] == 0:
        assert not got[0].any() and want[2][1] == 0                        # a gain of 0: silence, nothing limited


@pytest.mark.parametrize("lw", LWS)
def test_transparency(pkg, lw):
    """G = 4096 and no |x| over C: y[u] = x[u - D] bit for bit, nothing limited"""
    rng = np.random.default_rng(42)
    D = (1 << lw) - 1
    for C in (29204, 1, 32767):
        x = rng.integers(-C, C + 1, size=2 * 900, dtype=np.int64).astype(np.int16)
        x[[0, 3]], x[[5, 8]] = C, -C
        y, st, rec = pkg.pcm_limit_host(x, lw, 1, 0, (C, 874, 4096, 4096))
        assert np.array_equal(y[2 * D:], x[:-2 * D]) and not y[:2 * D].any(), (lw, C)
        assert ref.rec_tuple(rec[0]) == (900, 0, 32768, 0)
        assert np.array_equal(st[0, :2 * D], x[-2 * D:].astype(np.int32)) and (st[0, 2 * D:3 * D] == 32768).all() and (st[0, 3 * D:] == 1 << 23).all()


@pytest.mark.parametrize("lw", LWS)
def test_cut_invariance_over_ragged_cuts(pkg, lw):
    """any cut of a row into calls, 0-length and sub-D pieces included, gives the row's PCM, state and joined records"""
    rng = np.random.default_rng(43)
    n = sum(ref.CUTS)
    x = ref.random_full_range(rng, 2 * n)
    for corner in ref.CORNERS:
        par = _params(corner)
        whole = pkg.pcm_limit_host(x, lw, 1, 0, par)
        assert _same(pkg, whole, ref.process(x, lw, 1, 0, par)), (lw, corner)
        st, rec, at, outs = None, None, 0, []
        for c in ref.CUTS:
            o, st, rec = pkg.pcm_limit_host(x[2 * at:2 * (at + c)], lw, 1, 0, par, st, rec)
            outs.append(o)
            at += c
        assert np.array_equal(np.concatenate(outs), whole[0]) and np.array_equal(st, whole[1]) and rec.tobytes() == whole[2].tobytes(), (lw, corner)


def test_a_gain_ramp_across_calls_is_the_ramp_one_pair_at_a_time(pkg):
    """the ramp is a closed form of (gain0, gain_t, slew, J): three calls that carry J, the second behind a rebase, against the reference fed the
    gain of every pair by stepping towards the target by at most slew per pair"""
    rng = np.random.default_rng(44)
    lw, slew, C, delta = 3, 7, 20000, 3000
    x = ref.random_full_range(rng, 2 * 1500)
    cuts, targets = (400, 500, 600), (4096, 9000, 1000)
    # every pair's gain, iterated
    G, g = [], 4096
    for c, tgt in zip(cuts, targets):
        for _ in range(c):
            g += max(-slew, min(slew, tgt - g))
            G.append(g)
    # the reference with a per-pair gain: slew 65536 jumps to gain_t at once, so each pair is a call of its own
    st_r, rec_r, want = None, (0, 0, 32768, 0), []
    for i in range(1500):
        y, st_r, r, _ = ref.process(x[2 * i:2 * i + 2], lw, 32768, 65536, (C, delta, G[i], G[i]), st_r)
        rec_r = ref.join(rec_r, r)
        want.append(y)
    # the library: gain0 is where the ramp has got to when the target changes, J restarts
    st, rec, at, g0, outs = None, None, 0, 4096, []
    for c, tgt in zip(cuts, targets):
        half = c // 2
        for J, m in ((0, half), (half, c - half)):                          # two calls per target: the second carries J
            o, st, rec = pkg.pcm_limit_host(x[2 * at:2 * (at + m)], lw, slew, J, (C, delta, g0, tgt), st, rec)
            outs.append(o)
            at += m
        g0 = int(ref.ramp(g0, tgt, slew, c))
        assert g0 == G[at - 1]
    assert np.array_equal(np.concatenate(outs), np.concatenate(want)) and np.array_equal(st[0], st_r) and ref.rec_tuple(rec[0]) == rec_r


@pytest.mark.parametrize("lw,delta", [(2, 874), (6, 874), (8, 5000), (3, 1 << 23), (6, 1)])
def test_release_climbs_by_delta_per_pair(pkg, lw, delta):
    """one full-scale pair, then silence: r holds 256 g for D + 1 pairs and then climbs by exactly delta per pair; s is below 32768 for exactly
    2 D + k pairs, k = ceil((2^23 - 256 g) / delta) <= ceil(2^23 / delta), and 32768 from then on"""
    D, C = (1 << lw) - 1, 1000
    g = (C * 32768) // 32767
    k = -((-((1 << 23) - 256 * g)) // delta)
    assert k <= -((-(1 << 23)) // delta)
    par = (C, delta, 4096, 4096)
    head = np.zeros(2 * (D + 1), np.int16)
    head[0] = 32767
    y, st, rec = pkg.pcm_limit_host(head, lw, 1, 0, par)                    # the peak at pair 0 and the D pairs that still see it
    assert (st[0, 3 * D:] == 256 * g).all() and y[2 * D] == (32767 * g + 16384) >> 15 and abs(int(y[2 * D])) <= C
    probe = sorted(set(j for j in (1, 2, 3, D, 2 * D, k - 1, k, k + 1) if 1 <= j <= min(k + 1, 20000)))
    at = 0
    for j in probe:                                                       # j pairs of silence behind the head
        _, st, rec = pkg.pcm_limit_host(np.zeros(2 * (j - at), np.int16), lw, 1, 0, par, st, rec)
        at = j
        assert int(st[0, -1]) == min(1 << 23, 256 * g + j * delta), (lw, delta, j)
    if k <= 20000:
        _, st, rec = pkg.pcm_limit_host(np.zeros(2 * (k + D - at), np.int16), lw, 1, 0, par, st, rec)
        assert ref.rec_tuple(rec[0]) == (D + 1 + k + D, 2 * D + k, g, D)   # the smoothed gain reaches g exactly when the peak comes out
        _, st, after = pkg.pcm_limit_host(np.zeros(2 * 50, np.int16), lw, 1, 0, par, st)
        assert ref.rec_tuple(after[0]) == (50, 0, 32768, 0)
        assert -((-(1 << 23)) // delta) + 2 * D >= 2 * D + k


def test_in_place_on_the_host(pkg):
    """out may be in: the C routine called with out == in gives what it gives out of place"""
    import ctypes as C
    lib = pkg.load_library()
    rng = np.random.default_rng(45)
    x = ref.random_full_range(rng, 2 * 2500)
    par = np.array([(9000, 400, 4096, 30000)], dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
    want = pkg.pcm_limit_host(x, 6, 3, 10, par)
    buf, st, rec = x.copy(), pkg.limit.limit_state_init(6), pkg.limit.limit_identity()
    assert lib.sdrfm_pcm_limit_s16(buf.ctypes.data, 2500, 6, 3, 10, par.ctypes.data, st.ctypes.data, buf.ctypes.data, rec.ctypes.data) == 0
    assert np.array_equal(buf, want[0]) and np.array_equal(st, want[1]) and rec.tobytes() == want[2].tobytes()
    assert C.sizeof(pkg.lib.PcmLimitRec) == 32
