"""The look-ahead PCM limiter's true-peak form on the CPU.  Two programs of their own, built with ASan and UBSan and run as
programs: tests/native/limit_tp_check.cpp holds the lane's sums over the packed table of csrc/sdrfm_limit.h to the definition's at the extremes,
tests/native/limit_tp_sanity.c walks the plain-C host side (csrc/limit_tp.c) over its edges.  Then the C routine through the library against
tests/limit_tp_ref.py (the int64 numpy restatement of the definition).  Every comparison is integer equality of PCM, all 4 D + NT state words and
all four record fields, except the programme table of property 6, which compares two measured readings with each other."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import limit_tp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LWS = [2, 3, 6, 8]
TABLES = ["default", (8, 4), (2, 64)]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_arithmetic_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "limit_tp_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/limit_tp_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "limit_tp_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/limit_tp_sanity.c", "stm32f7-rtlsdr_amd/csrc/limit_tp.c", "stm32f7-rtlsdr_amd/csrc/limit.c",
                                           "stm32f7-rtlsdr_amd/csrc/truepeak.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan", "-I" + os.path.join(ROOT, "include")] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _coef(pkg, table):
    """(what the library is given, what the reference is given)"""
    if table == "default":
        assert np.array_equal(pkg.truepeak_default_coef(), ref.BS1770)       # the reference typed the Recommendation's table in on its own
        return None, ref.BS1770
    c = pkg.truepeak_coef(*table)
    return c, c


def _params(corner):
    C, G, delta = corner
    return (C, delta, G, G)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1][0], want[1]) and ref.rec_tuple(got[2][0]) == want[2]


def _combos():
    return [(lw, t) for lw in LWS for t in TABLES if (1 << lw) >= (12 if t == "default" else t[1]) // 2]


def test_the_combinations_cover_every_window_and_table():
    assert _combos() == [(2, (8, 4)), (3, "default"), (3, (8, 4)), (6, "default"), (6, (8, 4)), (6, (2, 64)), (8, "default"), (8, (8, 4)), (8, (2, 64))]


@pytest.mark.parametrize("lw,table", _combos())
@pytest.mark.parametrize("corner", ref.CORNERS)
def test_c_routine_is_the_definition_and_the_ceiling_holds(pkg, lw, table, corner):
    rng = np.random.default_rng(61)
    par = _params(corner)
    lib_c, ref_c = _coef(pkg, table)
    x = ref.random_full_range(rng, 2 * 700)
    got, want = pkg.pcm_limit_tp_host(x, lw, 1, 0, par, coef=lib_c), ref.process(x, lw, 1, 0, par, coef=ref_c)
    assert _same(got, want), (lw, table, corner)
    assert int(np.abs(got[0].astype(np.int64)).max()) <= corner[0]                       # property 1
    got2 = pkg.pcm_limit_tp_host(x[:600], lw, 1, 0, par, got[1], got[2], coef=lib_c)     # from a carried state, joined onto the first record
    want2 = ref.process(x[:600], lw, 1, 0, par, want[1], coef=ref_c)
    assert np.array_equal(got2[0], want2[0]) and np.array_equal(got2[1][0], want2[1]) and ref.rec_tuple(got2[2][0]) == ref.join(want[2], want2[2])
    assert int(np.abs(got2[0].astype(np.int64)).max()) <= corner[0]
    if corner[1] == 0:
        assert not got[0].any() and want[2][1] == 0                                      # a gain of 0: silence, nothing limited


@pytest.mark.parametrize("lw,nt", [(2, 12), (2, 64), (4, 64), (3, 20), (1, 4), (9, 4)])
def test_a_window_shorter_than_half_a_row_is_refused(pkg, lw, nt):
    x = np.zeros(16, np.int16)
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_limit_tp_host(x, lw, coef=pkg.truepeak_coef(2, nt))
    assert e.value.status == pkg.lib.EINVAL
    assert pkg.load_library().sdrfm_pcm_tplimit_state_words(lw, nt) == 0 and pkg.load_library().sdrfm_pcm_tplimit_latency(lw, nt) == 0


@pytest.mark.parametrize("lw,table", _combos())
def test_transparency(pkg, lw, table):
    """property 2.  G = 4096, no |x| over C and no T over C 2^15: y[u] = x[u - D - H] bit for bit, nothing limited.  The rows are full-range noise
    scaled down until the REFERENCE's T says the premise holds (and comes within a fifth of breaking it)"""
    lib_c, ref_c = _coef(pkg, table)
    NT = ref_c.shape[1]
    D, H = (1 << lw) - 1, NT // 2
    rng = np.random.default_rng(62)
    for C in (29204, 1000, 32767):
        x = rng.integers(-C, C + 1, size=2 * 900, dtype=np.int64)
        T = ref.process(np.clip(x, -32768, 32767).astype(np.int16), lw, 1, 0, (32767, 874, 4096, 4096), coef=ref_c)[4]
        x = (x * (C << 15) // (max(int(T.max()), C << 15) * 102 // 100)).astype(np.int16)   # 2 % of room for the rounding of the samples
        par = (C, 874, 4096, 4096)
        T = ref.process(x, lw, 1, 0, par, coef=ref_c)[4]
        assert int(T.max()) <= C << 15 and int(np.abs(x.astype(np.int64)).max()) <= C and int(T.max()) > (C << 15) * 0.8
        y, st, rec = pkg.pcm_limit_tp_host(x, lw, 1, 0, par, coef=lib_c)
        L = D + H
        assert np.array_equal(y[2 * L:], x[:-2 * L]) and not y[:2 * L].any(), (lw, table, C)
        assert ref.rec_tuple(rec[0]) == (900, 0, 32768, 0)
        assert np.array_equal(st[0, :2 * L], x[-2 * L:].astype(np.int32)) and (st[0, 2 * L:2 * L + D] == 32768).all() and (st[0, 2 * L + D:] == 1 << 23).all()


def test_the_detector_sees_between_the_samples(pkg):
    """a quarter-rate tone at 45 degrees whose samples all lie under C: the sample form passes it bit for bit, the true-peak form reduces it"""
    C, lw = 26028, 6
    t = np.arange(3000)
    tone = np.rint(32000 * np.sin(np.pi * t / 2 + np.pi / 4)).astype(np.int16)
    x = np.stack([tone, tone], axis=1).reshape(-1)
    assert int(np.abs(tone).max()) < C < 32000
    par = (C, 874, 4096, 4096)
    assert ref.rec_tuple(pkg.pcm_limit_host(x, lw, 1, 0, par)[2][0]) == (3000, 0, 32768, 0)
    y, _, rec = pkg.pcm_limit_tp_host(x, lw, 1, 0, par)
    assert int(rec["limited"][0]) > 2800 and int(rec["min_gain"][0]) < 32768 * 0.83


@pytest.mark.parametrize("lw", [3, 6, 8])
def test_true_peak_bound_at_constant_gain(pkg, lw):
    """property 5: once s is one value over a value's support, |A_y| <= C 2^15 + floor(max_p sum_k |coef[p][k]| / 2) in the meter's units.  A
    quarter-rate tone at 45 degrees with its samples under C and its true peak over it reaches a constant s within 4 D + 40 pairs."""
    C, n = 26028, 4 * 255 + 40 + 1500
    D, H, NT = (1 << lw) - 1, 6, 12
    t = np.arange(n)
    tone = np.rint(32000 * np.sin(np.pi * t / 2 + np.pi / 4)).astype(np.int16)
    x = np.stack([tone, -tone], axis=1).reshape(-1)
    par = (C, 874, 4096, 4096)
    y, _, _, s, T = ref.process(x, lw, 1, 0, par)
    assert np.array_equal(pkg.pcm_limit_tp_host(x, lw, 1, 0, par)[0], y)
    start = 4 * D + 40
    assert int(T.max()) > C << 15 and int(np.abs(x.astype(np.int64)).max()) < C
    assert (s[start:] == s[start]).all() and s[start] < 32768
    yy = y.astype(np.int64).reshape(-1, 2)
    A = ref.peaks(yy, ref.BS1770, start + NT, n - start - NT)             # every value whose support lies where s is constant
    bound = (C << 15) + int(np.abs(ref.BS1770).sum(axis=1).max()) // 2
    assert bound == 852918646
    print("lw %d: the output's true peak at constant gain %d <= %d" % (lw, int(A.max()), bound))
    assert int(A.max()) <= bound
    assert int(A.max()) > (C << 15) * 0.99                                 # and the limiter does not give the level away either


def test_programme_material_overshoots_less_than_under_the_sample_form(pkg, capsys):
    """property 6, measured and not bounded: on each seeded fixture, under the same ceiling (-2 dB) and make-up gain (x 4), the true-peak form's
    output reads less over the ceiling on sdrfm_pcm_truepeak_s16 than the sample form's.  The table is DESIGN.md §4.25's."""
    C = pkg.limit_ceiling(-2.0)
    par = (C, 874, 16384, 16384)
    rows = []
    for lw in (3, 6):
        for name, x in ref.fixtures().items():
            read = []
            for host in (pkg.pcm_limit_host, pkg.pcm_limit_tp_host):
                y = host(x, lw, 1, 0, par)[0]
                rec = pkg.pcm_truepeak_host(y)[0]
                peak = int(max(rec["peak_l"][0], rec["peak_r"][0]))
                assert peak == ref.true_peak(y)
                read.append(peak)
            rows.append((lw, name, read[0], read[1]))
    with capsys.disabled():
        for lw, name, a, b in rows:
            print("\n  LW %d %-10s sample form %+.3f dBTP, true-peak form %+.3f dBTP (ceiling %+.3f)" % (
                lw, name, 20 * np.log10(a / 2.0 ** 30), 20 * np.log10(b / 2.0 ** 30), 20 * np.log10(C / 32768.0)), end="")
    for lw, name, a, b in rows:
        assert max(0, b - (C << 15)) < max(0, a - (C << 15)), (lw, name, a, b)


@pytest.mark.parametrize("lw,table", _combos())
def test_cut_invariance_over_ragged_cuts_and_every_short_length(pkg, lw, table):
    """property 3: limit_ref.CUTS, then a cut at every length from 0 to D + H + 1 — PCM, state and joined records against one call"""
    lib_c, ref_c = _coef(pkg, table)
    L = (1 << lw) - 1 + ref_c.shape[1] // 2
    rng = np.random.default_rng(63)
    short = list(range(L + 2)) if L <= 40 else [0, 1, 2, L - 1, L, L + 1] + list(range(3, L - 1, 7))
    for cuts in (ref.CUTS, short + [50]):
        n = sum(cuts)
        x = ref.random_full_range(rng, 2 * n)
        for corner in ref.CORNERS[:2] if cuts is not ref.CUTS else ref.CORNERS:
            par = _params(corner)
            whole = pkg.pcm_limit_tp_host(x, lw, 1, 0, par, coef=lib_c)
            if cuts is ref.CUTS:
                assert _same(whole, ref.process(x, lw, 1, 0, par, coef=ref_c)), (lw, table, corner)
            st, rec, at, outs = None, None, 0, []
            for c in cuts:
                o, st, rec = pkg.pcm_limit_tp_host(x[2 * at:2 * (at + c)], lw, 1, 0, par, st, rec, coef=lib_c)
                outs.append(o)
                at += c
            assert np.array_equal(np.concatenate(outs), whole[0]) and np.array_equal(st, whole[1]) and rec.tobytes() == whole[2].tobytes(), (lw, table, corner)


def test_every_short_length_at_the_widest_window(pkg):
    """the cut at EVERY length from 0 to D + H + 1 where the sweep above thins them out: LW = 8 with 64 taps, D + H = 287"""
    lw, c = 8, pkg.truepeak_coef(2, 64)
    cuts = list(range(287 + 2))
    x = ref.random_full_range(np.random.default_rng(64), 2 * sum(cuts))
    par = (9000, 2000, 4096, 30000)
    whole = pkg.pcm_limit_tp_host(x, lw, 1, 0, (9000, 2000, 30000, 30000), coef=c)
    st, rec, at, outs = None, None, 0, []
    for n in cuts:
        o, st, rec = pkg.pcm_limit_tp_host(x[2 * at:2 * (at + n)], lw, 32768, 65536, par, st, rec, coef=c)     # J saturated: the ramp has ended
        outs.append(o)
        at += n
    assert np.array_equal(np.concatenate(outs), whole[0]) and np.array_equal(st, whole[1]) and rec.tobytes() == whole[2].tobytes()


def test_a_gain_ramp_across_calls(pkg):
    """steps 1's ramp is the sample form's closed form of (gain0, gain_t, slew, J): two calls that carry J against the reference's ramp"""
    rng = np.random.default_rng(65)
    lw, slew, par = 3, 7, (20000, 3000, 4096, 9000)
    x = ref.random_full_range(rng, 2 * 1500)
    o1, st, rec = pkg.pcm_limit_tp_host(x[:800], lw, slew, 0, par)
    o2, st, rec = pkg.pcm_limit_tp_host(x[800:], lw, slew, 400, par, st, rec)
    w1 = ref.process(x[:800], lw, slew, 0, par)
    w2 = ref.process(x[800:], lw, slew, 400, par, w1[1])
    assert np.array_equal(o1, w1[0]) and np.array_equal(o2, w2[0]) and np.array_equal(st[0], w2[1]) and ref.rec_tuple(rec[0]) == ref.join(w1[2], w2[2])


def test_in_place_on_the_host(pkg):
    """out may be in: the C routine called with out == in gives what it gives out of place"""
    lib = pkg.load_library()
    rng = np.random.default_rng(66)
    x = ref.random_full_range(rng, 2 * 2500)
    par = np.array([(9000, 400, 4096, 30000)], dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
    want = pkg.pcm_limit_tp_host(x, 6, 3, 10, par)
    buf, st, rec = x.copy(), pkg.limit.limit_tp_state_init(6), pkg.limit.limit_identity()
    assert lib.sdrfm_pcm_tplimit_s16(buf.ctypes.data, 2500, 6, 3, 10, par.ctypes.data, None, 0, 0, st.ctypes.data, buf.ctypes.data, rec.ctypes.data) == 0
    assert np.array_equal(buf, want[0]) and np.array_equal(st, want[1]) and rec.tobytes() == want[2].tobytes()


@pytest.mark.parametrize("lw", [3, 6, 8])
def test_where_the_waveform_never_passes_its_samples_it_is_the_sample_form_delayed_by_h(pkg, lw):
    """From a state whose interpolator history is zero, on an input whose T never decides — ceil(T / 2^15) <= max(the detector pair's sample
    magnitude, C) at every pair, checked on the reference's T — the outputs, g and r are sdrfm_pcm_limit_s16's on the same row behind H pairs of
    silence.  A constant row under the default table is such an input once its onset lies under the ceiling (the rows sum to at most 32820, their
    partial sums to 1.12 times 32768); the g and r words are taken from a stream that a loud passage has left limiting, so that the release runs."""
    D, H = (1 << lw) - 1, 6
    C, level = 20000, 17000
    par = (C, 300, 4096, 4096)
    assert int(ref.BS1770.sum(axis=1).max()) == 32820 and 32820 * level <= C << 15                   # the steady state reads 1.0016 of the level
    loud = np.full(2 * 400, 32767, np.int16)
    _, s_state, _ = pkg.pcm_limit_host(np.concatenate([loud, np.zeros(2 * D, np.int16)]), lw, 1, 0, par)   # x' history zero again, g and r still low
    assert not s_state[0, :2 * D].any() and int(s_state[0, -1]) < 1 << 23
    t_state = np.concatenate([np.zeros(2 * (D + H), np.int32), s_state[0, 2 * D:]])[None, :]
    x = np.empty(2 * 1200, np.int16)
    x[0::2], x[1::2] = level, -level
    y, st, rec, _, T = ref.process(x, lw, 1, 0, par, t_state[0])
    xs = np.abs(np.concatenate([np.zeros(2 * H, np.int64), x.astype(np.int64)]).reshape(-1, 2)).max(axis=1)[:1200]
    assert (((T + 32767) >> 15) <= np.maximum(xs, C)).all() and int(T.max()) > level << 15             # the premise, and the onset does overshoot the level
    got = pkg.pcm_limit_tp_host(x, lw, 1, 0, par, t_state)
    assert np.array_equal(got[0], y) and np.array_equal(got[1][0], st)
    delayed = np.concatenate([np.zeros(2 * H, np.int16), x])[:2 * 1200]
    want = pkg.pcm_limit_host(delayed, lw, 1, 0, par, s_state)
    assert np.array_equal(got[0], want[0]) and got[2].tobytes() == want[2].tobytes()
    assert np.array_equal(got[1][0, 2 * (D + H):], want[1][0, 2 * D:]) and int(want[2]["limited"][0]) > 100
