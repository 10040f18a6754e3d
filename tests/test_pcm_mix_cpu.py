"""The PCM mix bus on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
pcm_mix_check.cpp walks the launch geometry and the per-pair arithmetic of csrc/sdrfm_pcm_mix.h, tests/native/pcm_mix_sanity.c the plain-C host
side (csrc/pcm_mix.c) over exactly-sized heap rows and its refusals.  Then the C routine through the library against tests/pcm_mix_ref.py (the
definition restated with Python integers): outputs and records by equality over the case table, the identities, both rails, the join's laws, the
report, and the policies around the handle on plain values.  The mutation check holds the case table to two one-line mutants of the reference."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_mix_cases as cases
import pcm_mix_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ONE, NONE, SPAN = cases.ONE, cases.NONE, cases.SPAN
# the C routine against the reference: n around a workgroup's span is the device's concern; here a few n, every shape, with and without the curve
CPU_N = (0, 1, 3, 700)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr
    return r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_and_arithmetic_clean_under_asan_and_ubsan(pkg, tmp_path):
    """every pair of a row exactly once at every n in 0 .. 3 SPAN + 3 and at 2^20; the curve's interpolation against its definition over all 32769
    gains for the linear, the equal-power and the steepest table; the self-crossfade's sum over every slew of the table and n in 0 .. 65537; the
    modes; the 2^34 bound.  The geometry it prints is the Python mirror's."""
    exe = str(tmp_path / "pcm_mix_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/pcm_mix_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    grids = [tuple(int(v) for v in line.split()[1:]) for line in _run(exe).splitlines() if line.startswith("grid ")]
    assert len(grids) >= 10
    for n_bus, n, gx, gy in grids:
        assert pkg.mix.mix_geometry(n_bus, n) == (gx, gy), (n_bus, n)
    assert pkg.mix.SPAN == SPAN == 2048


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pcm_mix_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/pcm_mix_sanity.c", "stm32f7-rtlsdr_amd/csrc/pcm_mix.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _table_cases():
    """(name, rows, slot table, slew, J, curve name) over the case table"""
    for si, (n_in, n_bus, n_slots) in enumerate(cases.SHAPES):
        for ni, n in enumerate(CPU_N):
            for curve in (None, "equal_power"):
                slew = cases.SLEWS[(si + ni) % 3]
                J = (0, 5, 40000, 65536)[(si + ni) % 4]
                yield ("%d-%d-%d n=%d %s" % (n_in, n_bus, n_slots, n, curve), cases.rows(si * 16 + ni, n_in, n),
                       cases.slot_table(si * 16 + ni, n_in, n_bus, n_slots, first_mode=ni), slew, J, curve)
    for mode in range(5):                                              # the one-slot shape sees every mode
        yield ("1-1-1 mode %d" % mode, cases.rows(90 + mode, 1, 50), [[(0, mode, ONE, 12345)]], 7, 0, None)
    for kind in ("rail_lo", "rail_hi"):
        yield ("2-5-8 " + kind, cases.rows(0, 2, 40, kind), cases.slot_table(7, 2, 5, 8), 7, 3, "equal_power")


def _differs(pkg, name, x, table, slew, J, curve, **mutation):
    t = None if curve is None else pkg.mix_curve(curve)
    out, rec = pkg.pcm_mix_host(x, table, slew, J, t)
    want, wrec = ref.mix(x, table, slew, J, t, **mutation)
    return not (np.array_equal(out, want) and [ref.rec_tuple(r) for r in rec] == wrec)


def test_c_routine_is_the_definition(pkg):
    count = 0
    for case in _table_cases():
        assert not _differs(pkg, *case), case[0]
        count += 1
    assert count >= 4 * len(CPU_N) * 2 + 7


def test_case_table_catches_the_two_mutants(pkg):
    """the reference with the ramp evaluated at J + i instead of J + i + 1, and with the rounding constant dropped: each must turn cases red, or
    the table is too weak.  A case whose ramps have all ended (J = 40000 or 65536 in the table) cannot see the first, and a case of no pairs
    neither; the five one-slot cases ramp 32768 -> 12345 by 7 per pair from J = 0 over 50 full-range pairs, so both mutants must show in each."""
    early = [c[0] for c in _table_cases() if _differs(pkg, *c, ramp_at=0)]
    floor = [c[0] for c in _table_cases() if _differs(pkg, *c, rounding=0)]
    print("ramp at J + i:", len(early), early)
    print("no rounding constant:", len(floor), floor)
    for mode in range(5):
        assert "1-1-1 mode %d" % mode in early and "1-1-1 mode %d" % mode in floor, mode
    assert not [name for name in early + floor if " n=0 " in name]


def test_identities(pkg):
    x = cases.rows(3, 2, 3000)
    L, R = x[0, 0::2].astype(np.int64), x[0, 1::2].astype(np.int64)
    # unity: one STEREO slot at 32768 beside slots at 0 and without a source
    out, rec = pkg.pcm_mix_host(x, [[(0, 0, ONE, ONE), (1, 1, 0, 0), (NONE, 3, ONE, ONE)]], 1, 0)
    assert np.array_equal(out[0], x[0]) and ref.rec_tuple(rec[0])[:3] == (3000, 0, 0)
    # the self-crossfade at every slew, at a set's first pair and deep into the ramp; with the linear table and with none
    for slew in cases.IDENTITY_SLEWS:
        for J in (0, 1, ONE // slew, 65535, 65536):
            for curve in (None, pkg.mix_curve("linear")):
                for mode in range(5):
                    out, _ = pkg.pcm_mix_host(x[:, :200], [[(0, mode, ONE, 0), (0, mode, 0, ONE)]], slew, J, curve)
                    want, _ = pkg.pcm_mix_host(x[:, :200], [[(0, mode, ONE, ONE)]], slew, J, curve)
                    assert np.array_equal(out, want), (slew, J, mode)
                    if mode == 0:
                        assert np.array_equal(out[0], x[0, :200])
    # MONO at 32768 is (L + R + 1) >> 1 and never clips, the rails included
    rails = np.array([[-32768, -32768, 32767, 32767, -32768, 32767, 32767, -32768, 32767, 32766]], np.int16)
    for rows_, l, r in ((x[:1], L, R), (rails, rails[0, 0::2].astype(np.int64), rails[0, 1::2].astype(np.int64))):
        out, rec = pkg.pcm_mix_host(rows_, [[(0, 1, ONE, ONE)]], 1, 0)
        assert np.array_equal(out[0, 0::2], (l + r + 1) >> 1) and np.array_equal(out[0, 0::2], out[0, 1::2])
        assert ref.rec_tuple(rec[0])[1:3] == (0, 0)
    # MONO of (a, -a) is 0
    a = cases.rows(4, 1, 500)[0, 0::2].astype(np.int64)
    a = a[a > -32768]
    anti = np.empty((1, 2 * a.size), np.int16)
    anti[0, 0::2], anti[0, 1::2] = a, -a
    out, rec = pkg.pcm_mix_host(anti, [[(0, 1, ONE, ONE)]], 1, 0)
    assert not out.any() and ref.rec_tuple(rec[0]) == (a.size, 0, 0, 0)
    # SWAP of SWAP
    once, _ = pkg.pcm_mix_host(x[:1], [[(0, 4, ONE, ONE)]], 1, 0)
    assert np.array_equal(once[0, 0::2], x[0, 1::2]) and np.array_equal(once[0, 1::2], x[0, 0::2])
    twice, _ = pkg.pcm_mix_host(once, [[(0, 4, ONE, ONE)]], 1, 0)
    assert np.array_equal(twice[0], x[0])
    # LEFT and RIGHT
    left, _ = pkg.pcm_mix_host(x[:1], [[(0, 2, ONE, ONE)], [(0, 3, ONE, ONE)]], 1, 0)
    assert np.array_equal(left[0, 0::2], x[0, 0::2]) and np.array_equal(left[0, 1::2], x[0, 0::2])
    assert np.array_equal(left[1, 0::2], x[0, 1::2]) and np.array_equal(left[1, 1::2], x[0, 1::2])


def test_both_rails(pkg):
    """8 STEREO slots at 32768 on a row of -32768: the sum at its bound 2^34, peak = 2^18 and every output clipped"""
    n = 33
    out, rec = pkg.pcm_mix_host(cases.rows(0, 1, n, "rail_lo"), [[(0, 0, ONE, ONE)] * 8], 1, 0)
    assert (out == -32768).all() and ref.rec_tuple(rec[0]) == (n, n, n, 262144)
    out, rec = pkg.pcm_mix_host(cases.rows(0, 1, n, "rail_hi"), [[(0, 0, ONE, ONE)] * 8], 1, 0)
    assert (out == 32767).all() and ref.rec_tuple(rec[0]) == (n, n, n, 8 * 32767)
    # one channel only: LEFT of (rail, 0) through two slots clips both outputs; STEREO clips the left alone
    x = np.zeros((1, 2 * n), np.int16)
    x[0, 0::2] = 32767
    _, rec = pkg.pcm_mix_host(x, [[(0, 0, ONE, ONE)] * 2], 1, 0)
    assert ref.rec_tuple(rec[0]) == (n, n, 0, 65534)


def test_join_laws_and_cut_invariance(pkg):
    n_in, n_bus, n_slots = 3, 2, 2
    n = SPAN + 2 + 700 + SPAN
    x = cases.rows(11, n_in, n)
    table = cases.slot_table(11, n_in, n_bus, n_slots)
    curve = pkg.mix_curve("equal_power")
    whole, wrec = pkg.pcm_mix_host(x, table, 7, 0, curve)
    acc, at, parts, pieces = np.zeros(n_bus, pkg.MIX_DTYPE), 0, [], []
    for c in cases.cuts(n):
        out, rec = pkg.pcm_mix_host(x[:, 2 * at:2 * (at + c)], table, 7, min(at, 65536), curve)
        parts.append(out)
        pieces.append(rec)
        pkg.mix_add(acc, rec)
        at += c
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and acc.tobytes() == wrec.tobytes()
    a, b, c = pieces[1], pieces[2], pieces[4]
    left = pkg.mix_add(pkg.mix_add(a.copy(), b), c)
    right = pkg.mix_add(a.copy(), pkg.mix_add(b.copy(), c))
    assert left.tobytes() == right.tobytes()                                         # associative
    assert pkg.mix_add(a.copy(), b).tobytes() == pkg.mix_add(b.copy(), a).tobytes()  # commutative
    assert pkg.mix_add(a.copy(), np.zeros(n_bus, pkg.MIX_DTYPE)).tobytes() == a.tobytes()   # the identity
    assert ref.rec_tuple(left[0]) == ref.add(ref.add(ref.rec_tuple(a[0]), ref.rec_tuple(b[0])), ref.rec_tuple(c[0]))
    # the routine accumulates: a second call onto the first's records is the join
    _, r1 = pkg.pcm_mix_host(x[:, :1000], table, 7, 0, curve)
    _, r2 = pkg.pcm_mix_host(x[:, 1000:], table, 7, 500, curve, acc=r1)
    assert r2.tobytes() == wrec.tobytes()


def test_handle_bookkeeping_on_plain_values(pkg):
    """cases.HostMixer, what the GPU tests hold a PcmMixer to: a set_gains towards the targets a ramp already has restarts it where it has got to,
    so the PCM is the uncut ramp's; a jump lands on the target at once; set_routes leaves gains and J alone"""
    x = cases.rows(13, 3, 3000)
    table = cases.slot_table(13, 3, 2, 2)
    src, mode, g0, gt = cases.as_arrays(table)
    plain, cut = cases.HostMixer(pkg, 3, 2, 2, 7), cases.HostMixer(pkg, 3, 2, 2, 7)
    plain.load(table)
    cut.load(table)
    want = plain.process_batch(x)
    got = [cut.process_batch(x[:, :2 * 1234])]
    cut.set_gains(gt)                                                  # the same targets, 1234 pairs into the ramps
    assert cut.J == 0 and np.array_equal(cut.slots["gt"], gt)
    assert [int(v) for v in cut.slots["g0"].reshape(-1)] == [ref.ramp(int(a), int(b), 7, 1234) for a, b in zip(g0.reshape(-1), gt.reshape(-1))]
    got.append(cut.process_batch(x[:, 2 * 1234:]))
    assert np.array_equal(np.concatenate(got, axis=1), want) and cut.rec.tobytes() == plain.rec.tobytes()
    out, _ = ref.mix(x[:, :400], table, 7, 0)
    assert np.array_equal(want[:, :400], out)
    cut.set_routes(mode=3)
    assert cut.J == 3000 - 1234 and np.array_equal(cut.slots["src"], src) and (cut.slots["mode"] == 3).all()
    cut.set_gains(777, jump=True)
    assert (cut.slots["g0"] == 777).all() and (cut.slots["gt"] == 777).all() and cut.J == 0
    with pytest.raises(ValueError):                                    # every slot at 777: none is free
        cut.crossfade(1, 2, "left")


def test_report_and_degenerate_records(pkg):
    rep = pkg.mix_report(np.zeros(2, pkg.MIX_DTYPE))
    assert all(np.isnan(rep[f]).all() for f in ("peak_dbfs", "clipped_frac"))
    rec = np.zeros(3, pkg.MIX_DTYPE)
    rec["n"], rec["clipped_l"], rec["clipped_r"], rec["peak"] = (10, 10, 8), (0, 10, 2), (0, 10, 0), (0, 262144, 16384)
    rep = pkg.mix_report(rec)
    for k in range(3):
        want = ref.report(ref.rec_tuple(rec[k]))
        for f in want:
            assert float(rep[f][k]) == want[f] or abs(float(rep[f][k]) - want[f]) <= 1e-12, (k, f)
    assert rep["peak_dbfs"][0] == -np.inf and rep["clipped_frac"].tolist() == [0.0, 1.0, 0.125]
    assert abs(rep["peak_dbfs"][2] + 20 * math.log10(2)) < 1e-12


def test_refusals_through_python(pkg):
    x = cases.rows(0, 2, 8)
    for bad in ([[(2, 0, ONE, ONE)]], [[(0, 5, ONE, ONE)]], [[(0, 0, ONE + 1, ONE)]], [[(0, 0, ONE, ONE + 1)]], [[(0, 0, 0, 0)] * 9]):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.pcm_mix_host(x, bad)
        assert e.value.status == pkg.lib.EINVAL
    for kw in (dict(slew=0), dict(slew=ONE + 1), dict(J=65537)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.pcm_mix_host(x, [[(0, 0, ONE, ONE)]], **kw)
        assert e.value.status == pkg.lib.EINVAL
    nondecreasing = pkg.mix_curve("linear")
    nondecreasing[64] = 0
    with pytest.raises(pkg.SdrfmError):
        pkg.pcm_mix_host(x, [[(0, 0, ONE, ONE)]], curve=nondecreasing)


def test_curves(pkg):
    for kind in ("equal_power", "linear"):
        t = pkg.mix_curve(kind)
        assert t.dtype == np.uint16 and t.shape == (129,) and int(t[0]) == 0 and int(t[128]) == ONE
        assert (np.diff(t.astype(np.int64)) >= 0).all() and ref.curve_ok(t) and pkg.mix.mix_check_curve(t)
    assert np.array_equal(pkg.mix_curve("linear"), 256 * np.arange(129))
    eq = pkg.mix_curve("equal_power").astype(np.int64)
    assert np.array_equal(eq, [round(32768 * math.sin(math.pi * j / 256)) for j in range(129)]) and eq[64] == 23170
    assert abs(int(eq[64]) ** 2 * 2 - ONE ** 2) < 2 * ONE                            # equal power at the middle
    with pytest.raises(ValueError):
        pkg.mix_curve("cosine")
    for j, v in ((0, 1), (128, 32767), (50, 0)):
        bad = pkg.mix_curve("equal_power")
        bad[j] = v
        assert not pkg.mix.mix_check_curve(bad) and not ref.curve_ok(bad)
    assert not pkg.mix.mix_check_curve(np.zeros(128, np.uint16))
    # the ramp's closed form is the iteration
    for x0, xt, slew in ((0, ONE, 7), (ONE, 0, 7), (100, 30000, 255), (30000, 100, 32768), (5, 5, 1)):
        for n in (0, 1, 2, 100, 4681, 4682, 5000):
            assert ref.ramp(x0, xt, slew, n) == ref.ramp_iterated(x0, xt, slew, n)


def test_slew_and_fade(pkg):
    assert pkg.fade_pairs(1) == 32768 and pkg.fade_pairs(7) == 4682 and pkg.fade_pairs(32768) == 1 and pkg.fade_pairs(32767) == 2
    for bad in (0, 32769, -1):
        with pytest.raises(ValueError):
            pkg.fade_pairs(bad)
    assert pkg.slew_for(0.02) == 34 and pkg.slew_for(0.02, 44100) == 37 and pkg.slew_for(1.0) == 1 and pkg.slew_for(100.0) == 1
    assert pkg.slew_for(0.0) == ONE and pkg.slew_for(-1.0) == ONE and pkg.slew_for(1e-9) == ONE
    for s in (0.001, 0.01, 0.1, 0.5):                                                # the fade lasts what was asked for, within the rounding
        assert abs(pkg.fade_pairs(pkg.slew_for(s)) - s * 48000) <= 0.5 * s * 48000 / pkg.slew_for(s) + 1


def test_dead_channel_modes(pkg):
    def alarm(left=False, right=False, silent=False):
        return dict(silent=silent, left_dead=left, right_dead=right, out_of_phase=False, mono=False, clipping=False)
    got = pkg.dead_channel_modes([alarm(), alarm(left=True), alarm(right=True), alarm(silent=True)])
    assert got.dtype == np.uint32 and got.tolist() == [pkg.mix.STEREO, pkg.mix.RIGHT, pkg.mix.LEFT, pkg.mix.STEREO]
    assert pkg.dead_channel_modes([]).shape == (0,)
    # from the audio meter itself: a stream whose left channel has gone quiet plays its right channel on both sides
    n = 48000
    pcm = np.zeros((2, 2 * n), np.int16)
    tone = np.rint(8000 * np.sin(2 * np.pi * 440 / 48000 * np.arange(n))).astype(np.int16)
    pcm[0, 1::2] = tone
    pcm[1, 0::2] = pcm[1, 1::2] = tone
    alarms = pkg.audio_alarms(pkg.audio_meter_report(pkg.pcm_audio_meter_host(pcm, 8), 48000.0), silence_s=0.5)
    assert pkg.dead_channel_modes(alarms).tolist() == [pkg.mix.RIGHT, pkg.mix.STEREO]


def test_crossfade_plan(pkg):
    plan = pkg.mix.crossfade_plan
    sl = np.zeros((2, 3), pkg.MIX_SLOT_DTYPE)
    sl["src"] = NONE
    k, src, mode, target = plan(sl, 0, 32, 1, 5, "mono")
    assert k == 0 and src[1, 0] == 5 and mode[1, 0] == pkg.mix.MONO and target.tolist() == [[0, 0, 0], [ONE, 0, 0]]
    assert (src[0] == NONE).all() and src[1, 1] == NONE
    # slot 0 playing, slot 1 still fading out (not yet at 0), slot 2 free; bus 0's targets stay
    sl[1, 0] = (5, 1, ONE, ONE)
    sl[1, 1] = (4, 0, ONE, 0)
    sl[0, 2] = (1, 0, 0, 777)
    k, src, mode, target = plan(sl, 100, 32, 1, 2)
    assert k == 2 and src[1].tolist() == [5, 4, 2] and mode[1].tolist() == [1, 0, 0] and target.tolist() == [[0, 0, 777], [0, 0, ONE]]
    # ... and once that fade has ended slot 1 is the first free one
    k, _, _, _ = plan(sl, 1024, 32, 1, 2)
    assert k == 1
    # no free slot: every one in use or still fading
    sl[1, 2] = (2, 0, 0, ONE)
    with pytest.raises(ValueError):
        plan(sl, 100, 32, 1, 3)
    with pytest.raises(ValueError):
        plan(sl, 0, 32, 2, 3)
    with pytest.raises(ValueError):
        plan(sl[:1], 0, 32, 0, 3, "sideways")
