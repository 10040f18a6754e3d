"""The audio meter on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
audio_meter_check.cpp holds the mask-to-runs function and the joins of csrc/sdrfm_audio_meter.h to naive loops, tests/native/audio_meter_sanity.c
walks the plain-C host side (csrc/audio_meter.c) over its edges.  Then the C routine, the join and the report through the library against
tests/audio_meter_ref.py (the numpy restatement the GPU tests use) and float64 numpy, the case generator through the host de-emphasis
routine, and audio_alarms on five synthetic programmes.  Every record comparison is integer equality of all fields."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import audio_meter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_run_header_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "audio_meter_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/audio_meter_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "audio_meter_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/audio_meter_sanity.c", "stm32f7-rtlsdr_amd/csrc/audio_meter.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def test_dtype_is_the_reference_layout(pkg):
    assert pkg.AUDIO_METER_DTYPE == ref.DTYPE and pkg.AUDIO_METER_DTYPE.itemsize == 192
    assert [pkg.AUDIO_METER_DTYPE.fields[n][1] for n in ref.DTYPE.names] == [ref.DTYPE.fields[n][1] for n in ref.DTYPE.names]


def test_reference_runs_against_a_loop():
    rng = np.random.default_rng(3)
    for t in range(400):
        q = rng.random(int(rng.integers(0, 90))) < (0.0, 0.2, 0.5, 0.9, 1.0)[t % 5]
        count = lead = trail = longest = run = 0
        alive = True
        for v in q:
            if v:
                count, run = count + 1, run + 1
                lead = run if alive else lead
                longest = max(longest, run)
            else:
                run, alive = 0, False
        trail = run
        assert ref.runs(q) == (count, lead, trail, longest), q


def _cases():
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 2, 63, 64, 65, 257, 4801):
        L, R = ref.random_full_range(rng, 2, n)
        out += [(ref.interleave(L, R)[s], q) for s in range(2) for q in (0, 3, 32767)]
    n = 300
    out.append((ref.interleave(np.full(n, -32768), np.full(n, 32767)), 32767))          # the rails
    out.append((ref.interleave(np.full(n, -32768), np.full(n, 32767)), 0))
    out.append((np.zeros(2 * n, np.int16), 0))                                              # all quiet
    out.append((ref.interleave(np.full(n, 5), np.full(n, -5)), 5))                          # all quiet at the threshold
    out.append((ref.interleave(np.full(n, 6), np.full(n, -6)), 5))                          # all loud one above it
    out.append((np.zeros(0, np.int16), 7))                                                  # n = 0
    return out


def test_c_routine_is_the_definition(pkg):
    for pcm, q in _cases():
        got = pkg.pcm_audio_meter_host(pcm, q)
        want = ref.records(pcm[None, :], q)
        assert ref.same(got, want), (pcm.size // 2, q, ref.diff(got, want))
    zero = np.zeros(1, pkg.AUDIO_METER_DTYPE)
    assert ref.same(pkg.pcm_audio_meter_host(np.zeros(0, np.int16), 7), zero)


def test_additivity_over_ragged_cuts(pkg):
    """any cut of a row into calls, cuts inside a run included, gives the row's record: through the C routine's acc, through
    sdrfm_audio_meter_add of per-piece records, and through the reference's own join"""
    rng = np.random.default_rng(12)
    L, R = ref.random_full_range(rng, 1, 1500)
    L[0, 400:900] = 0                                                                       # one long run on L for the cuts to fall into
    R[0, 700:1100] = 1
    pcm = ref.interleave(L, R)[0]
    for q in (0, 1):
        whole = pkg.pcm_audio_meter_host(pcm, q)
        assert ref.same(whole, ref.records(pcm[None, :], q))
        for t in range(12):
            cuts = sorted([0, 1500] + [int(c) for c in rng.integers(0, 1501, int(rng.integers(1, 9)))] + [401, 899, 900][:t % 4])
            acc = np.zeros(1, pkg.AUDIO_METER_DTYPE)
            added = np.zeros(1, pkg.AUDIO_METER_DTYPE)
            joined = np.zeros((), ref.DTYPE)
            for a, b in zip(cuts[:-1], cuts[1:]):
                piece = pcm[2 * a:2 * b]
                acc = pkg.pcm_audio_meter_host(piece, q, acc=acc)
                pkg.audio_meter_add(added, pkg.pcm_audio_meter_host(piece, q))
                joined = ref.join(joined, ref.record(piece, q))
            assert ref.same(acc, whole) and ref.same(added, whole) and ref.same(joined.reshape(1), whole), (q, cuts, ref.diff(acc, whole))


def test_add_on_hand_made_records(pkg):
    a, b = np.zeros(1, pkg.AUDIO_METER_DTYPE), np.zeros(1, pkg.AUDIO_METER_DTYPE)
    a["n"], b["n"] = 1 << 31, (1 << 31) - 5
    a["sum_l"], b["sum_l"] = -(1 << 46), 12345
    a["sq_l"], b["sq_l"] = 1 << 61, (1 << 61) - 1
    a["sq_r"], b["sq_r"] = (1 << 62) - 7, 7
    a["cross"], b["cross"] = -(1 << 61), -(1 << 61) + 3
    a["peak_l"], b["peak_l"] = 32768, 5
    a["peak_r"], b["peak_r"] = 5, 32767
    a["clip_l"], b["clip_r"] = 9, 11
    a["quiet_l"] = (1 << 31, 1 << 31, 1 << 31, 1 << 31)                                     # all quiet, then a record that starts quiet
    b["quiet_l"] = (100, 40, 0, 50)
    a["quiet_r"] = (1000, 0, 300, 600)
    b["quiet_r"] = (b["n"][0], b["n"][0], b["n"][0], b["n"][0])
    a["quiet_both"] = (10, 3, 4, 5)
    b["quiet_both"] = (20, 6, 7, 8)
    want = ref.join(a[0], b[0])
    assert int(want["quiet_l"]["lead"]) == (1 << 31) + 40 and int(want["quiet_l"]["longest"]) == (1 << 31) + 40 and int(want["quiet_l"]["trail"]) == 0
    assert int(want["quiet_r"]["trail"]) == int(b["n"][0]) + 300 and int(want["quiet_r"]["longest"]) == int(b["n"][0]) + 300 and int(want["quiet_r"]["lead"]) == 0
    assert tuple(want["quiet_both"].tolist()) == (30, 3, 7, 10)
    assert int(want["sq_l"]) == (1 << 62) - 1 and int(want["cross"]) == -(1 << 62) + 3
    got = pkg.audio_meter_add(a.copy(), b)
    assert ref.same(got, want.reshape(1)), ref.diff(got, want.reshape(1))
    other = pkg.audio_meter_add(b.copy(), a)                                                # the join is ordered
    assert not ref.same(other, got) and ref.same(other, ref.join(b[0], a[0]).reshape(1))
    zero = np.zeros(1, pkg.AUDIO_METER_DTYPE)
    assert ref.same(pkg.audio_meter_add(zero.copy(), a), a) and ref.same(pkg.audio_meter_add(a.copy(), zero), a)


def test_report_against_float64_numpy(pkg):
    rng = np.random.default_rng(13)
    fs = 48000.0
    L, R = ref.random_full_range(rng, 3, 2000)
    R[1] = L[1] // 2                                                                        # correlated
    L[2, 1200:] = 0                                                                         # a trailing silence on L
    pcm = ref.interleave(L, R)
    rec = pkg.pcm_audio_meter_host(pcm, 2)
    rep = pkg.audio_meter_report(rec, fs)
    for s in range(3):
        l, r = L[s].astype(np.float64), R[s].astype(np.float64)
        n = l.size
        want = dict(rms_l_dbfs=10 * np.log10((l * l).sum() / n / 32768.0 ** 2), rms_r_dbfs=10 * np.log10((r * r).sum() / n / 32768.0 ** 2),
                    peak_l_dbfs=20 * np.log10(np.abs(l).max() / 32768.0), peak_r_dbfs=20 * np.log10(np.abs(r).max() / 32768.0),
                    dc_l=l.mean(), dc_r=r.mean(), rail_l=np.mean((l == -32768) | (l == 32767)), rail_r=np.mean((r == -32768) | (r == 32767)),
                    quiet_l=np.mean(np.abs(l) <= 2), quiet_r=np.mean(np.abs(r) <= 2), quiet_both=np.mean((np.abs(l) <= 2) & (np.abs(r) <= 2)),
                    correlation=(l * r).sum() / np.sqrt((l * l).sum() * (r * r).sum()),
                    mid_dbfs=10 * np.log10((((l + r) / 2) ** 2).sum() / n / 32768.0 ** 2), side_dbfs=10 * np.log10((((l - r) / 2) ** 2).sum() / n / 32768.0 ** 2))
        want["side_mid_db"] = want["side_dbfs"] - want["mid_dbfs"]
        for k, v in want.items():
            assert abs(rep[k][s] - v) <= 1e-9 * max(1.0, abs(v)), (s, k, rep[k][s], v)     # (float64 evaluation order only)
        for p, key in (("quiet_l", "l"), ("quiet_r", "r"), ("quiet_both", "both")):
            assert rep["longest_%s_s" % key][s] == int(rec[p]["longest"][s]) / fs and rep["trail_%s_s" % key][s] == int(rec[p]["trail"][s]) / fs
    assert rep["trail_l_s"][2] == 800 / fs
    # n = 0: NaN throughout; a silent channel: -inf dB and no correlation; anti-phase: no mid
    empty = pkg.audio_meter_report(np.zeros(1, pkg.AUDIO_METER_DTYPE), fs)
    assert all(np.isnan(v[0]) for v in empty.values())
    lonly = pkg.audio_meter_report(pkg.pcm_audio_meter_host(ref.interleave(np.array([100, -100]), np.array([0, 0])), 0), fs)
    assert lonly["rms_r_dbfs"][0] == -np.inf and lonly["peak_r_dbfs"][0] == -np.inf and np.isnan(lonly["correlation"][0]) and lonly["side_mid_db"][0] == 0.0
    anti = pkg.audio_meter_report(pkg.pcm_audio_meter_host(ref.interleave(np.array([100, -300]), np.array([-100, 300])), 0), fs)
    assert anti["correlation"][0] == -1.0 and anti["mid_dbfs"][0] == -np.inf and anti["side_mid_db"][0] == np.inf
    quiet = pkg.audio_meter_report(pkg.pcm_audio_meter_host(np.zeros(8, np.int16), 0), fs)
    assert np.isnan(quiet["side_mid_db"][0]) and quiet["mid_dbfs"][0] == -np.inf and quiet["trail_both_s"][0] == 4 / fs
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.audio_meter_report(rec, bad)
        assert e.value.status == pkg.lib.EINVAL


def test_case_rows_come_out_as_the_intended_integers(pkg):
    """alpha = 1 and gain = 1: the host routine's chain gives pcm = rint(x), so the case generator's integer-valued rows put their int16 pattern
    into the PCM — what the GPU tests rely on to place exact values"""
    rng = np.random.default_rng(14)
    L, R = ref.random_full_range(rng, 2, 700)
    L[0, :4], R[0, :4] = (-32768, 32767, 0, -1), (32767, -32768, 1, 0)
    for Li, Ri in ((L, R), ref.one_loud_pair(3, 130), ref.one_quiet_pair(3, 130)):
        xl, xr = ref.rows_of(Li, Ri)
        for s in range(xl.shape[0]):
            pcm, state = pkg.pcm_deemph_stereo_s16_host(xl[s], xr[s], ref.ALPHA, ref.GAIN)
            assert np.array_equal(pcm, ref.interleave(Li, Ri)[s]) and state == (float(Li[s, -1]), float(Ri[s, -1]))


def _programme(pkg, left, right, quiet_lsb=3):
    """float audio at 48 kHz through the host de-emphasis routine at 75 us -> the report of its PCM"""
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    pcm, _ = pkg.pcm_deemph_stereo_s16_host(left, right, alpha, 1.0)
    return pkg.audio_meter_report(pkg.pcm_audio_meter_host(pcm, quiet_lsb), 48000.0)


def test_alarms_on_five_synthetic_programmes(pkg):
    """a stereo tone, L only, anti-phase, a tone that stops halfway and full-scale overdrive: each raises exactly its own alarm"""
    t = np.arange(48000) / 48000.0
    a, b = 9000.0 * np.sin(2 * np.pi * 440.0 * t), 9000.0 * np.sin(2 * np.pi * 620.0 * t)
    stop = np.where(t < 0.5, 1.0, 0.0)
    names = ("silent", "left_dead", "right_dead", "out_of_phase", "mono", "clipping")
    cases = [("stereo tone", a, b, []), ("L only", a, 0 * a, ["right_dead"]), ("R only", 0 * a, b, ["left_dead"]), ("anti-phase", a, -a, ["out_of_phase"]),
             ("stops halfway", a * stop, b * stop, ["silent"]), ("overdrive", 40.0 * a, 40.0 * b, ["clipping"]), ("mono", a, a, ["mono"])]
    for name, l, r, want in cases:
        rep = _programme(pkg, l, r)
        got = pkg.audio_alarms(rep, silence_s=0.25)[0]
        assert sorted(got) == sorted(names)
        assert [k for k in names if got[k]] == want, (name, got, {k: v[0] for k, v in rep.items()})
    # the documented defaults: a quarter of a second of silence is no alarm at two seconds
    rep = _programme(pkg, a * stop, b * stop)
    assert not any(pkg.audio_alarms(rep)[0].values())
    assert (pkg.sink.SILENCE_S, pkg.sink.PHASE_CORR, pkg.sink.MONO_SIDE_DB, pkg.sink.CLIP_SHARE) == (2.0, -0.5, -40.0, 1e-4)


def test_monitor_joins_reads_in_order(pkg):
    """a silence that spans three reads is one run in AudioMonitor's summary"""
    L = np.concatenate([np.full(100, 3000), np.zeros(500, np.int64), np.full(50, -3000)])
    pcm = ref.interleave(L, L)
    mon = pkg.AudioMonitor(1, 48000.0)
    for a, b in ((0, 250), (250, 251), (251, 400), (400, 650)):
        mon.push(pkg.pcm_audio_meter_host(pcm[2 * a:2 * b], 0))
    s = mon.summary(silence_s=0.001)[0]
    assert s["n"] == 650 and s["reads"] == 4 and s["longest_both_s"] == 500 / 48000.0 and s["trail_both_s"] == 0.0
    assert ref.same(mon.meters, ref.records(pcm[None, :], 0)) and s["alarms"]["mono"] and not s["alarms"]["silent"]
