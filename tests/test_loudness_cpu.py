"""The loudness meter on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
loudness_check.cpp holds the index functions, the ring rule and the matrix-power table of csrc/sdrfm_loudness.h to naive loops,
tests/native/loudness_sanity.c walks the plain-C host side (csrc/loudness.c) over its edges.  Then the C routine through the library against
scipy.signal.lfilter (tests/loudness_ref.py), the gate on the EBU Tech 3341 and Tech 3342 programmes against the values the documents ask
for and against exact list gating, additivity over ragged cuts, and LoudnessMonitor and loudness_alarms."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import loudness_cases as lc
import loudness_ref as ref

ROOT = lc.ROOT
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("reduced", [True, False], ids=["reduced-tile", "library-geometry"])
def test_run_header_clean_under_asan_and_ubsan(tmp_path, reduced):
    exe = str(tmp_path / "loudness_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + (["-DLOUDNESS_CHECK_REDUCED"] if reduced else []) + [
        "-o", exe, os.path.join(ROOT, "tests/native/loudness_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "loudness_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/loudness_sanity.c", "stm32f7-rtlsdr_amd/csrc/loudness.c")]
    cmd = ["gcc", "-std=c99", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def test_c_routine_against_scipy(pkg):
    """the same two biquads through scipy.signal.lfilter; its evaluation order is its own, so loud sub-blocks to 1e-9 and the rest to the
    absolute term"""
    coef = pkg.loudness_default_coef()
    assert np.array_equal(coef, ref.K48)
    for n, bl in ((4800, 64), (9745, 100), (48000, 4800)):
        pcm = lc.interleave(*lc.random_rows(n, 2))
        got, st = pkg.pcm_loudness_host(pcm, bl, coef)
        assert got.shape == (2, n // bl, 2) and (st["pos"] == n).all()
        for s in range(2):
            want = ref.energies(pcm[s], bl)
            assert np.all(np.abs(got[s] - want) <= 1e-9 * want + 1e-3 * bl), (n, bl, s)
    tone = lc.programme([(1.0, -23)])
    got, _ = pkg.pcm_loudness_host(tone, 4800, coef)
    assert np.allclose(got[0], ref.energies(tone, 4800), rtol=1e-9, atol=0)


def _gate(pkg, pcm, bl=4800):
    e, _ = pkg.pcm_loudness_host(pcm, bl)
    with pkg.LoudnessGate(bl) as g:
        for a in range(0, e.shape[1], 7):                                                   # pushed in pieces: the gate's state carries
            g.push(e[0, a:a + 7])
        return g.report(), ref.gate_list(e[0], bl)


@pytest.mark.parametrize("case", sorted(lc.TECH_3341))
def test_integrated_loudness_ebu_tech_3341(pkg, case):
    segments, want = lc.TECH_3341[case]
    rep, lst = _gate(pkg, lc.programme(segments))
    print("case %d: integrated %.3f (list gating %.3f), M %.3f, S %.3f" % (case, rep["i"], lst["i"], rep["m"], rep["s"]))
    assert abs(rep["i"] - want) <= 0.1, (case, rep)
    assert abs(lst["i"] - lc.LIST_I[case]) <= 0.0015 and abs(rep["i"] - lst["i"]) <= 2 * lc.GATE_I_DIFF
    assert rep["n_gating"] == lst["n_gating"] and rep["n_abs"] == lst["n_abs"]
    if case == 1:
        assert abs(rep["m"] - want) <= 0.1 and abs(rep["s"] - want) <= 0.1 and abs(rep["max_m"] - want) <= 0.1 and abs(rep["max_s"] - want) <= 0.1
    if case == 4:
        assert rep["n_abs"] < rep["n_gating"]                                                # the -72 dBFS ends fall to the absolute gate


@pytest.mark.parametrize("case", sorted(lc.TECH_3342))
def test_loudness_range_ebu_tech_3342(pkg, case):
    segments, want = lc.TECH_3342[case]
    rep, lst = _gate(pkg, lc.programme(segments))
    print("case %d: LRA %.3f (list gating %.3f)" % (case, rep["lra"], lst["lra"]))
    assert abs(rep["lra"] - want) <= 1.0, (case, rep)
    assert abs(lst["lra"] - lc.LIST_LRA[case]) <= 0.006 and abs(rep["lra"] - lst["lra"]) <= 2 * lc.GATE_LRA_DIFF


def test_histogram_gate_against_list_gating(pkg):
    """the largest difference between the 0.1 LU histograms and exact list gating, over the EBU programmes and a random programme: recorded in
    tests/loudness_cases.py, asserted with a margin of 2, and far inside what the specifications allow"""
    di = dl = 0.0
    progs = [lc.programme(seg) for seg, _ in list(lc.TECH_3341.values()) + list(lc.TECH_3342.values())] + [lc.random_programme()]
    for pcm in progs:
        rep, lst = _gate(pkg, pcm)
        di, dl = max(di, abs(rep["i"] - lst["i"])), max(dl, abs(rep["lra"] - lst["lra"]))
        assert abs(rep["m"] - lst["m"]) <= 1e-9 and abs(rep["s"] - lst["s"]) <= 1e-9
        assert rep["n_rel"] >= lst["n_rel"]                                                  # the bin that holds the gate is kept whole
    print("histogram against list gating: integrated %.4f LU, range %.4f LU" % (di, dl))
    assert di <= 2 * lc.GATE_I_DIFF and dl <= 2 * lc.GATE_LRA_DIFF
    assert di >= lc.GATE_I_DIFF / 2 and dl >= lc.GATE_LRA_DIFF / 2                           # measurements, not guesses
    assert 2 * lc.GATE_I_DIFF < 0.1 and 2 * lc.GATE_LRA_DIFF < 1.0


def test_additivity_over_ragged_cuts(pkg):
    """any cut of a row into calls gives the row's sub-blocks: indices and counts exactly, energies to the device's tolerance (the host
    routine walks the same operations whatever the cut, so in fact to the bit)"""
    rng = np.random.default_rng(12)
    n, bl = 1500, 100
    pcm = lc.interleave(*lc.random_rows(n, 1))[0]
    whole, st_whole = pkg.pcm_loudness_host(pcm, bl)
    for t in range(12):
        cuts = sorted([0, n] + [int(c) for c in rng.integers(0, n + 1, int(rng.integers(1, 9)))] + [99, 100, 101][:t % 4])
        st, got = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            e, st = pkg.pcm_loudness_host(pcm[2 * a:2 * b], bl, state=st)
            assert e.shape[1] == b // bl - a // bl and int(st["pos"][0]) == b               # exactly
            got.append(e)
        got = np.concatenate(got, axis=1)
        ok, why = lc.within(got, whole, bl)
        assert ok and got.tobytes() == whole.tobytes() and st.tobytes() == st_whole.tobytes(), (cuts, why)


def test_monitor_reports_a_gap_and_alarms(pkg):
    tone = lc.programme([(8.0, -23)])
    e, _ = pkg.pcm_loudness_host(np.stack([tone, tone // 4]), 4800)
    mon = pkg.LoudnessMonitor(2, 4800)
    assert mon.push(0, e[:, :40]) == 0 and mon.push(40, e[:, 40:40]) == 0 and mon.push(40, e[:, 40:50]) == 0
    s = mon.summary()
    assert [x["n_blocks"] for x in s] == [50, 50] and s[0]["gaps"] == 0 and abs(s[0]["i"] + 23.0) <= 0.1 and abs(s[1]["i"] + 35.0) <= 0.2
    assert abs(s[0]["s"] + 23.0) <= 0.1 and s[0]["lra"] <= 0.1
    assert pkg.loudness_alarms(s) == [dict(too_loud=False, too_quiet=False, gap=False), dict(too_loud=False, too_quiet=True, gap=False)]
    assert pkg.loudness_alarms(s, target=-30.0, tol=2.0)[0] == dict(too_loud=True, too_quiet=False, gap=False)
    assert mon.push(60, e[:, 60:80]) == 10                                                   # ten sub-blocks lost: reported, the windows start over
    s = mon.summary()
    assert s[0]["gaps"] == 1 and s[0]["lost"] == 10 and s[0]["n_blocks"] == 20 and np.isnan(s[0]["s"])
    assert pkg.loudness_alarms(s)[0]["gap"] and pkg.loudness_alarms(s)[0]["too_loud"] is False
    fresh = pkg.LoudnessMonitor(1, 4800)
    assert pkg.loudness_alarms(fresh.summary()) == [dict(too_loud=False, too_quiet=False, gap=False)]   # NaN raises nothing
    fresh.push(0, np.zeros((1, 10, 2)))
    assert fresh.summary()[0]["i"] == -np.inf and pkg.loudness_alarms(fresh.summary())[0]["too_quiet"]
    assert pkg.loudness.LOUDNESS_TOL == 1.0
    mon.close()
    fresh.close()
