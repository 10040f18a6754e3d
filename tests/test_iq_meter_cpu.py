"""The raw-capture IQ meter on the CPU.  Two programs of their own, built with ASan and UBSan and run as programs: tests/native/
iq_meter_check.cpp walks the launch geometry and the per-dword arithmetic of csrc/sdrfm_iq_meter.h, tests/native/iq_meter_sanity.c the plain-C
host side (csrc/iq_meter.c) over exactly-sized heap rows and its refusals.  Then the C routine through the library against tests/iq_meter_ref.py
(the numpy restatement of the definition): records and rows by integer equality, the reports within 1e-9, the recovery of a known impairment,
the degenerate records and the gain policy."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import iq_meter_cases as cases
import iq_meter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr
    return r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_and_arithmetic_clean_under_asan_and_ubsan(pkg, tmp_path):
    """every byte of a row exactly once at every nbytes in 0 .. 4096 and at the maximum, row offsets 0 .. 17; the 32-bit lane bound at the maximum
    with all-255 bytes; the SWAR rail test over all 2^16 halfwords; the dot-product masks at both parities.  The geometry it prints is the Python
    mirror's, which the GPU tests take their shapes from."""
    exe = str(tmp_path / "iq_meter_check")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests/native/iq_meter_check.cpp")]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    from importlib import import_module
    geometry = import_module("stm32f7-rtlsdr_amd.iqmeter").iq_meter_geometry
    grids = [tuple(int(v) for v in line.split()[1:]) for line in _run(exe).splitlines() if line.startswith("grid ")]
    assert len(grids) >= 10
    for ns, nbytes, bps, share in grids:
        assert geometry(ns, nbytes) == (bps, share), (ns, nbytes)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_side_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "iq_meter_sanity")
    src = [os.path.join(ROOT, p) for p in ("tests/native/iq_meter_sanity.c", "stm32f7-rtlsdr_amd/csrc/iq_meter.c")]
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-static-libasan"] + SAN + ["-o", exe] + src + ["-lm"]
    subprocess.run(cmd, check=True, cwd=ROOT, capture_output=True, text=True)
    _run(exe)


def _check_row(pkg, x):
    rec, rows = pkg.iq_meter_host(x, with_hist=True)
    want = ref.record(x)
    assert ref.rec_tuple(rec[0]) == want
    assert np.array_equal(rows[0].astype(np.int64), ref.hist(x))
    assert ref.ties(want, rows[0])
    assert ref.rec_tuple(pkg.iq_meter_host(x)[0]) == want            # the record alone


def test_c_routine_is_the_definition(pkg):
    for nbytes in (0, 2) + cases.SMALL + cases.STEP + (100002,):
        _check_row(pkg, cases.random_rows(7, 1, nbytes)[0])
    for value in (0, 255, 128):
        x = cases.constant(value, 4096 + 6)
        _check_row(pkg, x)
        n = x.size // 2
        rail = n if value in (0, 255) else 0
        assert ref.rec_tuple(pkg.iq_meter_host(x)[0]) == (n, n * value, n * value, n * value ** 2, n * value ** 2, n * value ** 2, rail, rail)
    x = cases.ramp()
    _check_row(pkg, x)
    # all 65536 pairs once: sum b = 256 * 32640, sum b^2 = 256 * 5559680, sum bI bQ = 32640^2, 512 rail bytes per component
    assert ref.rec_tuple(pkg.iq_meter_host(x)[0]) == (65536, 256 * 32640, 256 * 32640, 256 * 5559680, 256 * 5559680, 32640 ** 2, 512, 512)


def test_ragged_even_cuts_add_up_and_add_is_associative(pkg):
    x = cases.random_rows(8, 1, 20000)[0]
    whole, hwhole = pkg.iq_meter_host(x, with_hist=True)
    acc, hacc, at = np.zeros(1, pkg.IQ_METER_DTYPE), np.zeros((1, 512), np.uint64), 0
    pieces = []
    for c in cases.CUTS + (6, 0, 1022, 20000):
        c = min(c, x.size - at)
        rec, rows = pkg.iq_meter_host(x[at:at + c], with_hist=True)
        assert ref.rec_tuple(rec[0]) == ref.record(x[at:at + c])
        pkg.iq_meter_add(acc, rec)
        pkg.iq_hist_add(hacc, rows.astype(np.uint32))
        pieces.append(rec)
        at += c
    assert at == x.size and acc.tobytes() == whole.tobytes() and np.array_equal(hacc, hwhole)
    # the routine accumulates: a second piece onto the first's record and row is the join
    r2, h2 = pkg.iq_meter_host(x[5000:], *pkg.iq_meter_host(x[:5000], with_hist=True))
    assert r2.tobytes() == whole.tobytes() and np.array_equal(h2, hwhole)
    # (a + b) + c == a + (b + c), on records of different calls
    a, b, c = pieces[0].copy(), pieces[2].copy(), pieces[3].copy()
    left = pkg.iq_meter_add(pkg.iq_meter_add(a.copy(), b), c)
    right = pkg.iq_meter_add(a.copy(), pkg.iq_meter_add(b.copy(), c))
    assert left.tobytes() == right.tobytes() and ref.rec_tuple(left[0]) == ref.add(ref.add(ref.rec_tuple(a[0]), ref.rec_tuple(b[0])), ref.rec_tuple(c[0]))


def _report_matches(pkg, x):
    rec, rows = pkg.iq_meter_host(x, with_hist=True)
    got, want = pkg.iq_meter_report(rec), ref.report(ref.record(x))
    for f in ref.REPORT_FIELDS:
        assert ref.close(float(got[f][0]), want[f]), (f, float(got[f][0]), want[f])
    hgot, hwant = pkg.iq_hist_report(rows), ref.hist_report(ref.hist(x))
    assert int(hgot["n"][0]) == hwant["n"]
    for f in hwant:
        if f != "n":
            assert ref.close(float(hgot[f][0]), hwant[f]), (f, float(hgot[f][0]), hwant[f])
    return got, hgot


def test_reports_are_the_restatement(pkg):
    for x in (cases.random_rows(9, 1, 50000)[0], cases.ramp(), cases.constant(128, 64), cases.constant(0, 64), cases.constant(255, 2),
              np.tile(np.array([0, 255, 255, 0], np.uint8), 500), np.tile(np.array([10, 200], np.uint8), 77)):
        _report_matches(pkg, x)
    # a long quiet capture: 2^25 pairs that differ from 128 in ONE bit of a few samples — the variance is 15 orders under sum b^2 and survives
    rec = np.zeros(1, pkg.IQ_METER_DTYPE)
    n, k = 1 << 25, 3
    rec["n"], rec["sum_i"], rec["sum_q"] = n, 128 * n + k, 128 * n
    rec["sum_ii"], rec["sum_qq"], rec["sum_iq"] = 128 * 128 * (n - k) + 129 * 129 * k, 128 * 128 * n, 128 * (128 * n + k)
    got, want = pkg.iq_meter_report(rec), ref.report(ref.rec_tuple(rec[0]))
    assert want["rms_dbfs"] < -110 and math.isnan(want["gain_db"])
    for f in ref.REPORT_FIELDS:
        assert ref.close(float(got[f][0]), want[f]), (f, float(got[f][0]), want[f])


# Recovery of a known impairment (IMPAIR in iq_meter_cases.py: g = 1.05, 3 degrees, DC (+2.3, -1.7)) by the moment estimators, which is a property of
# the DEFINITION and so the same for host and device.  The tolerances are 3 x the largest error of tests/iq_meter_ref.py's report over the eight seeds
# 0 .. 7 of each capture kind (240 000 pairs), measured with numpy alone:
#                 gain_db    skew_rad   dc_i     dc_q
#   stations      0.0027     0.00034    0.306    0.0085      (means over the seeds: 0.4246 dB against 0.4238, 2.99 against 3 degrees)
#   noise only    0.0465     0.00318    0.364    0.0752
# dc_i reads 0.3 LSB low in every seed: impair_iq leaves I a byte plus 2.3, which rounds to the byte plus 2 — the capture's own DC, not the meter's
# error.  The image rejection follows from gain and skew: 28.93 dB for this impairment, read within 0.3 dB in all sixteen captures.
RECOVERY = {"stations": dict(gain_db=3 * 0.0027, skew_rad=3 * 0.00034, dc_i=3 * 0.306, dc_q=3 * 0.0085),
            "noise": dict(gain_db=3 * 0.0465, skew_rad=3 * 0.00318, dc_i=3 * 0.364, dc_q=3 * 0.0752)}


@pytest.mark.parametrize("kind", ["stations", "noise"])
def test_report_recovers_a_known_impairment(pkg, kind):
    tol = RECOVERY[kind]
    truth = dict(gain_db=20 * math.log10(cases.IMPAIR["gain_q"]), skew_rad=float(cases.IMPAIR["skew_rad"]), dc_i=cases.IMPAIR["dc_i"], dc_q=cases.IMPAIR["dc_q"])
    for seed in (0, 5):
        x = (cases.stations_capture if kind == "stations" else cases.noise_capture)(pkg, seed)
        got, hgot = _report_matches(pkg, x)
        for f in tol:
            print(kind, seed, f, float(got[f][0]), truth[f])
            assert abs(float(got[f][0]) - truth[f]) <= tol[f], (kind, seed, f, float(got[f][0]), truth[f])
        assert abs(float(got["image_rejection_db"][0]) - 28.926) <= 0.9          # 3 x the 0.3 dB above
        assert float(got["rail_share_i"][0]) == 0.0 and float(hgot["peak_i"][0]) < 1.0
        assert float(got["total_dbfs"][0]) > float(got["rms_dbfs"][0])


def test_degenerate_records(pkg):
    rep = pkg.iq_meter_report(np.zeros(2, pkg.IQ_METER_DTYPE))
    assert all(np.isnan(rep[f]).all() for f in ref.REPORT_FIELDS)                 # n == 0: NaN, as the other report routines answer
    hrep = pkg.iq_hist_report(np.zeros(512, np.uint64))
    assert int(hrep["n"][0]) == 0 and all(np.isnan(hrep[f][0]) for f in hrep if f != "n")
    for value in (0, 128, 255):
        rep = pkg.iq_meter_report(pkg.iq_meter_host(cases.constant(value, 1000)))
        assert rep["rms_dbfs"][0] == -np.inf and rep["dc_i"][0] == value - 127.5 and np.isfinite(rep["total_dbfs"][0])
        assert np.isnan(rep["gain_db"][0]) and np.isnan(rep["skew_rad"][0]) and np.isnan(rep["image_rejection_db"][0])
    # one component constant: a level, but no imbalance
    x = cases.random_rows(3, 1, 1000)[0]
    x[1::2] = 77
    rep = pkg.iq_meter_report(pkg.iq_meter_host(x))
    assert np.isfinite(rep["rms_dbfs"][0]) and np.isnan(rep["gain_db"][0]) and np.isnan(rep["image_rejection_db"][0])
    # a tone that just touches the rails reads 0 dBFS
    ph = 2 * np.pi * 0.0123 * np.arange(100000)
    t = np.empty(200000, np.uint8)
    t[0::2], t[1::2] = np.rint(127.5 + 127.5 * np.cos(ph)), np.rint(127.5 + 127.5 * np.sin(ph))
    assert abs(pkg.iq_meter_report(pkg.iq_meter_host(t))["rms_dbfs"][0]) < 0.01


def test_gain_policy_corners(pkg):
    def rep(lvl, ri=0.0, rq=0.0):
        return {"rms_dbfs": np.array([lvl]), "rail_share_i": np.array([ri]), "rail_share_q": np.array([rq])}
    assert pkg.gain_advice(rep(-12.0))[0] == 0.0
    assert pkg.gain_advice(rep(-15.5))[0] == 3.5 and pkg.gain_advice(rep(-9.0))[0] == -3.0
    assert pkg.gain_advice(rep(-40.0))[0] == 6.0 and pkg.gain_advice(rep(-1.0))[0] == -6.0          # clamped
    assert pkg.gain_advice(rep(-18.0))[0] == 6.0 and pkg.gain_advice(rep(-18.0 + 1e-9))[0] < 6.0
    assert pkg.gain_advice(rep(-30.0, ri=2e-4))[0] == -6.0 and pkg.gain_advice(rep(-30.0, rq=2e-4))[0] == -6.0   # rails beat a low reading
    assert pkg.gain_advice(rep(-30.0, ri=1e-4, rq=1e-4))[0] == 6.0                                  # AT the limit is not over it
    assert pkg.gain_advice(rep(-np.inf))[0] == 6.0 and pkg.gain_advice(rep(np.nan))[0] == 0.0
    assert pkg.gain_advice(rep(-20.0), target_dbfs=-10.0, max_step_db=3.0)[0] == 3.0
    assert pkg.gain_advice(rep(-20.0, ri=0.5), max_rail_share=0.6)[0] == 6.0
    both = pkg.gain_advice({"rms_dbfs": np.array([-12.0, -20.0]), "rail_share_i": np.array([1.0, 0.0]), "rail_share_q": np.zeros(2)})
    assert both.tolist() == [-6.0, 6.0]
    gains = [0, 9, 14, 27, 37, 77, 87, 125, 144, 157, 166, 197]                                     # (any list a caller's tuner reports)
    assert pkg.nearest_gain(gains, 87, 0.0) == 87 and pkg.nearest_gain(gains, 87, 6.0) == 144      # 147 wanted: 144 is 3 off, 157 is 10 off
    assert pkg.nearest_gain(gains, 0, -6.0) == 0 and pkg.nearest_gain(gains, 197, 6.0) == 197      # the ends hold
    assert pkg.nearest_gain([100, 110], 100, 0.5) == 100                                            # a tie goes to the lower
    assert pkg.nearest_gain([110, 100], 93, 1.2) == 100 and pkg.nearest_gain([50], 0, 3.0) == 50
    with pytest.raises(ValueError):
        pkg.nearest_gain([], 0, 0.0)
    # the loop closes: the advice from a real report lands on a list entry
    r = pkg.iq_meter_report(pkg.iq_meter_host(cases.noise_capture(pkg, 1)))
    step = pkg.gain_advice(r)[0]
    assert abs(step - (-12.0 - r["rms_dbfs"][0])) < 1e-12 and pkg.nearest_gain(gains, 87, step) in gains


def test_impair_iq(pkg):
    x = cases.random_rows(4, 2, 64)
    assert np.array_equal(pkg.impair_iq(x), x)                                                      # no impairment: the bytes
    y = pkg.impair_iq(x, dc_i=3.0, dc_q=-2.0)
    assert np.array_equal(y[:, 0::2], np.clip(x[:, 0::2].astype(int) + 3, 0, 255)) and np.array_equal(y[:, 1::2], np.clip(x[:, 1::2].astype(int) - 2, 0, 255))
    z = pkg.impair_iq(x, drive=4.0)
    assert z.min() == 0 and z.max() == 255 and z.dtype == np.uint8 and z.shape == x.shape           # overdriven: clipped to the rails
