"""CPU checks of scan.hicut_policy: monotone in the pilot's SNR, 32768 at and above full_db, floor_q15 at and below
floor_db, linear in dB between them; 32768 for mono and absent streams; the strong stations of a scan scenario untouched; and the
defaults are the ones profiles/hicut_ladder.txt records."""
import os
import re

import numpy as np

import scan_cases as sc
from test_stream_status_cpu import tuned_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _steadiness(snr_db):
    """pilot_snr_db's inverse: s = 1 + (2 rho + 1) / (rho + 1)^2"""
    rho = 10.0 ** (np.asarray(snr_db, np.float64) / 10.0)
    return 1.0 + (2.0 * rho + 1.0) / (rho + 1.0) ** 2


def _streams(snr_db, stereo=True, present=True):
    snr_db = np.atleast_1d(np.asarray(snr_db, np.float64))
    report = dict(pilot_steadiness=_steadiness(snr_db))
    status = [dict(stream=s, present=present, stereo=present and stereo) for s in range(snr_db.size)]
    return report, status


def test_policy_is_monotone_and_pinned_at_both_ends(pkg):
    scan = pkg.scan
    snr = np.arange(0.0, 30.0, 0.25)
    report, status = _streams(snr)
    assert np.allclose(pkg.pilot_snr_db(report), snr, atol=1e-9)
    h = pkg.hicut_policy(report, status)
    assert h.dtype == np.uint16 and h.shape == snr.shape
    assert np.all(np.diff(h.astype(np.int64)) >= 0)
    full, floor_db, floor_q = scan.STEREO_OFF_DB, scan.HICUT_FLOOR_DB, scan.HICUT_FLOOR_Q15
    assert np.all(h[snr >= full + 1e-6] == 32768) and np.all(h[snr <= floor_db - 1e-6] == floor_q)
    mid = (snr > floor_db) & (snr < full)
    assert mid.any() and np.all((h[mid] > floor_q) & (h[mid] < 32768))
    # exactly at the corners, and linear in dB between them, rounded to nearest
    report, status = _streams([full, floor_db, (full + floor_db) / 2.0])
    got = pkg.hicut_policy(report, status)
    assert abs(int(got[0]) - 32768) <= 1 and abs(int(got[1]) - floor_q) <= 1 and abs(int(got[2]) - (32768 + floor_q) // 2) <= 1
    # other corners
    report, status = _streams([25.0, 20.0, 15.0, 10.0, 5.0])
    assert list(pkg.hicut_policy(report, status, full_db=20.0, floor_db=10.0, floor_q15=4096)) == [32768, 32768, (32768 + 4096) // 2, 4096, 4096]
    # +-inf: a pure tone and pure noise
    rep = dict(pilot_steadiness=np.array([1.0, 2.0, 0.9, 2.5]))
    assert list(pkg.hicut_policy(rep, _streams([0.0] * 4)[1])) == [32768, floor_q, 32768, floor_q]


def test_mono_and_absent_streams_are_left_alone(pkg):
    report, _ = _streams([3.0, 3.0, 3.0, 3.0])
    status = [dict(stream=0, present=True, stereo=True), dict(stream=1, present=True, stereo=False), dict(stream=2, present=False, stereo=False),
              dict(stream=3, present=False, stereo=True)]
    got = pkg.hicut_policy(report, status)
    assert list(got) == [pkg.scan.HICUT_FLOOR_Q15, 32768, 32768, 32768]


def test_strong_stations_of_a_scenario_get_no_high_cut(pkg):
    tuned, rep, truth = tuned_streams(pkg)
    status = pkg.stream_status(rep, tuned)
    got = pkg.hicut_policy(rep, status)
    assert all(s["present"] for s in status) and [s["stereo"] for s in status].count(False) == 1
    assert list(got) == [32768] * 4, (got, pkg.pilot_snr_db(rep))
    # the same candidates of a capture of noise: nothing present, nothing cut
    tuned, rep, _ = tuned_streams(pkg, "noise-only")
    assert list(pkg.hicut_policy(rep, pkg.stream_status(rep, tuned))) == [32768] * 4


def test_defaults_are_the_ladders(pkg):
    with open(os.path.join(ROOT, "profiles", "hicut_ladder.txt")) as fh:
        text = fh.read()
    m = re.search(r"^picked: floor_db ([0-9.]+), floor_q15 (\d+)$", text, re.M)
    assert m, text
    assert float(m.group(1)) == pkg.scan.HICUT_FLOOR_DB and int(m.group(2)) == pkg.scan.HICUT_FLOOR_Q15
    m = re.search(r"^hicut_policy's defaults: full_db ([0-9.]+) .*floor_db ([0-9.]+), floor_q15 (\d+)\.$", text, re.M)
    assert m and float(m.group(1)) == pkg.scan.STEREO_OFF_DB and float(m.group(2)) == pkg.scan.HICUT_FLOOR_DB and int(m.group(3)) == pkg.scan.HICUT_FLOOR_Q15
    import inspect
    sig = inspect.signature(pkg.hicut_policy)
    assert (sig.parameters["full_db"].default, sig.parameters["floor_db"].default, sig.parameters["floor_q15"].default) == (
        pkg.scan.STEREO_OFF_DB, pkg.scan.HICUT_FLOOR_DB, pkg.scan.HICUT_FLOOR_Q15)
    assert pkg.scan.HICUT_FLOOR_DB < pkg.scan.STEREO_OFF_DB and 1024 <= pkg.scan.HICUT_FLOOR_Q15 < 32768
