"""CPU checks of the scan record's definition (tests/scan_ref.py) and of what is made of it: sdrfm_scan_report's formulas
against float64 numpy on the reference's own d, the exact additivity of records over ragged cuts, the int64 bounds at the refusal limits,
the four scan scenarios through find_stations (their measured deviations and pilot steadiness are kept in
tests/golden/scan_scenarios.json, so that the two thresholds' margins are visible), and how many d's of every GPU case sit at the gate."""
import json
import os

import numpy as np
import pytest

import scan_cases as sc
import scan_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_scenarios.json")


def _meters(pkg, recs):
    m = np.zeros(len(recs), pkg.METER_DTYPE)
    for k, r in enumerate(recs):
        for f, v in r.items():
            m[f][k] = v
    return m


def test_report_is_the_float64_formulas_on_the_references_d(pkg):
    su, refs = sc.case_reference(pkg, sc.CASES[1])                  # default shape: a station, a carrier, a constant
    D, fs = su["shape"][1], sc.tc.fs_of(su["shape"][1])
    rep = pkg.meter_report(_meters(pkg, [r["rec"] for r in refs]), fs, D)
    hz = fs / (2 * np.pi * D)
    for s, r in enumerate(refs):
        d, p, pw = (r[k].astype(np.float64) for k in ("d", "p", "pw"))
        n = d.size
        # the fixed-point steps: half a step per term at the most, so the means are within half a step
        assert abs(rep["freq_err_hz"][s] - d.mean() * hz) <= 2.0 ** -25 * hz
        var = (d * d).mean() - d.mean() ** 2
        assert abs(rep["dev_rms_hz"][s] ** 2 - var * hz * hz) <= (2.0 ** -25 * (1 + 2 * np.pi)) * hz * hz + 1e-9 * var * hz * hz
        assert abs(10 ** (rep["level_dbfs"][s] / 10) * 127.5 ** 2 - p.mean()) <= 2.0 ** -9 + 1e-12 * p.mean()
        assert abs(rep["pilot_rms_rad"][s] ** 2 - pw.mean()) <= 2.0 ** -25 + 1e-12 * pw.mean()
        assert rep["pilot_frac"][s] == (r["pw"] >= r["pmin2"]).sum() / n
        assert rep["pilot_dev_hz"][s] == pytest.approx(rep["pilot_rms_rad"][s] * hz / pkg.pilot_gain(D, fs), rel=1e-12)
        if su["names"][s] == "station":
            want = n * (pw * pw).sum() / pw.sum() ** 2
            assert rep["pilot_steadiness"][s] == pytest.approx(want, rel=1e-4) and want < 1.05
            assert abs(rep["freq_err_hz"][s]) < 100.0 and 35e3 < rep["dev_rms_hz"][s] < 45e3
    assert pkg.pilot_gain(10, 2.4e6) == pytest.approx(0.98982, abs=1e-5)


def test_records_add_up_exactly_over_ragged_cuts(pkg):
    su = sc.case_setup(pkg, sc.CASES[4])                            # T7 D3 P5: the phase of the input against D matters
    D = su["shape"][1]
    iq, hz, rot = su["iq"][0], su["ctaps"][0], su["rot"][0]
    whole = sr.scan_ref(iq, hz, rot, D, su["b"], su["pilot_min"])["rec"]
    rng = np.random.default_rng(5)
    marks = np.sort(2 * rng.integers(1, iq.size // 2, 9))
    cuts = [0, 2, 2] + [int(v) for v in np.diff(np.concatenate([[6], marks, [iq.size]]))]
    cuts[3] += 2                                                     # (0 + 2 + 2 + the rest from byte 4)
    assert sum(cuts) == iq.size
    acc, samples, m0 = np.zeros(1, pkg.METER_DTYPE), 0, 0
    for c in cuts:
        samples += c // 2
        m1 = samples // D                                            # the d's whose newest input the calls so far hold
        pkg.meter_add(acc, _meters(pkg, [sr.scan_ref(iq, hz, rot, D, su["b"], su["pilot_min"], m0, m1)["rec"]]))
        m0 = m1
    assert sr.rec_of(acc[0]) == whole and whole["n"] == iq.size // 2 // D


def test_worst_case_sums_stay_inside_int64():
    """the bounds the handle refuses beyond — sum(|hr| + |hi|) <= 16, sum(|br| + |bi|) <= 8, 4 MiB a call — evaluated at their limits"""
    f32 = np.float32
    y = f32(127.5) * f32(16)                                        # |yr|, |yi| <= 127.5 sum|h|
    p = f32(2) * y * y
    n = (4 << 20) // 2                                               # D = 1: a d per sample
    q = f32(8) * f32(np.pi)                                          # |qr|, |qi| <= sum|b| max|d|
    pw = f32(2) * q * q
    assert y == 2040 and p == 8323200 and pw <= 1270 and n == 1 << 21
    worst = dict(rf_q=int(np.rint(p * f32(2 ** 8))) * n, freq_q=int(np.rint(f32(np.pi) * f32(2 ** 24))) * n,
                 dev_q=int(np.rint(f32(np.pi) * f32(np.pi) * f32(2 ** 24))) * n, pilot_q=int(np.rint(f32(1270) * f32(2 ** 24))) * n,
                 pilot2_q=int(np.rint(f32(1270) * f32(1270) * f32(2 ** 20))) * n)
    for k, bound in (("rf_q", 52), ("freq_q", 47), ("dev_q", 49), ("pilot_q", 56), ("pilot2_q", 62)):
        assert worst[k] < 2 ** bound <= 2 ** 62, (k, worst[k])


def _table(pkg):
    out = {}
    for name in sc.SCENARIOS:
        offsets, _, rep = sc.scenario_reference(pkg, name)
        out[name] = dict(offsets_khz=[float(f / 1e3) for f in offsets], dev_rms_hz=[round(float(v), 1) for v in rep["dev_rms_hz"]],
                         pilot_steadiness=[round(float(v), 4) for v in rep["pilot_steadiness"]])
    return out


@pytest.mark.parametrize("name", list(sc.SCENARIOS))
def test_scenario_finds_exactly_the_stations(pkg, name):
    """0.1 s of capture, 23 candidates: find_stations returns exactly the true set with the right stereo flags, every tuning error is
    within 100 Hz of the truth (fp32 d and the start-up d[0] = 0 are inside that), and the measured deviations and steadiness are the
    recorded ones"""
    offsets, meters, rep = sc.scenario_reference(pkg, name)
    row, truth = sc.scenario_capture(pkg, name)
    assert row.size == 2 * 240000 and offsets.size == 23 and offsets[0] == -1.1e6 and offsets[-1] == 1.1e6
    found = pkg.find_stations(rep, offsets, sc.GRID_HZ)
    for f, t in sc.check_found(found, truth):
        assert abs(f["offset_hz"] - t["offset_hz"]) <= 100.0, (f, t)
        assert f["offset_hz"] == offsets[f["candidate"]] + rep["freq_err_hz"][f["candidate"]]
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    have = _table(pkg)[name]
    assert have["offsets_khz"] == want["offsets_khz"]
    # (the capture comes from numpy's generator and libm: the recorded figures are held to a part in a thousand, not to the last digit)
    assert np.allclose(have["dev_rms_hz"], want["dev_rms_hz"], rtol=1e-3) and np.allclose(have["pilot_steadiness"], want["pilot_steadiness"], rtol=1e-3)
    # the margins of the two thresholds: no candidate between 47 and 64 kHz, no station's pilot between 1.03 and 1.8
    dev, ste = np.array(have["dev_rms_hz"]), np.array(have["pilot_steadiness"])
    assert not ((dev > 47e3) & (dev < 64e3)).any(), dev
    stations = [f["candidate"] for f in found]
    assert not ((ste[stations] > 1.03) & (ste[stations] < 1.8)).any() and (np.delete(ste, stations) > 1.8).all(), ste


@pytest.mark.parametrize("case", sc.CASES, ids=[sc.case_id(c) for c in sc.CASES])
def test_few_d_of_a_gpu_case_sit_at_the_gate(pkg, case):
    su, refs = sc.case_reference(pkg, case)
    for s, r in enumerate(refs):
        frac = float(sr.ambiguous(r["pw"], r["pmin2"]).mean())
        assert frac <= sc.EXCLUDED_CAP, (sc.case_id(case), s, su["names"][s], frac)


if __name__ == "__main__":                                          # python tests/test_scan_ref.py: writes the golden table anew
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, "w") as fh:
        json.dump(_table(importlib.import_module("stm32f7-rtlsdr_amd")), fh, indent=1)
        fh.write("\n")
