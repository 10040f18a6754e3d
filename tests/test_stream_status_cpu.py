"""CPU checks of stream_status on the scan scenarios' reference records (tests/scan_cases.py, tests/scan_ref.py): the
streams of a receiver tuned to the grid candidates nearest the true stations, and to the same candidates of a capture of noise."""
import numpy as np

import scan_cases as sc

SCENARIO = "crystal+7kHz-and-mono"


def tuned_streams(pkg, scenario=SCENARIO):
    """(offsets_hz the four streams are tuned to, their entries of the scenario's reference report, the truth in that order)"""
    offsets, _, report = sc.scenario_reference(pkg, scenario)
    truth = sorted(sc.scenario_capture(pkg, SCENARIO)[1], key=lambda t: t["offset_hz"])   # (noise-only: the same four candidates)
    cand = [int(np.argmin(np.abs(offsets - t["offset_hz"]))) for t in truth]
    return offsets[cand], {k: v[cand] for k, v in report.items()}, truth


def test_drifted_stations_are_present_and_located(pkg):
    tuned, rep, truth = tuned_streams(pkg)
    assert len(truth) == 4 and [t["stereo"] for t in truth].count(False) == 1
    status = pkg.stream_status(rep, tuned)
    assert len(status) == 4 and [s["stream"] for s in status] == [0, 1, 2, 3]
    for s, t, f in zip(status, truth, tuned):
        print("tuned %+.0f Hz: present %s stereo %s offset %+.1f Hz (true %+.1f), %.1f dBFS" % (f, s["present"], s["stereo"], s["offset_hz"],
                                                                                                 t["offset_hz"], s["level_dbfs"]))
        assert s["present"] is True and s["stereo"] is t["stereo"], (s, t)
        assert abs(s["offset_hz"] - t["offset_hz"]) < 100.0, (s, t)
        assert s["offset_hz"] == f + rep["freq_err_hz"][s["stream"]] and s["level_dbfs"] == rep["level_dbfs"][s["stream"]]
    # the policy is find_stations': the same candidates, offsets, levels and flags where both look
    offsets, _, report = sc.scenario_reference(pkg, SCENARIO)
    found = {f["candidate"]: f for f in pkg.find_stations(report, offsets, sc.GRID_HZ)}
    for s, f in zip(status, tuned):
        g = found[int(np.argmin(np.abs(offsets - f)))]
        assert (s["offset_hz"], s["level_dbfs"], s["stereo"]) == (g["offset_hz"], g["level_dbfs"], g["stereo"])


def test_noise_leaves_every_stream_absent_and_where_it_was(pkg):
    tuned, rep, _ = tuned_streams(pkg, "noise-only")
    status = pkg.stream_status(rep, tuned)
    assert len(status) == 4
    for s, f in zip(status, tuned):
        assert s["present"] is False and s["stereo"] is False and s["offset_hz"] == f, (s, f)
        assert np.isfinite(s["level_dbfs"])


def test_max_err_hz_is_honoured(pkg):
    tuned, rep, _ = tuned_streams(pkg)
    errs = np.abs(rep["freq_err_hz"])
    assert (errs > 6e3).all() and (errs < 8e3).all(), errs          # the crystal's 7 kHz
    for s, f in zip(pkg.stream_status(rep, tuned, max_err_hz=8e3), tuned):
        assert s["present"] and s["offset_hz"] != f
    for s, f in zip(pkg.stream_status(rep, tuned, max_err_hz=6e3), tuned):
        assert not s["present"] and not s["stereo"] and s["offset_hz"] == f, s
    # the bound is strict, stream by stream
    lim = float(np.sort(errs)[1])
    assert [s["present"] for s in pkg.stream_status(rep, tuned, max_err_hz=lim)] == [bool(e < lim) for e in errs]


def test_an_empty_record_is_an_absent_stream(pkg):
    rep = pkg.meter_report(np.zeros(2, pkg.METER_DTYPE), sc.FS, 10)
    for s, f in zip(pkg.stream_status(rep, [1e5, -2e5]), (1e5, -2e5)):
        assert not s["present"] and not s["stereo"] and s["offset_hz"] == f
