"""CPU checks of scan.pilot_snr_db and scan.audio_policy on the scan scenarios' reference records (tests/scan_cases.py)
and on the ladder of tools/audio_ladder.py, whose rungs are what the policy's two defaults were read from."""
import importlib.util
import os

import numpy as np
import pytest

import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 32768


def _streams(pkg, scenario, stations):
    """(offsets the streams are tuned to, their entries of the scenario's reference report, stream_status of them) for the given stations"""
    offsets, _, report = sc.scenario_reference(pkg, scenario)
    cand = [int(np.argmin(np.abs(offsets - st["offset_hz"]))) for st in stations]
    rep = {k: v[cand] for k, v in report.items()}
    return offsets[cand], rep, pkg.stream_status(rep, offsets[cand])


def test_pilot_snr_db_inverts_the_steadiness_of_a_tone_in_noise(pkg):
    got = pkg.pilot_snr_db(dict(pilot_steadiness=np.array([1.0, 1.5, 2.0, 0.9, 2.5, np.nan])))
    # s = 1.5: u = 1 - sqrt(1/2), rho = 1 / u - 1 = sqrt(2) + 1
    assert got[0] == np.inf and got[2] == -np.inf and got[3] == np.inf and got[4] == -np.inf and got[5] == -np.inf
    assert abs(got[1] - 10 * np.log10(np.sqrt(2.0) + 1.0)) < 1e-12
    # the forward relation, and monotone: the steadier the pilot the higher the estimate
    rho = 10.0 ** (np.linspace(-30.0, 60.0, 181) / 10.0)
    s = 1.0 + (2.0 * rho + 1.0) / (rho + 1.0) ** 2
    back = pkg.pilot_snr_db(dict(pilot_steadiness=s))
    ok = rho < 1e5                                                   # (beyond, 2 - s is 1 to the last bits of a double)
    assert np.abs(back[ok] - 10 * np.log10(rho[ok])).max() < 1e-4
    grid = np.linspace(1.0001, 1.9999, 2000)
    assert (np.diff(pkg.pilot_snr_db(dict(pilot_steadiness=grid))) < 0).all()
    assert pkg.pilot_snr_db(dict(pilot_steadiness=1.25)).shape == (1,)


def test_policy_on_the_weak_stations_scenario(pkg):
    import tuned_cases as tc
    stations = tc.STATIONS + sc.WEAK
    tuned, rep, status = _streams(pkg, "two-weak-extra", stations)
    snr = pkg.pilot_snr_db(rep)
    blend, gain = pkg.audio_policy(rep, status)
    print("pilot SNR (dB) %s -> blend %s, gain %s" % ([round(float(v), 1) for v in snr], list(blend), list(gain)))
    assert blend.dtype == gain.dtype == np.uint16 and blend.shape == gain.shape == (5,)
    assert all(s["present"] and s["stereo"] for s in status)
    assert (blend[:3] == ONE).all() and (snr[:3] > 27.0).all()      # the three strong stations
    assert blend[3] == ONE and abs(snr[3] - 24.0) < 1.0             # "WEAK -14"
    assert 16384 < blend[4] < 26214, (blend[4], snr[4])             # "WEAK -20": 18.4 dB -> 0.64, +-1.4 dB
    assert (gain == ONE).all()
    # the corners are arguments
    b2, _ = pkg.audio_policy(rep, status, stereo_full_db=float(snr[4]), stereo_off_db=0.0)
    assert b2[4] == ONE
    b3, _ = pkg.audio_policy(rep, status, stereo_full_db=60.0, stereo_off_db=float(snr[4]))
    assert b3[4] == 0 and (b3[:3] > 0).all() and (b3[:3] < ONE).all()


def test_policy_on_the_drifted_scenario_with_a_mono_station(pkg):
    stations = sorted(sc.scenario_capture(pkg, "crystal+7kHz-and-mono")[1], key=lambda t: t["offset_hz"])
    tuned, rep, status = _streams(pkg, "crystal+7kHz-and-mono", stations)
    blend, gain = pkg.audio_policy(rep, status)
    mono = [k for k, st in enumerate(stations) if not st["stereo"]]
    assert len(mono) == 1 and status[mono[0]]["present"] and not status[mono[0]]["stereo"]
    assert blend[mono[0]] == 0 and gain[mono[0]] == ONE
    assert all(blend[k] == ONE and gain[k] == ONE for k in range(4) if k not in mono)


def test_policy_mutes_every_stream_of_a_capture_of_noise(pkg):
    stations = sorted(sc.scenario_capture(pkg, "crystal+7kHz-and-mono")[1], key=lambda t: t["offset_hz"])   # (the same four candidates)
    tuned, rep, status = _streams(pkg, "noise-only", stations)
    blend, gain = pkg.audio_policy(rep, status)
    assert not any(s["present"] for s in status)
    assert (gain == 0).all() and (blend == 0).all()
    blend, gain = pkg.audio_policy(rep, status, mute_absent=False)
    assert (gain == ONE).all() and (blend == 0).all()


@pytest.fixture(scope="module")
def ladder_tool():
    spec = importlib.util.spec_from_file_location("audio_ladder", os.path.join(ROOT, "tools", "audio_ladder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_ladder_the_defaults_were_read_from(pkg, ladder_tool):
    assert ladder_tool.AMPLITUDES == (100.0, 10.0, 5.0, 3.0, 2.0)
    rows = ladder_tool.ladder()
    for line in ladder_tool.table(rows):
        print(line)
    snr = [r["pilot_snr_db"] for r in rows]
    assert all(a > b for a, b in zip(snr, snr[1:])), snr              # the estimate falls strictly with the amplitude
    assert rows[0]["blend"] == ONE and rows[-1]["blend"] == 0
    assert all(r["gain"] == ONE and r["present"] for r in rows)
    # what the defaults rest on: no loss where the policy still gives full stereo, a loss where it has begun to blend
    for r in rows:
        if r["blend"] == ONE:
            assert r["stereo_snr_db"] >= r["mono_snr_db"], r
        if r["blend"] < ONE // 2:
            assert r["stereo_snr_db"] < r["mono_snr_db"], r
