"""CPU checks of the deviation histogram's definition on the reference's d (tests/scan_ref.py): rows add up over ragged cuts
and sum to the record's n; the generated monitoring scenarios of tests/scan_hist_cases.py — mono tone stations of 50 and 75 kHz peak
deviation, a station 7 kHz off its tuning, noise only — through sdrfm_scan_hist_report, their measured figures kept in
tests/golden/scan_hist_scenarios.json; the hist kernel's step geometry against the plain kernel's; and, for every GPU case that is held to
the reference from bytes, the share of d's within 1e-5 rad of a bin edge."""
import json
import os

import numpy as np
import pytest

import pilot_shape_cases as ps
import scan_hist_cases as hc
import scan_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_hist_scenarios.json")
BIN_HZ = hc.FS / (2.0 * np.pi * hc.D) / 64.0
FIELDS = ("centre_hz", "peak_pos_hz", "peak_neg_hz", "peak_hz", "over_min", "over_max", "mpx_power_dbr")


def test_definition_on_hand_made_d():
    d = np.array([0.0, -0.0, 2.0 ** -7, -2.0 ** -25, -2.0 ** -24, 1.0 / 64 - 2.0 ** -25, 1.0 / 64 - 2.0 ** -24, np.pi, -np.pi, 3.140625, -3.140625], np.float32)
    h = hc.hist_of(d)
    # rint to even: -2^-25 2^24 = -0.5 -> -0, bin 256; 1/64 - 2^-25 -> 2^18 - 0.5 -> 2^18 (even), bin 257; 1/64 - 2^-24 -> 2^18 - 1, bin 256
    want = {256: 5, 255: 1, 257: 1, 457: 2, 54: 1, 55: 1}
    assert {int(b): int(h[b]) for b in np.flatnonzero(h)} == want, {int(b): int(h[b]) for b in np.flatnonzero(h)}
    assert int(h.sum()) == d.size and h.size == hc.BINS


def test_rows_add_up_over_ragged_cuts_and_sum_to_n(pkg):
    cs = hc.tuned_case(pkg, hc.TUNED_CASES[1])                      # T7-D3-P5: station, unmodulated carrier, random
    D = cs["shape"][1]
    rng = np.random.default_rng(77)
    for s, r in enumerate(cs["refs"]):
        M = r["d"].size
        cuts = [0, 0, 1, 3] + sorted(int(v) for v in rng.integers(4, M, 6)) + [M, M]
        acc = np.zeros(hc.BINS, np.uint64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = hc.hist_of(r["d"][a:b])
            rec = sr.scan_ref(cs["iq"][s], cs["ctaps"][s], cs["rot"][s], D, cs["b"], 0.05, a, b)["rec"]
            assert int(part.sum()) == rec["n"] == b - a, (s, a, b)
            pkg.hist_add(acc, part.astype(np.uint32))
        assert np.array_equal(acc, hc.hist_of(r["d"])) and int(acc.sum()) == r["rec"]["n"] == M
        assert not acc[:54].any() and not acc[458:].any()


def _table(pkg):
    out = {}
    for name in hc.SCENARIOS:
        sn = hc.scenario(pkg, name)
        rep = pkg.hist_report(sn["hist"], sn["meters"], hc.FS, hc.D, limit_hz=75e3)
        lo, hi = pkg.deviation_quantile(sn["hist"], sn["meters"], hc.FS, hc.D, 0.01)
        out[name] = dict({f: round(float(rep[f][0]), 3) if f.endswith("hz") or f.endswith("dbr") else round(float(rep[f][0]), 6) for f in FIELDS},
                         n=int(rep["n"][0]), bins_in_use=int(np.count_nonzero(sn["hist"])), deviation_passed_1pct_hz=[round(float(lo[0]), 3), round(float(hi[0]), 3)],
                         edge_share=round(hc.edge_share(sn["ref"]["d"][hc.SCENARIO_WARM:]), 6))
    return out


@pytest.mark.parametrize("name", list(hc.SCENARIOS))
def test_scenarios(pkg, name):
    """the structural facts, and the measured figures against the recorded ones"""
    sn = hc.scenario(pkg, name)
    st, hist, meters = sn["truth"], sn["hist"], sn["meters"]
    assert int(hist.sum()) == int(meters["n"][0]) == hc.SCENARIO_SAMPLES // hc.D - hc.SCENARIO_WARM
    rep = {f: float(v[0]) for f, v in pkg.hist_report(hist, meters, hc.FS, hc.D, limit_hz=75e3).items()}
    plain = pkg.meter_report(meters, hc.FS, hc.D)
    print(name, rep)
    assert rep["centre_hz"] == plain["freq_err_hz"][0]
    assert 0.0 <= rep["over_min"] <= rep["over_max"] <= 1.0 and rep["peak_hz"] == max(rep["peak_pos_hz"], -rep["peak_neg_hz"])
    if st is not None:
        assert rep["peak_hz"] >= st["peak_hz"] - BIN_HZ, (rep["peak_hz"], st["peak_hz"])
        assert abs(rep["centre_hz"] - (st["offset_hz"] - sn["tuned_hz"])) <= 100.0, rep["centre_hz"]          # §4.13's bound on a tuning error
        # a tone of peak deviation p has the modulation power p^2 / 2: 20 log10(p / 19 kHz) against BS.412's reference, the noise on top of it
        assert abs(rep["mpx_power_dbr"] - 20.0 * np.log10(st["peak_hz"] / 19e3)) <= 0.1, rep["mpx_power_dbr"]
    else:
        assert rep["peak_hz"] > 119e3 and rep["over_max"] > 0.3        # d is uniform in +-pi on an empty channel: 120 kHz either way
    if name == "tone-50kHz":
        assert rep["over_max"] == 0.0 and rep["peak_hz"] < 75e3        # as measured: nothing of a 50 kHz station beyond 75 kHz
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    have = _table(pkg)[name]
    assert have["n"] == want["n"]
    # (the capture comes from numpy's generator and libm: the recorded figures are held to a bin or a part in a thousand, not to the last digit)
    for f in ("centre_hz", "peak_pos_hz", "peak_neg_hz", "peak_hz"):
        assert abs(have[f] - want[f]) <= BIN_HZ, (name, f, have[f], want[f])
    for f in ("over_min", "over_max"):
        assert abs(have[f] - want[f]) <= 1e-3, (name, f, have[f], want[f])
    assert abs(have["mpx_power_dbr"] - want["mpx_power_dbr"]) <= 0.01


def test_modulation_monitor_over_a_scenario_in_calls(pkg):
    """the 75 kHz station cut into five calls of 20 ms: the monitor's running histogram and record are the one call's"""
    sn = hc.scenario(pkg, "tone-75kHz")
    d, M, W = sn["ref"]["d"], sn["ref"]["d"].size, hc.SCENARIO_WARM
    h, b = hc.sc.shape_taps(pkg, hc.sc.SHAPES["default"])
    mon = pkg.ModulationMonitor(1, hc.FS, hc.D)
    for a in range(0, M, M // 5):                                    # (the first call without the stream's first d's, as the scenario is)
        rec = sr.scan_ref(sn["row"], pkg.tuned_channel_taps(h, sn["tuned_hz"], hc.FS), pkg.tuned_rotation(sn["tuned_hz"], hc.FS, hc.D), hc.D, b, 0.05, max(a, W),
                          a + M // 5)["rec"]
        m = np.zeros(1, pkg.METER_DTYPE)
        for k, v in rec.items():
            m[k][0] = v
        mon.push(m, hc.hist_of(d[max(a, W):a + M // 5]).astype(np.uint32)[None, :])
    assert np.array_equal(mon.hist, sn["hist"]) and mon.meters.tobytes() == sn["meters"].tobytes()
    s = mon.summary()[0]
    rep = pkg.hist_report(sn["hist"], sn["meters"], hc.FS, hc.D)
    assert s["calls"] == 5 and s["over_max"] == rep["over_max"][0] and s["mpx_power_dbr"] == rep["mpx_power_dbr"][0]
    assert s["peak_hz"] >= 75e3 - BIN_HZ and 0.0 <= s["calls_over"] <= 1.0


def test_hist_step_geometry():
    """the bins take 2048 B (and what rounds the plain layout up to 16) of the LDS budget: the default shape keeps the full step at 53 168 B,
    the four LDS-limited shapes get a shorter step than the plain call's"""
    assert hc.step_of(hc.hist_lds, (64, 10, 101)) == (1023, 53168) and hc.step_of(hc.scan_lds, (64, 10, 101)) == (1023, 51120)
    want = {(256, 64, 255): (217, 223), (1, 64, 255): (227, 235), (255, 17, 3): (793, 821), (64, 16, 101): (853, 881)}
    for shape in ps.SCAN_SHAPES + [(64, 10, 101)]:
        (nh, lh), (np_, lp) = hc.step_of(hc.hist_lds, shape), hc.step_of(hc.scan_lds, shape)
        assert lh <= hc.LDS_BUDGET and lh % 16 == 0 and lh - hc.HIST_LDS_BYTES >= hc.scan_lds(*shape, nh + 1, nh)
        assert np_ == ps.scan_step(shape)["NDT"]
        if shape in ps.SCAN_LDS_LIMITED:
            assert (nh, np_) == want[shape], (shape, nh, np_)
        else:
            assert nh == np_ == 1023, (shape, nh, np_)


@pytest.mark.parametrize("case", hc.TUNED_CASES, ids=["%s-%dstreams" % (c[0], len(c[1])) for c in hc.TUNED_CASES])
def test_few_d_of_a_gpu_case_sit_at_a_bin_edge(pkg, case):
    """the GPU test lets a d change its bin where the reference's d lies within 1e-5 rad of the edge: that must stay a small share of every
    stream, the unmodulated carriers included (a smooth density gives 2 * 1e-5 * 64 = 0.13 %)"""
    cs = hc.tuned_case(pkg, case)
    for s, r in enumerate(cs["refs"]):
        share = hc.edge_share(r["d"])
        print("%s stream %d (%s): %.3f %% of %d d's within 1e-5 rad of a bin edge, %d bins in use" % (case[0], s, cs["names"][s], 100 * share, r["d"].size,
                                                                                                 np.count_nonzero(hc.hist_of(r["d"]))))
        assert share <= hc.EDGE_CAP, (case[0], s, cs["names"][s], share)
        assert int(hc.near_edge(r["d"]).sum()) == int(round(share * r["d"].size))
    for s, nm in enumerate(cs["names"]):
        if nm == "unmodulated":
            assert np.count_nonzero(hc.hist_of(cs["refs"][s]["d"])) <= 16


if __name__ == "__main__":                                          # python tests/test_scan_hist_ref.py: writes the golden table anew
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, "w") as fh:
        json.dump(_table(importlib.import_module("stm32f7-rtlsdr_amd")), fh, indent=1)
        fh.write("\n")
