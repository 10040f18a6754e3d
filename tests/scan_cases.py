"""The cases tests/test_scan_gpu.py holds the scan kernels to tests/scan_ref.py on, built without a device so that tests/test_scan_ref.py can
look at the reference side alone, and the four scan scenarios both files go through.

The cases are tests/tuned_cases.py's by import: its SHAPES reduced to (T, D, P), its OFFSETS and NBYTES, and its classes — 1 / 3 / 7 streams
of station / carrier / const in turn at pilot_min 0.05, random bytes at pilot_min 1e3 (the gate shut: the pilot powers of noise lie
anywhere, so any threshold among them would have d's at it)."""
import numpy as np

import scan_ref
import tuned_cases as tc

SHAPES = {name: s[:3] for name, s in tc.SHAPES.items()}         # (T, D, P)
OFFSETS, NBYTES, EXCLUDED_CAP = tc.OFFSETS, tc.NBYTES, tc.EXCLUDED_CAP
CASES = [("default", 1, "signal"), ("default", 3, "signal"), ("default", 7, "signal"), ("default", 3, "random"), ("T7-D3-P5", 7, "signal"),
         ("T7-D3-P5", 1, "random"), ("T16-D8", 3, "signal"), ("T16-D8", 7, "random"), ("Ta>Tr", 1, "signal")]

_refs = {}


def case_id(case):
    return "%s-%dstreams-%s" % case


def shape_taps(pkg, shape):
    """(h, b) of a shape: the channel low-pass and the pilot taps of tuned_cases.shape_taps"""
    T, D, P = shape
    fs = tc.fs_of(D)
    return pkg.lowpass_taps(T, min(120e3 / fs, 0.45)), pkg.stereo_pilot_taps(P, fs / D)


def case_setup(pkg, case):
    """dict(shape, h, b, ns, pilot_min, iq [ns, NBYTES], names, cycles, ctaps [ns, 2T], rot [ns]) of a case"""
    name, ns, kind = case
    shape = SHAPES[name]
    T, D, P = shape
    fs, idx = tc.fs_of(D), CASES.index(case)
    classes = ("station", "carrier", "const") if kind == "signal" else ("random",)
    names = [classes[s % len(classes)] for s in range(ns)]
    cycles = [OFFSETS[(s + idx) % len(OFFSETS)] for s in range(ns)]
    iq = np.stack([tc.stream_input(pkg, names[s], cycles[s], fs, NBYTES // 2, 7000 + 10 * idx + s) for s in range(ns)])
    h, b = shape_taps(pkg, shape)
    ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cycles])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cycles], np.float32)
    return dict(shape=shape, h=h, b=b, ns=ns, pilot_min=0.05 if kind == "signal" else 1e3, iq=iq, names=names, cycles=cycles, ctaps=ctaps, rot=rot)


def case_reference(pkg, case):
    """(setup, per-stream scan_ref.scan_ref results), computed once"""
    if case not in _refs:
        su = case_setup(pkg, case)
        D = su["shape"][1]
        _refs[case] = (su, [scan_ref.scan_ref(su["iq"][s], su["ctaps"][s], su["rot"][s], D, su["b"], su["pilot_min"]) for s in range(su["ns"])])
    return _refs[case]


# ---- the four scan scenarios: 0.1 s of one 2.4 MS/s capture, candidates on a 100 kHz grid from -1.1 to +1.1 MHz
FS, GRID_HZ, SCENARIO_SAMPLES, PILOT_MIN = 2.4e6, 100e3, 240000, 0.05
WEAK = [dict(offset_hz=-900e3, left_hz=500.0, right_hz=1.9e3, pi=0x3104, ps="WEAK -14", amplitude=40.0 * 10 ** (-14 / 20)),
        dict(offset_hz=+1000e3, left_hz=900.0, right_hz=2.7e3, pi=0x3105, ps="WEAK -20", amplitude=40.0 * 10 ** (-20 / 20))]
MONO = dict(offset_hz=-800e3, left_hz=1.2e3, right_hz=1.2e3, pi=0x3106, ps="MONO 800", pilot=False)
SCENARIOS = {                                                    # name -> (stations, crystal offset in Hz, seed)
    "three-on-the-grid": (tc.STATIONS, 0.0, 41),
    "crystal+7kHz-and-mono": (tc.STATIONS + [MONO], 7e3, 42),
    "two-weak-extra": (tc.STATIONS + WEAK, 0.0, 43),
    "noise-only": ([], 0.0, 44),
}

_scen = {}


def scenario_capture(pkg, name):
    """(iq row [2 SCENARIO_SAMPLES] uint8, truth: list of dict(offset_hz: where the carrier lies in the capture, stereo)), made once"""
    if name not in _scen:
        stations, xtal, seed = SCENARIOS[name]
        sts = [dict(dict(amplitude=40.0, rds_phase=0.5 * k, groups=pkg.rds_encode_groups(st["pi"], st["ps"])), **st) for k, st in enumerate(stations)]
        for st in sts:
            st["offset_hz"] = st["offset_hz"] + xtal
        row = pkg.make_iq_stations(SCENARIO_SAMPLES, sts, fs=FS, seed=seed)[0]
        row.setflags(write=False)
        _scen[name] = (row, [dict(offset_hz=st["offset_hz"], stereo=bool(st.get("pilot", True))) for st in sts])
    return _scen[name]


def scenario_taps(pkg):
    return shape_taps(pkg, SHAPES["default"])


_scen_refs = {}


def scenario_reference(pkg, name):
    """(offsets_hz of the candidates, the reference's records as a METER_DTYPE array, pkg.meter_report of them), computed once"""
    if name not in _scen_refs:
        row, _ = scenario_capture(pkg, name)
        h, b = scenario_taps(pkg)
        offsets = pkg.scan_grid(FS, GRID_HZ)
        meters = np.zeros(offsets.size, pkg.METER_DTYPE)
        for c, f in enumerate(offsets):
            r = scan_ref.scan_ref(row, pkg.tuned_channel_taps(h, f, FS), pkg.tuned_rotation(f, FS, 10), 10, b, PILOT_MIN)["rec"]
            for k, v in r.items():
                meters[k][c] = v
        _scen_refs[name] = (offsets, meters, pkg.meter_report(meters, FS, 10))
    return _scen_refs[name]


def check_found(found, truth):
    """find_stations' result against the truth: exactly the true set, each at the candidate nearest to it, the right stereo flags; returns
    the (found, true) pairs"""
    assert len(found) == len(truth), (found, truth)
    pairs = []
    for t in sorted(truth, key=lambda t: t["offset_hz"]):
        near = [f for f in found if abs(f["offset_hz"] - t["offset_hz"]) < GRID_HZ / 2]
        assert len(near) == 1, (t, found)
        assert near[0]["stereo"] == t["stereo"], (t, near[0])
        pairs.append((near[0], t))
    return pairs
