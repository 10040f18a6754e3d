"""The cases tests/test_bcast_tuned_gpu.py holds the tuned broadcast kernels to tests/tuned_ref.py on, built without a device so that
tests/test_tuned_ref.py can look at the reference side alone (how many of a case's outputs sit at the pilot gate).

A case is (shape, streams, kind).  Stream s is tuned to OFFSETS[(s + case index) % 5] cycles per sample and its input holds, at that
offset, what its class says: kind "signal" gives station / carrier / const in turn at pilot_min 0.05 (a carrier is a station without pilot
and subcarriers, const has no signal at all), kind "random" gives random bytes at pilot_min 1e3 (the gate shut: the pilot powers of noise
lie anywhere, so any threshold among them would have d's at it)."""
import numpy as np

import tuned_ref

SHAPES = {                                                      # (T, D, P, Ta, Da, Tr, Dr)
    "default": (64, 10, 101, 32, 5, 255, 25),
    "T7-D3-P5": (7, 3, 5, 5, 4, 9, 2),
    "T16-D8": (16, 8, 65, 32, 8, 64, 16),
    "Ta>Tr": (23, 10, 101, 64, 5, 33, 25),
}
RATE = {8: 2.048e6}                                             # D -> fs; 2.4 MS/s otherwise
OFFSETS = (0.25, -0.25, 0.5, 0.0417, -0.1667)                   # cycles per sample
CASES = [("default", 3, "signal"), ("default", 7, "signal"), ("default", 1, "random"), ("T7-D3-P5", 7, "signal"), ("T7-D3-P5", 3, "random"),
         ("T16-D8", 1, "signal"), ("T16-D8", 7, "random"), ("Ta>Tr", 3, "signal"), ("Ta>Tr", 1, "random")]
NBYTES = 125000                                                 # per stream: M >= 6 steps of the fast kernel, 3 workgroups a stream at the least
GROUPS = [(0x1234, 0x0408, 0xE0CD, 0x4142), (0x1234, 0x2400, 0x5244, 0x5320), (0x1234, 0x0409, 0xE0CD, 0x4344)]
EXCLUDED_CAP = 0.004                                            # of a case's outputs

_inputs, _refs = {}, {}


def case_id(case):
    return "%s-%dstreams-%s" % case


def fs_of(D):
    return RATE.get(D, 2.4e6)


def shape_taps(pkg, shape):
    T, D, P, Ta, Da, Tr, Dr = shape
    fs = fs_of(D)
    h = pkg.lowpass_taps(T, min(120e3 / fs, 0.45))
    ga = pkg.lowpass_taps(Ta, min(15e3 / (fs / D), 0.45))
    gr = pkg.lowpass_taps(Tr, min(3e3 / (fs / D), 0.45))
    b = pkg.stereo_pilot_taps(P, fs / D)
    return h, ga, gr, b, float(pkg.stereo_diff_gain(D, fs)), float(pkg.rds_gain(D, fs))


def stream_input(pkg, cls, cycles, fs, nsamp, seed):
    """one row of bytes: class `cls` at `cycles` per sample, made once"""
    key = (cls, cycles, fs, nsamp, seed)
    if key not in _inputs:
        if cls in ("station", "carrier"):
            st = dict(offset_hz=cycles * fs, amplitude=100.0, left_hz=1e3, right_hz=3.1e3, groups=GROUPS, rds_phase=0.4 * seed, pilot=cls == "station")
            row = pkg.make_iq_stations(nsamp, [st], fs=fs, seed=seed)[0]
        else:
            row = pkg.make_iq(1, nsamp, mode=cls, fs=fs, first_id=seed)[0]
        row.setflags(write=False)
        _inputs[key] = row
    return _inputs[key]


def case_setup(pkg, case):
    """dict(shape, taps, ns, pilot_min, iq [ns, NBYTES], names, cycles, ctaps [ns, 2T], rot [ns]) of a case"""
    name, ns, kind = case
    shape = SHAPES[name]
    T, D = shape[0], shape[1]
    fs, idx = fs_of(D), CASES.index(case)
    classes = ("station", "carrier", "const") if kind == "signal" else ("random",)
    names = [classes[s % len(classes)] for s in range(ns)]
    cycles = [OFFSETS[(s + idx) % len(OFFSETS)] for s in range(ns)]
    iq = np.stack([stream_input(pkg, names[s], cycles[s], fs, NBYTES // 2, 7000 + 10 * idx + s) for s in range(ns)])
    h = shape_taps(pkg, shape)[0]
    ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cycles])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cycles], np.float32)
    return dict(shape=shape, taps=shape_taps(pkg, shape), ns=ns, pilot_min=0.05 if kind == "signal" else 1e3, iq=iq, names=names, cycles=cycles,
                ctaps=ctaps, rot=rot)


def case_reference(pkg, case):
    """(setup, per-stream references: tuned_ref.bcast_ref on the definition's tuned d), computed once"""
    if case not in _refs:
        su = case_setup(pkg, case)
        T, D, P, Ta, Da, Tr, Dr = su["shape"]
        h, ga, gr, b, dg, rg = su["taps"]
        refs = []
        for s in range(su["ns"]):
            d = tuned_ref.tuned_d(su["iq"][s], su["ctaps"][s], su["rot"][s], D)
            refs.append(dict(tuned_ref.bcast_ref(d, b, ga, gr, su["pilot_min"], dg, rg, Da, Dr), d=d))
        _refs[case] = (su, refs)
    return _refs[case]


def case_keeps(su, refs):
    """(fraction of the case's outputs whose window holds a d at the gate, per-stream keep masks of the audio and of the RDS outputs, the
    per-stream counts of d's at the gate)"""
    T, D, P, Ta, Da, Tr, Dr = su["shape"]
    keep_a, keep_r, n_amb, bad, total = [], [], [], 0, 0
    for r in refs:
        amb = tuned_ref.ambiguous(r["rds"])
        ka = tuned_ref.clean_outputs(amb, r["L"].size, Ta, Da)
        kr = tuned_ref.clean_outputs(amb, r["bb"].size, Tr, Dr)
        keep_a.append(ka)
        keep_r.append(kr)
        n_amb.append(int(amb.sum()))
        bad += int((~ka).sum()) + int((~kr).sum())
        total += ka.size + kr.size
    return (bad / total if total else 0.0), keep_a, keep_r, n_amb


# ---- the three-station capture: one 2.4 MS/s row, stations at -400, +100 and +600 kHz, amplitude 40 each, about 1.05 s
STATIONS = [dict(offset_hz=-400e3, left_hz=1e3, right_hz=3.1e3, pi=0x3101, ps="WEST 400"),
            dict(offset_hz=+100e3, left_hz=700.0, right_hz=2.3e3, pi=0x3102, ps="MID +100"),
            dict(offset_hz=+600e3, left_hz=1.5e3, right_hz=4.1e3, pi=0x3103, ps="EAST 600")]
STATIONS_SAMPLES = 2520000
# L/R separation of the three stations through tests/tuned_ref.py (dB, the smaller of the separation in L and in R), as
# tests/test_tuned_ref.py measures and asserts it; the GPU test asserts these figures minus 1 dB
STATIONS_SEPARATION_DB = (40.53, 41.01, 40.60)

_capture = []


def three_stations(pkg):
    """(iq [1, 2 STATIONS_SAMPLES], per-station dicts with `groups` added), made once"""
    if not _capture:
        sts = [dict(st, amplitude=40.0, rds_phase=0.5 * k, groups=pkg.rds_encode_groups(st["pi"], st["ps"])) for k, st in enumerate(STATIONS)]
        iq = pkg.make_iq_stations(STATIONS_SAMPLES, sts, fs=2.4e6, seed=31)
        iq.setflags(write=False)
        _capture.append((iq, sts))
    return _capture[0]
