"""The cases tests/test_bcast_retune_gpu.py holds a re-tuned broadcast handle to tests/retune_ref.py on, built without a
device so that tests/test_retune_ref.py can look at the reference side alone (how many of a case's outputs sit at the pilot gate).

A case is (shape, streams, kind) on the shapes, classes, pilot_min and NBYTES of tests/tuned_cases.py.  Stream s holds its class at the
NEW offset and starts tuned DELTAS[s % 3] away from it: 5 kHz below, 7 kHz above, or 2 kHz below fs / (2 D) with the new offset 2 kHz
above it, where rot crosses +-pi.  One event re-tunes every stream after N0 input samples: all three phases of the handle are non-zero
there at every shape."""
import numpy as np

import retune_ref
import tuned_cases as tc

CASES = [("default", 3, "signal"), ("default", 7, "signal"), ("default", 1, "random"), ("T7-D3-P5", 7, "signal"), ("T16-D8", 3, "signal"),
         ("Ta>Tr", 3, "signal"), ("Ta>Tr", 1, "random")]
N0 = 30029                                                      # input samples before the event: m0 = 3002 / 10009 / 3753 at D = 10 / 3 / 8
DELTAS = ("+5k", "-7k", "wrap")
BASE = (0.0417, -0.1667, 0.25)                                  # cycles per sample of the new offset where it is not the wrap's

_setups, _refs = {}, {}


def case_id(case):
    return "%s-%dstreams-%s" % case


def phases(shape, n0=N0):
    """(input phase, audio decimator phase, RDS decimator phase) after n0 samples"""
    T, D, P, Ta, Da, Tr, Dr = shape
    return n0 % D, (n0 // D) % Da, (n0 // D) % Dr


def offsets(shape, s):
    """(old, new) offset in Hz of stream s"""
    D = shape[1]
    fs, kind = tc.fs_of(D), DELTAS[s % 3]
    if kind == "wrap":
        return fs / (2 * D) - 2e3, fs / (2 * D) + 2e3
    new = BASE[(s // 3) % len(BASE)] * fs
    return (new - 5e3, new) if kind == "+5k" else (new + 7e3, new)


def case_setup(pkg, case):
    """dict(shape, taps, ns, pilot_min, iq [ns, NBYTES], names, old_hz, new_hz, old / new: (ctaps [ns, 2T], rot [ns]), carry [ns, 2])"""
    if case not in _setups:
        name, ns, kind = case
        shape = tc.SHAPES[name]
        T, D = shape[0], shape[1]
        fs, idx = tc.fs_of(D), CASES.index(case)
        assert all(phases(shape)), phases(shape)
        classes = ("station", "carrier", "const") if kind == "signal" else ("random",)
        names = [classes[(s + idx) % len(classes)] for s in range(ns)]
        old_hz, new_hz = (np.array(v) for v in zip(*[offsets(shape, s) for s in range(ns)]))
        iq = np.stack([tc.stream_input(pkg, names[s], new_hz[s] / fs, fs, tc.NBYTES // 2, 7500 + 10 * idx + s) for s in range(ns)])
        taps = tc.shape_taps(pkg, shape)
        tune = lambda off: (np.stack([pkg.tuned_channel_taps(taps[0], f, fs) for f in off]),
                            np.array([pkg.tuned_rotation(f, fs, D) for f in off], np.float32))
        carry = np.stack([pkg.retune_carry(o, n, T, fs) for o, n in zip(old_hz, new_hz)])
        _setups[case] = dict(shape=shape, taps=taps, ns=ns, pilot_min=0.05 if kind == "signal" else 1e3, iq=iq, names=names, old_hz=old_hz,
                             new_hz=new_hz, old=tune(old_hz), new=tune(new_hz), carry=carry)
    return _setups[case]


def case_reference(pkg, case, with_carry, restart=()):
    """(setup, per-stream retune_ref.retune_bcast results) of the case's one event, with the carry of taps.retune_carry or with (1, 0);
    the streams in `restart` restart there instead.  Computed once."""
    key = (case, bool(with_carry), tuple(restart))
    if key not in _refs:
        su = case_setup(pkg, case)
        refs = []
        for s in range(su["ns"]):
            ev = retune_ref.event(su["new"][0][s], su["new"][1][s], n0=N0, carry=su["carry"][s] if with_carry else (1.0, 0.0), restart=s in restart)
            refs.append(retune_ref.retune_bcast(su["iq"][s], su["shape"], su["taps"], su["pilot_min"], [ev], hz=su["old"][0][s], rot=su["old"][1][s]))
        _refs[key] = (su, refs)
    return _refs[key]


def excluded(refs):
    """the share of the outputs whose window holds a d at the gate"""
    bad = sum(int((~r["keep_a"]).sum()) + int((~r["keep_r"]).sum()) for r in refs)
    total = sum(r["keep_a"].size + r["keep_r"].size for r in refs)
    return bad / total if total else 0.0


def two_step_reference(pkg, case):
    """(setup, halfway (ctaps, rot), the two carries, per-stream references) of old -> halfway -> new with both events at N0; the wrap
    stream's halfway rotation is pi itself.  Computed once."""
    key = (case, "two-step")
    if key not in _refs:
        su = case_setup(pkg, case)
        shape = su["shape"]
        T, D = shape[0], shape[1]
        fs, h = tc.fs_of(D), su["taps"][0]
        mid_hz = (su["old_hz"] + su["new_hz"]) / 2
        mid = (np.stack([pkg.tuned_channel_taps(h, f, fs) for f in mid_hz]), np.array([pkg.tuned_rotation(f, fs, D) for f in mid_hz], np.float32))
        c1 = np.stack([pkg.retune_carry(o, m, T, fs) for o, m in zip(su["old_hz"], mid_hz)])
        c2 = np.stack([pkg.retune_carry(m, n, T, fs) for m, n in zip(mid_hz, su["new_hz"])])
        refs = [retune_ref.retune_bcast(su["iq"][s], shape, su["taps"], su["pilot_min"],
                                        [retune_ref.event(mid[0][s], mid[1][s], n0=N0, carry=c1[s]),
                                         retune_ref.event(su["new"][0][s], su["new"][1][s], n0=N0, carry=c2[s])],
                                        hz=su["old"][0][s], rot=su["old"][1][s]) for s in range(su["ns"])]
        _refs[key] = (su, mid, (c1, c2), refs)
    return _refs[key]


def follow_reference(pkg, row, tuned_hz, chosen_hz, n0, pilot_min):
    """per-stream references of the end-to-end case: the default shape's streams on one row, tuned to tuned_hz and moved to chosen_hz with
    the carry of taps.retune_carry after n0 samples"""
    shape = tc.SHAPES["default"]
    T, D = shape[0], shape[1]
    taps, fs = tc.shape_taps(pkg, shape), tc.fs_of(D)
    refs = []
    for old, new in zip(tuned_hz, chosen_hz):
        ev = retune_ref.event(pkg.tuned_channel_taps(taps[0], new, fs), pkg.tuned_rotation(new, fs, D), n0=n0, carry=pkg.retune_carry(old, new, T, fs))
        refs.append(retune_ref.retune_bcast(row, shape, taps, pilot_min, [ev], hz=pkg.tuned_channel_taps(taps[0], old, fs),
                                            rot=pkg.tuned_rotation(old, fs, D)))
    return refs
