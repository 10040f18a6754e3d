"""The cases tests/test_scan_shapes_gpu.py and tests/test_bcast_tuned_shapes_gpu.py sweep the tuned walk, the scan kernel
(§4.13) and the metered forms (§4.14) over, built without a device so that tests/test_pilot_shapes_cpu.py can look at the reference side
alone: the step geometry every shape gets (Python copies of scan_lds, bcast_lds and bcast_lds_tuned), how many outputs sit at the pilot
gate, and the magnitude case that takes a record to the top of its range.

A case is a shape.  Case k has 1, 3 or 7 streams (SCAN_STREAMS, BCAST_STREAMS); stream s is tuned to tuned_cases.OFFSETS[(s + k) % 5] cycles
per sample and its row holds, as in tuned_cases, station / carrier / const in turn at that offset where fs / D carries a station's pilot,
random / counter / const in turn where it does not.  Against the references the pilot threshold is
test_rds_shapes_gpu._pick_pilot_min's on the reference's pilot powers of the stations and carriers; without any it is 1e3, the gate shut
(the pilot powers of noise lie anywhere, so any threshold among them would have d's at it).  The comparisons that are exact on the device
alone take mid_gate's threshold instead, in the middle of the rows' powers, so that the gate is on and off in them.  A case's bytes are
a ragged sequence of calls around one long call: the smallest number of whole steps for which every stream gets three workgroups at the
least and every workgroup two full steps, whatever the kernel's occupancy (long_call_d).  More streams on a shared row do not make that
call shorter: with more streams than the device runs workgroups the split falls to one or two workgroups a stream, and below that it is
64 workgroups a stream at any stream count."""
import numpy as np

import scan_ref
import tuned_cases as tc
import tuned_ref
from test_bcast_shapes_gpu import FAST, GENERIC, _split, _taps
from test_rds_shapes_gpu import _fs, _pick_pilot_min

LDS_BUDGET, FAST_NY, MAX_CALL = 64 << 10, 1024, 4 << 20         # the host geometry of csrc/sdrfm_pilot_front.h; a metered call's bytes
CUS, PER_CU = 256, range(1, 9)                                  # the device the long call is sized for: its units, workgroups a unit may hold

SCAN_SHAPES = [(1, 1, 1), (256, 1, 1), (1, 64, 255), (255, 17, 3), (64, 16, 101), (128, 10, 101), (256, 64, 255)]      # (T, D, P)
SCAN_STREAMS = [3, 7, 3, 1, 7, 1, 7]
BCAST_SHAPES = GENERIC + [(256, 16, 255, 256, 1, 256, 1)] + FAST                                                     # (T, D, P, Ta, Da, Tr, Dr)
BCAST_STREAMS = [3, 7, 1, 3, 1, 7] + [3] + [7, 1, 3, 3, 1]
SCAN_LDS_LIMITED = [(256, 64, 255), (1, 64, 255), (255, 17, 3), (64, 16, 101)]
# what the host geometry gives by hand: shape -> (NDT, LDS bytes or None)
SCAN_STEPS = {(256, 64, 255): (223, 65040), (1, 64, 255): (235, None), (255, 17, 3): (821, 65528), (64, 16, 101): (881, None)}
BCAST_D64 = (256, 64, 255, 256, 64, 256, 64)
BCAST_D64_STEPS = {True: 201, False: 205}                       # tuned -> NDT


def scan_id(shape):
    return "T%d-D%d-P%d" % shape


def bcast_id(shape):
    return "T%d-D%d-P%d-Ta%d-Da%d-Tr%d-Dr%d" % shape


# ---- the step geometry ----------------------------------------------------------------------------------------------------------------
def scan_lds(T, D, P, NY, NDT):
    H = P - 1
    rw = (max((NY - 1) * D + T + 4, H + NDT + 4) + 3) & ~3
    return 4 * rw + 8 * NY + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 8 * T


def bcast_lds(T, D, P, Ta, Tr, NY, NDT):
    H = P - 1 + max(Ta, Tr) - 1
    zp = (Tr - 1 + NDT) | 1
    rw = (max((NY - 1) * D + T + 4, H + NDT + (Ta - 1 + NDT) + 2 * zp) + 3) & ~3
    return (4 * rw + 8 * NY + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 4 * ((Tr + 3) & ~3) + 4 * Ta + 4 * T + 8 * (Tr - 1) + 4 * (Ta - 1))


def bcast_lds_tuned(T, D, P, Ta, Tr, NY, NDT):
    return bcast_lds(T, D, P, Ta, Tr, NY, NDT) + 4 * T


def _step(lds, fast):
    """dict(NY, NDT, lds, fast) of front_step / front_step_generic: the fast kernel's fixed step where it fits, or the largest even NY
    whose LDS fits the budget"""
    if fast and lds(FAST_NY, FAST_NY - 1) <= LDS_BUDGET:
        return dict(NY=FAST_NY, NDT=FAST_NY - 1, lds=lds(FAST_NY, FAST_NY - 1), fast=True)
    ny = 1024
    while ny > 2 and lds(ny, ny - 1) > LDS_BUDGET:
        ny -= 2
    return dict(NY=ny, NDT=ny - 1, lds=lds(ny, ny - 1), fast=False)


def scan_step(shape, generic=True):
    T, D, P = shape
    return dict(_step(lambda ny, ndt: scan_lds(T, D, P, ny, ndt), not generic and shape == (64, 10, 101)), H=P - 1)


def bcast_step(shape, tuned, generic=True):
    T, D, P, Ta, Da, Tr, Dr = shape
    fn = bcast_lds_tuned if tuned else bcast_lds
    return dict(_step(lambda ny, ndt: fn(T, D, P, Ta, Tr, ny, ndt), not generic and (T, D, P) == (64, 10, 101)), H=P - 1 + max(Ta, Tr) - 1)


def scan_name(shape, generic):
    return "scan-fast T64 D10 P101" if scan_step(shape, generic)["fast"] else "scan-generic T%d D%d P%d" % shape


def bcast_name(shape, tuned, generic):
    kind = "fast" if bcast_step(shape, tuned, generic)["fast"] else "generic"
    return "bcast-%s%s T%d D%d P%d Ta%d Da%d Tr%d Dr%d" % ((kind, "-tuned" if tuned else "") + tuple(shape))


def split_ok(M, ndt, H, ns, cus=CUS):
    """a call of M new d's gives every stream >= 3 workgroups and every workgroup >= 2 full steps, at every occupancy"""
    for per_cu in PER_CU:
        bps, span = _split(M, ndt, H, ns, per_cu * cus)
        if bps < 3 or span < 2 * ndt:
            return False
    return True


def long_call_d(ndt, H, ns):
    """the fewest whole steps' worth of new d's that split_ok takes"""
    k = 6
    while not split_ok(k * ndt, ndt, H, ns):
        k += 1
    return k * ndt


def ragged_cuts(D, H, ndt, ns, decims, seed):
    """(even byte counts, the long call's): 0, 2, calls below one output of each decimator behind d (decims: their D's), a call whose M is
    below H (where H > 0; it leaves the input phase at D - 1), 2 D + 1 samples (D > 1: a phase != 0), a second 0, the long call, three
    random ones"""
    cuts = [0, 2] + [2 * D * dd - 4 for dd in decims if D * dd > 2]
    if H >= 4:
        cuts.append(2 * D * (H // 2) - 2)
    if D > 1:
        cuts.append(2 * (2 * D + 1))
    long_ = 2 * D * long_call_d(ndt, H, ns)
    cuts += [0, long_]
    rng = np.random.default_rng(seed)
    cuts += [int(v) for v in 2 * rng.integers(1, D * min(ndt, 300), 3)]
    assert all(c >= 0 and c % 2 == 0 for c in cuts) and sum(cuts) <= MAX_CALL, (cuts, sum(cuts))
    return cuts, long_


def pilot_taps(pkg, shape):
    """b of a shape: the pilot band-pass at fs / D, the unit tap where P = 1"""
    return _taps(pkg, shape[0], shape[1], shape[2], 1, 1)[3]


# ---- inputs, tunings, thresholds -----------------------------------------------------------------------------------------------------
def _classes(D):
    return ("station", "carrier", "const") if _fs(D) / D >= 120e3 else ("random", "counter", "const")


def _front(pkg, T, D, ns, idx, nsamp, seed0):
    """names, cycles per sample, rows, ctaps and rot of a case's streams"""
    fs, classes = _fs(D), _classes(D)
    names = [classes[s % len(classes)] for s in range(ns)]
    cycles = [tc.OFFSETS[(s + idx) % len(tc.OFFSETS)] for s in range(ns)]
    iq = np.stack([tc.stream_input(pkg, names[s], cycles[s], fs, nsamp, seed0 + 10 * idx + s) for s in range(ns)])
    h = pkg.lowpass_taps(T, min(120e3 / fs, 0.45))
    ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cycles])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cycles], np.float32)
    return names, cycles, iq, h, ctaps, rot


def _place(names, pws):
    """the threshold against the references: _pick_pilot_min on the stations and carriers — it lies in the widest gap of their pooled
    powers, which is between two streams' —, tuned_cases' 0.05 for a station alone (a gap of one station's powers is inside its pilot's
    ripple), 1e3 (the gate shut) without any"""
    use = [p for p, c in zip(pws, names) if c in ("station", "carrier")]
    if len(use) == 1:
        return 0.05
    return float(_pick_pilot_min(use)) if use else 1e3


def mid_gate(names, pws):
    """a threshold in the middle of the rows' pilot powers (the constant rows left out where there are others): _pick_pilot_min's rule"""
    return float(_pick_pilot_min([p for p, c in zip(pws, names) if c != "const" and (p > 0).sum() >= 4] or pws))


def offset_zero_gate(case, b):
    """mid_gate on the reference's pilot powers of a case's rows at offset 0: taps (h, 0), rot 0"""
    D = case["shape"][1]
    hz = tuned_ref.pairs(case["h"])
    return mid_gate(case["names"], [scan_ref.scan_ref(row, hz, 0.0, D, b, 1.0)["pw"] for row in case["iq"]])


def _with_gate(r, pilot_min):
    """a scan_ref result at another threshold: n_pilot alone depends on it"""
    pmin2 = np.float32(pilot_min) * np.float32(pilot_min)
    return dict(r, pmin2=pmin2, rec=dict(r["rec"], n_pilot=int((r["pw"] >= pmin2).sum())))


_scan, _bcast, _mag = {}, {}, []


def scan_case(pkg, shape):
    """dict(shape, idx, fs, ns, names, cycles, iq [ns, bytes], h, b, ctaps, rot, cuts, long, step, pilot_min, refs: scan_ref.scan_ref of
    every stream's whole row), made once"""
    if shape not in _scan:
        T, D, P = shape
        idx = SCAN_SHAPES.index(shape)
        ns, step = SCAN_STREAMS[idx], scan_step(shape)
        cuts, long_ = ragged_cuts(D, step["H"], step["NDT"], ns, (), 600 + idx)
        names, cycles, iq, h, ctaps, rot = _front(pkg, T, D, ns, idx, sum(cuts) // 2, 7600)
        b = pilot_taps(pkg, shape)
        refs = [scan_ref.scan_ref(iq[s], ctaps[s], rot[s], D, b, 1.0) for s in range(ns)]
        pm = _place(names, [r["pw"] for r in refs])
        _scan[shape] = dict(shape=shape, idx=idx, fs=_fs(D), ns=ns, names=names, cycles=cycles, iq=iq, h=h, b=b, ctaps=ctaps, rot=rot, cuts=cuts,
                            long=long_, step=step, pilot_min=pm, refs=[_with_gate(r, pm) for r in refs])
    return _scan[shape]


def scan_shares(case):
    """per stream: the share of its d's at the gate"""
    return [float(scan_ref.ambiguous(r["pw"], r["pmin2"]).mean()) for r in case["refs"]]


def bcast_case(pkg, shape):
    """dict(shape, idx, fs, ns, names, cycles, iq, taps: (h, ga, gr, b, dg, rg), ctaps, rot, cuts, long, steps: {tuned: step}, pilot_min,
    refs: tuned_ref.bcast_ref on the definition's tuned d, with d), made once; the keys tuned_cases.case_keeps reads are there"""
    if shape not in _bcast:
        T, D, P, Ta, Da, Tr, Dr = shape
        idx = BCAST_SHAPES.index(shape)
        ns, fs = BCAST_STREAMS[idx], _fs(D)
        steps = {tuned: bcast_step(shape, tuned) for tuned in (False, True)}
        # sized on the untuned step (the larger one): the tuned walk's workgroups then take two full steps of theirs as well
        cuts, long_ = ragged_cuts(D, steps[False]["H"], steps[False]["NDT"], ns, (Da, Dr), 700 + idx)
        names, cycles, iq, h, ctaps, rot = _front(pkg, T, D, ns, idx, sum(cuts) // 2, 7800)
        _, ga, gr, b = _taps(pkg, T, D, P, Ta, Tr)
        dg, rg = float(pkg.stereo_diff_gain(D, fs)), float(pkg.rds_gain(D, fs)) if fs / D >= 120e3 else 2.0
        pws = [scan_ref.scan_ref(iq[s], ctaps[s], rot[s], D, b, 1.0)["pw"] for s in range(ns)]
        pm = _place(names, pws)
        refs = []
        for s in range(ns):
            d = tuned_ref.tuned_d(iq[s], ctaps[s], rot[s], D)
            refs.append(dict(tuned_ref.bcast_ref(d, b, ga, gr, pm, dg, rg, Da, Dr), d=d))
        _bcast[shape] = dict(shape=shape, idx=idx, fs=fs, ns=ns, names=names, cycles=cycles, iq=iq, taps=(h, ga, gr, b, dg, rg), h=h, ctaps=ctaps,
                             rot=rot, cuts=cuts, long=long_, steps=steps, pilot_min=pm, refs=refs)
    return _bcast[shape]


# ---- the record at the top of its range ----------------------------------------------------------------------------------------------
MAG_SHAPE, MAG_BCAST_SHAPE = (1, 1, 5), (1, 1, 5, 1, 1, 1, 1)
MAG_WARM, MAG_BYTES = 2 * 8, 4 << 20                            # a first call that fills the pilot filter's history, then the 4 MiB call
MAG_GATES = (1e-18, 1e3)                                        # every d passes, none does


def magnitude_case(pkg):
    """Two streams of MAG_WARM + MAG_BYTES bytes at T = 1, D = 1, P = 5 with the taps on the refusal bounds — h = 16, so sum(|hr| + |hi|) is
    16, and b = (2, -2, 2, -1, 1), so sum(|br| + |bi|) is 8, all exact in fp32 — at offset 0.  Stream 0 alternates between the byte pairs
    (255, 255) and (0, 19): two full-scale phasors 3.06 rad apart, d = +-3.06 in turn, q = 8 d.  Stream 1 is a full-scale phasor whose
    phase falls by 2.5 rad a sample: d = -2.5, q = 2 d.  dict(h, b, ctaps, rot, iq [2, bytes], refs: scan_ref.scan_ref of the second
    call's d's at MAG_GATES[0]), made once."""
    if not _mag:
        n = (MAG_WARM + MAG_BYTES) // 2
        iq = np.empty((2, 2 * n), np.uint8)
        iq[0].reshape(-1, 2)[0::2] = (255, 255)
        iq[0].reshape(-1, 2)[1::2] = (0, 19)
        z = 127.5 * np.exp(-2.5j * np.arange(n))
        iq[1, 0::2] = np.clip(np.rint(127.5 + z.real), 0, 255)
        iq[1, 1::2] = np.clip(np.rint(127.5 + z.imag), 0, 255)
        iq.setflags(write=False)
        h, b = np.array([16.0], np.float32), np.array([2, -2, 2, -1, 1], np.complex64)
        ctaps, rot = np.tile(tuned_ref.pairs(h), (2, 1)), np.zeros(2, np.float32)
        refs = [scan_ref.scan_ref(iq[s], ctaps[s], 0.0, 1, b, MAG_GATES[0], MAG_WARM // 2, n) for s in range(2)]
        _mag.append(dict(h=h, b=b, ctaps=ctaps, rot=rot, iq=iq, refs=refs))
    return _mag[0]
