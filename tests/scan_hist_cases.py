"""What tests/test_scan_hist_ref.py (CPU) and the two GPU files of the hist call share, built without a device: the numpy
definition of a stream's deviation histogram from its d's, the count of d's the device may put on either side of a bin edge, the inputs of
the GPU cases that are held to tests/scan_ref.py from bytes, and the generated monitoring scenarios.

The GPU cases against the reference take no constant rows: a constant d of 0 sits on the edge of bin 256 and every one of its d's would be
edge-ambiguous.  Their classes are station / carrier / random from tests/tuned_cases.py and an unmodulated carrier whose d sits in the
middle of a bin."""
import numpy as np

import scan_cases as sc
import scan_ref
import tuned_cases as tc

BINS, SHIFT, ZERO_BIN = 512, 18, 256
TOL_D = 1e-5                                                    # the project's device-against-reference bound on d (radians)
EDGE_CAP = 0.004                                                # of a stream's d's
Q24 = np.float32(2.0 ** 24)


def hist_of(d):
    """the definition: the bincount of floor(rint(d 2^24) / 2^18) + 256 over float32 d's"""
    d = np.asarray(d, np.float32)
    return np.bincount((np.rint(d * Q24).astype(np.int64) >> SHIFT) + ZERO_BIN, minlength=BINS).astype(np.uint64)


def near_edge(d, tol=TOL_D):
    """per interior bin edge e = 1 .. BINS - 1 (the lower edge of bin e, (e - 256) / 64 rad): how many d's lie within tol of it; int64 [BINS],
    entry 0 unused"""
    d = np.asarray(d, np.float64)
    k = np.rint(d * 64.0)                                           # the nearest edge, in 1/64 rad
    hit = np.abs(d - k / 64.0) <= tol
    return np.bincount((k[hit].astype(np.int64) + ZERO_BIN).clip(0, BINS - 1), minlength=BINS)


def edge_share(d, tol=TOL_D):
    """the share of d's within tol of a bin edge (a smooth density gives 2 tol 64 = 0.13 %)"""
    d = np.asarray(d, np.float64)
    return float((np.abs(d - np.rint(d * 64.0) / 64.0) <= tol).mean()) if d.size else 0.0


def cumulative_ok(got, want, slack):
    """for every bin edge: |cumulative device count - cumulative reference count| <= the reference d's within TOL_D of that edge; returns the
    list of edges that fail"""
    cg, cw = np.cumsum(np.asarray(got, np.int64)), np.cumsum(np.asarray(want, np.int64))
    # the counts below edge e are cum[e - 1]
    return [int(e) for e in range(1, BINS) if abs(int(cg[e - 1]) - int(cw[e - 1])) > int(slack[e])]


# ---- the unmodulated carrier: amplitude 100 at an offset whose d sits in the middle of bin `bin_`, N(0, 4) noise on the bytes
def carrier_row(cycles, fs, D, nsamp, seed, bin_=260):
    d_mid = (bin_ - ZERO_BIN + 0.5) / 64.0                          # rad per D samples
    f = cycles * fs + d_mid * fs / (2.0 * np.pi * D)
    rng = np.random.default_rng(seed)
    z = 100.0 * np.exp(1j * (rng.random() * 2.0 * np.pi + 2.0 * np.pi * f / fs * np.arange(nsamp)))
    noise = rng.normal(0.0, 2.0, size=(2, nsamp))
    row = np.empty(2 * nsamp, np.uint8)
    row[0::2] = np.clip(np.rint(127.5 + z.real + noise[0]), 0, 255)
    row[1::2] = np.clip(np.rint(127.5 + z.imag + noise[1]), 0, 255)
    return row


# ---- the GPU cases held to scan_ref from bytes: (shape name, classes of the streams); stream s is tuned to OFFSETS[(s + index) % 5]
TUNED_CASES = [("default", ("station", "carrier", "random", "unmodulated", "station", "unmodulated", "random")),
               ("T7-D3-P5", ("station", "unmodulated", "random")),
               ("T16-D8", ("unmodulated", "carrier", "random"))]
_tuned = {}


def tuned_case(pkg, case):
    """dict(shape, ns, names, cycles, iq [ns, NBYTES], h, b, ctaps, rot, refs: scan_ref.scan_ref of every row), made once"""
    if case not in _tuned:
        name, names = case
        shape = sc.SHAPES[name]
        T, D, P = shape
        fs, idx, ns = tc.fs_of(D), TUNED_CASES.index(case), len(names)
        cycles = [sc.OFFSETS[(s + idx) % len(sc.OFFSETS)] for s in range(ns)]
        rows = []
        for s in range(ns):
            if names[s] == "unmodulated":
                rows.append(carrier_row(cycles[s], fs, D, sc.NBYTES // 2, 9100 + 10 * idx + s, bin_=260 - 9 * s))
            else:
                rows.append(tc.stream_input(pkg, names[s], cycles[s], fs, sc.NBYTES // 2, 9000 + 10 * idx + s))
        iq = np.stack(rows)
        iq.setflags(write=False)
        h, b = sc.shape_taps(pkg, shape)
        ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cycles])
        rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cycles], np.float32)
        refs = [scan_ref.scan_ref(iq[s], ctaps[s], rot[s], D, b, 0.05) for s in range(ns)]
        _tuned[case] = dict(shape=shape, ns=ns, names=list(names), cycles=cycles, iq=iq, h=h, b=b, ctaps=ctaps, rot=rot, refs=refs)
    return _tuned[case]


# ---- the monitoring scenarios: 0.1 s at 2.4 MS/s, D = 10, one stream each, tuned to `tuned_hz`
FS, D, SCENARIO_SAMPLES = 2.4e6, 10, 240000
SCENARIO_WARM = 8                                                # d's left out at the start: the channel filter fills from an empty history there
SCENARIOS = {                                                    # name -> (station or None, tuned_hz, seed)
    "tone-50kHz": (dict(offset_hz=200e3, tone_hz=1e3, peak_hz=50e3), 200e3, 51),
    "tone-75kHz": (dict(offset_hz=-300e3, tone_hz=1e3, peak_hz=75e3), -300e3, 52),
    "offset+7kHz": (dict(offset_hz=407e3, tone_hz=1e3, peak_hz=50e3), 400e3, 53),
    "noise-only": (None, 100e3, 54),
}
_scen = {}


def scenario(pkg, name):
    """dict(row, tuned_hz, truth: the station's dict or None, ref: scan_ref.scan_ref of the row, meters: the reference's record as a
    METER_DTYPE array [1], hist: uint64 [1, 512]), made once; record and histogram are those of the d's from SCENARIO_WARM on — d[1] and
    d[2] of a stream that starts from an empty history are a jump of about +-pi, which a monitor leaves out by dropping its first call.  A
    mono station with one tone on both channels has m = 0.87 sin: its deviation_hz is peak_hz / 0.87."""
    if name not in _scen:
        st, tuned_hz, seed = SCENARIOS[name]
        sts = [] if st is None else [dict(offset_hz=st["offset_hz"], amplitude=100.0, left_hz=st["tone_hz"], right_hz=st["tone_hz"], groups=[], pilot=False,
                                          deviation_hz=st["peak_hz"] / 0.87)]
        row = pkg.make_iq_stations(SCENARIO_SAMPLES, sts, fs=FS, seed=seed)[0]
        row.setflags(write=False)
        h, b = sc.shape_taps(pkg, sc.SHAPES["default"])
        ref = scan_ref.scan_ref(row, pkg.tuned_channel_taps(h, tuned_hz, FS), pkg.tuned_rotation(tuned_hz, FS, D), D, b, 0.05, SCENARIO_WARM)
        meters = np.zeros(1, pkg.METER_DTYPE)
        for k, v in ref["rec"].items():
            meters[k][0] = v
        _scen[name] = dict(row=row, tuned_hz=tuned_hz, truth=st, ref=ref, meters=meters, hist=hist_of(ref["d"][SCENARIO_WARM:])[None, :])
    return _scen[name]


# ---- the step geometry of the hist kernel (Python copies of scan_hist_lds and front_step_generic in csrc/sdrfm_scan.hip)
LDS_BUDGET, HIST_LDS_BYTES = 64 << 10, 4 * BINS


def scan_lds(T, D, P, NY, NDT):
    H = P - 1
    rw = (max((NY - 1) * D + T + 4, H + NDT + 4) + 3) & ~3
    return 4 * rw + 8 * NY + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 8 * T


def hist_lds(T, D, P, NY, NDT):
    return ((scan_lds(T, D, P, NY, NDT) + 15) & ~15) + HIST_LDS_BYTES


def step_of(lds, shape):
    """(NDT, LDS bytes) of the generic kernel's step under the LDS function `lds`: the largest even NY that fits the budget"""
    ny = 1024
    while ny > 2 and lds(*shape, ny, ny - 1) > LDS_BUDGET:
        ny -= 2
    return ny - 1, lds(*shape, ny, ny - 1)


# ---- the top of the range: T = 1, D = 1, three streams of 4 MiB
TOP_SHAPE, TOP_BYTES = (1, 1, 5), 4 << 20
TOP_A, TOP_B = (255, 254), (1, 2)                                # x = (127.5, 126.5) and (-126.5, -125.5): 3.1e-5 rad short of antipodal
_top = []


def top_case():
    """iq [3, 4 MiB]: stream 0 constant bytes (d = 0 exactly: every count in bin 256); stream 1 alternates two byte pairs that are
    3.1e-5 rad short of antipodal, so d = +-(pi - 3.1e-5) in turn: the two extreme bins 457 and 54; stream 2 a full-scale phasor whose
    phase falls by 2.5 rad a sample (tests/pilot_shape_cases.py's)"""
    if not _top:
        n = TOP_BYTES // 2
        iq = np.empty((3, 2 * n), np.uint8)
        iq[0].reshape(-1, 2)[:] = (200, 60)
        iq[1].reshape(-1, 2)[0::2] = TOP_A
        iq[1].reshape(-1, 2)[1::2] = TOP_B
        z = 127.5 * np.exp(-2.5j * np.arange(n))
        iq[2, 0::2] = np.clip(np.rint(127.5 + z.real), 0, 255)
        iq[2, 1::2] = np.clip(np.rint(127.5 + z.imag), 0, 255)
        iq.setflags(write=False)
        _top.append(iq)
    return _top[0]
