"""CPU checks of the scan handle's hist call and its host side: the three symbols exported, declared and listed; every
refusal of sdrfm_scan_process_batch_hist before a device is looked for; sdrfm_scan_hist_add and sdrfm_scan_hist_report (csrc/scan.c) on
hand-made rows against float64 numpy; the Python mirror's deviation_quantile and ModulationMonitor on synthetic rows."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

NAMES = ["sdrfm_scan_process_batch_hist", "sdrfm_scan_hist_add", "sdrfm_scan_hist_report"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrfm.h")
FS, D = 2.4e6, 10
K = FS / (2.0 * 3.14159265358979323846 * D)                      # Hz per rad, as csrc/scan.c forms it
BINS = 512


def test_symbols_are_exported_declared_and_listed(pkg):
    lib = pkg.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n) and n in pkg.ABI_SYMBOLS, n
        assert re.search(r"^int\s+%s\(" % n, text, re.M), n
    decl = re.search(r"^int\s+sdrfm_scan_process_batch_hist\(([^;]*)\);", text, re.M)
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(lib.sdrfm_scan_process_batch_hist.argtypes) == 8 and args[5] == "uint32_t* hist" and args[6] == "size_t hist_stride", args
    assert re.search(r"^#define\s+SDRFM_SCAN_HIST_BINS\s+512u", text, re.M) and pkg.HIST_BINS == BINS
    assert lib.sdrfm_abi_version() == 1
    assert C.sizeof(pkg.lib.ScanHistReport) == 64 and [n for n, _ in pkg.lib.ScanHistReport._fields_][0] == "n"
    for n in ("HIST_BINS", "hist_add", "hist_edges_hz", "hist_report", "deviation_quantile", "ModulationMonitor"):
        assert hasattr(pkg, n) and n in pkg.__all__, n
    for n in ("process_batch_hist", "process_batch_hist_device"):
        assert callable(getattr(pkg.ScanDemod, n)), n


def test_refusals_come_before_a_device_is_looked_for(pkg):
    """a NULL handle whatever else is given; NULL meters, NULL hist and hist_stride 511 before the handle is looked at; then the plain call's
    own refusals in its order — unknown flags, an odd count, a count above the maximum — on a stand-in handle of zeroed memory (its maximum
    is 0), which no call may write or read further than its refusal.  Nothing is written to either output"""
    lib, L = pkg.load_library(), pkg.lib
    meters = np.full(4, 5, pkg.METER_DTYPE)
    hist = np.full((4, BINS), 9, np.uint32)
    iq = np.zeros(64, np.uint8)
    m, hp, ip = C.c_void_p(meters.ctypes.data), C.c_void_p(hist.ctypes.data), C.c_void_p(iq.ctypes.data)
    call = lib.sdrfm_scan_process_batch_hist
    assert call(None, ip, 64, 64, m, hp, BINS, 0) == L.EINVAL
    assert call(None, None, 0, 0, None, None, 0, 0) == L.EINVAL
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    assert call(h, ip, 64, 64, None, hp, BINS, 0) == L.EINVAL
    assert call(h, ip, 64, 64, m, None, BINS, 0) == L.EINVAL
    assert call(h, ip, 64, 64, m, hp, BINS - 1, 0) == L.EINVAL
    assert call(h, ip, 64, 64, m, hp, 0, 0) == L.EINVAL
    assert call(h, ip, 64, 63, m, hp, BINS - 1, 0) == L.EINVAL       # the stride's refusal before the odd count's
    assert call(h, ip, 64, 63, m, hp, BINS, L.F_OVERLAP) == L.EINVAL  # the flags' before the odd count's
    assert call(h, ip, 64, 64, m, hp, BINS, 4) == L.EINVAL
    assert call(h, ip, 64, 63, m, hp, BINS, 0) == L.EODD
    assert call(h, ip, 64, 63, m, hp, BINS, L.F_DEVICE_PTRS) == L.EODD
    assert call(h, ip, 64, 64, m, hp, BINS, 0) == L.ECAPACITY
    assert call(h, ip, 64, 2, m, hp, 520, 0) == L.ECAPACITY
    # the plain call on the same stand-in: the same statuses in the same order
    plain = lib.sdrfm_scan_process_batch
    assert plain(h, ip, 64, 63, m, L.F_OVERLAP) == L.EINVAL and plain(h, ip, 64, 63, m, 0) == L.EODD and plain(h, ip, 64, 64, m, 0) == L.ECAPACITY
    assert (meters["n"] == 5).all() and (meters["reserved"] == 5).all() and (hist == 9).all()
    assert block.raw == bytes(1 << 16)
    # the Python mirror raises the status
    scn = pkg.ScanDemod.__new__(pkg.ScanDemod)
    scn._lib, scn._h, scn.n_streams, scn.cfg = lib, None, 1, pkg.ScanConfig(pilot_coeffs=np.zeros(3, np.complex64))
    with pytest.raises(pkg.SdrfmError) as e:
        scn.process_batch_hist(np.zeros((1, 100), np.uint8))
    assert e.value.status == L.EINVAL and "sdrfm_scan_process_batch_hist" in str(e.value)


# ---- csrc/scan.c: sdrfm_scan_hist_add
def test_hist_add_sums_every_bin_in_64_bits(pkg):
    lib = pkg.load_library()
    acc = np.zeros(BINS + 1, np.uint64)
    acc[BINS] = 77                                                   # a word behind the row: not touched
    row = np.arange(BINS, dtype=np.uint32)
    row[457] = 0xFFFFFFFF
    for _ in range(3):
        assert lib.sdrfm_scan_hist_add(acc.ctypes.data, row.ctypes.data) == pkg.lib.OK
    assert np.array_equal(acc[:BINS], 3 * row.astype(np.uint64)) and int(acc[457]) == 3 * 0xFFFFFFFF and int(acc[BINS]) == 77
    assert lib.sdrfm_scan_hist_add(None, row.ctypes.data) == pkg.lib.EINVAL and lib.sdrfm_scan_hist_add(acc.ctypes.data, None) == pkg.lib.EINVAL
    a2 = np.zeros((2, BINS), np.uint64)
    h2 = np.zeros((2, BINS), np.uint32)
    h2[0, 54], h2[1, 457] = 7, 9
    pkg.hist_add(pkg.hist_add(a2, h2), h2)
    assert int(a2[0, 54]) == 14 and int(a2[1, 457]) == 18 and int(a2.sum()) == 32


# ---- csrc/scan.c: sdrfm_scan_hist_report against float64 numpy
def _report(pkg, hist, m=None, fs=FS, D_=D, limit=75e3):
    r = pkg.lib.ScanHistReport()
    hist = np.ascontiguousarray(hist, np.uint64)
    rc = pkg.load_library().sdrfm_scan_hist_report(hist.ctypes.data, None if m is None else C.addressof(m), fs, D_, limit, C.byref(r))
    return rc, r


def _meter(pkg, **kw):
    m = pkg.lib.ScanMeter()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _numpy_report(hist, centre, limit):
    """the header's definitions in float64 numpy, the edges formed as csrc/scan.c forms them"""
    hist = np.asarray(hist, np.float64)
    b = np.arange(BINS)
    lo, hi = K * ((b - 256) / 64.0) - centre, K * ((b - 255) / 64.0) - centre
    use = hist > 0
    n = hist.sum()
    return dict(peak_pos_hz=hi[use].max(), peak_neg_hz=lo[use].min(), peak_hz=max(hi[use].max(), -lo[use].min()),
                over_min=hist[use & ((lo > limit) | (hi <= -limit))].sum() / n, over_max=hist[use & ((hi > limit) | (lo < -limit))].sum() / n)


def _row(**bins):
    h = np.zeros(BINS, np.uint64)
    for b, v in bins.items():
        h[int(b[1:])] = v
    return h


def test_report_of_a_single_bin(pkg):
    h = _row(b300=5)
    rc, r = _report(pkg, h)
    assert rc == pkg.lib.OK and r.n == 5
    centre = K * (44.5 / 64.0)                                       # the bin's middle
    assert r.centre_hz == pytest.approx(centre, rel=1e-13)
    assert r.peak_pos_hz == pytest.approx(K / 128.0, rel=1e-9) and r.peak_neg_hz == pytest.approx(-K / 128.0, rel=1e-9) and r.peak_hz == pytest.approx(K / 128.0, rel=1e-9)
    assert r.over_min == 0.0 and r.over_max == 0.0 and math.isnan(r.mpx_power_dbr)
    # with the record: the centre is the record's mean d, operation for operation sdrfm_scan_report's freq_err_hz
    m = _meter(pkg, n=5, freq_q=5 * 11665408, dev_q=5 * 8111104)    # d = 0.6953125 rad each (44.5 / 64): dq = d 2^24, e 2^24 = d^2 2^24 rounded
    rc, r = _report(pkg, h, m)
    rep = pkg.lib.ScanReport()
    assert pkg.load_library().sdrfm_scan_report(C.addressof(m), FS, D, 1.0, C.byref(rep)) == pkg.lib.OK
    assert rc == pkg.lib.OK and r.centre_hz == rep.freq_err_hz == pytest.approx(centre, rel=1e-13)
    want = _numpy_report(h, r.centre_hz, 75e3)
    assert all(getattr(r, k) == v for k, v in want.items()), (want, r.peak_pos_hz, r.peak_neg_hz)
    assert r.mpx_power_dbr == (10.0 * math.log10(2.0 * rep.dev_rms_hz ** 2 / 19000.0 ** 2) if rep.dev_rms_hz > 0 else -math.inf)


def test_report_of_both_extreme_bins(pkg):
    h = _row(b54=3, b457=1)
    rc, r = _report(pkg, h)
    centre = K * ((3 * (54 - 255.5) + (457 - 255.5)) / 64.0 / 4.0)
    assert rc == pkg.lib.OK and r.n == 4 and r.centre_hz == pytest.approx(centre, rel=1e-13)
    want = _numpy_report(h, r.centre_hz, 75e3)
    assert all(getattr(r, k) == v for k, v in want.items()), want
    assert r.peak_pos_hz == K * (202 / 64.0) - r.centre_hz and r.peak_neg_hz == K * (-202 / 64.0) - r.centre_hz
    assert r.peak_hz == r.peak_pos_hz > 170e3 and r.over_min == 0.25 and r.over_max == 0.25         # bin 54 lies 60.1 kHz below the centre
    # with a record whose mean d is 0: both bins wholly outside +-75 kHz (they begin 120 kHz out)
    m = _meter(pkg, n=4, freq_q=0, dev_q=4 * (9 << 24))
    rc, r = _report(pkg, h, m)
    assert rc == pkg.lib.OK and r.centre_hz == 0.0 and r.peak_pos_hz == K * (202 / 64.0) == -r.peak_neg_hz == r.peak_hz
    assert r.over_min == 1.0 and r.over_max == 1.0
    assert r.mpx_power_dbr == pytest.approx(10 * math.log10(2 * (3 * K) ** 2 / 19000.0 ** 2), rel=1e-12)


def test_report_of_no_d_and_refused_arguments(pkg):
    rc, r = _report(pkg, np.zeros(BINS, np.uint64))
    assert rc == pkg.lib.OK and r.n == 0
    assert all(math.isnan(getattr(r, f)) for f, _ in pkg.lib.ScanHistReport._fields_[1:])
    rc, r = _report(pkg, np.zeros(BINS, np.uint64), _meter(pkg))
    assert rc == pkg.lib.OK and r.n == 0 and math.isnan(r.mpx_power_dbr) and math.isnan(r.centre_hz)
    h = _row(b256=2)
    lib = pkg.load_library()
    out = pkg.lib.ScanHistReport()
    assert lib.sdrfm_scan_hist_report(None, None, FS, D, 75e3, C.byref(out)) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_hist_report(h.ctypes.data, None, FS, D, 75e3, None) == pkg.lib.EINVAL
    for kw in (dict(D_=0), dict(fs=0.0), dict(fs=-1.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(limit=-1.0), dict(limit=float("nan")),
               dict(limit=float("inf"))):
        assert _report(pkg, h, **kw)[0] == pkg.lib.EINVAL, kw
    assert _report(pkg, h, _meter(pkg, n=3))[0] == pkg.lib.EINVAL     # a record of other calls than the histogram's
    assert _report(pkg, h, _meter(pkg, n=2))[0] == pkg.lib.OK and _report(pkg, h, limit=0.0)[0] == pkg.lib.OK


def test_limits_inside_on_and_between_bin_edges(pkg):
    """a record with mean d 0 puts the centre at 0 exactly, so a limit of K (j / 64) lies on the edge between bins 255 + j and 256 + j; a
    deviation is outside iff it is MORE than the limit from the centre, and a bin holds its lower edge and not its upper one"""
    h = _row(b246=1, b266=2, b267=4, b245=8, b256=16)                # edges in 1/64 rad: [-10, -9) [10, 11) [11, 12) [-11, -10) [0, 1)
    m = _meter(pkg, n=31, freq_q=0, dev_q=31 << 10)
    edge = lambda j: K * (j / 64.0)
    cases = {
        "inside bin 266 (and bin 245)": (0.5 * (edge(10) + edge(11)), 4, 4 + 2 + 8),
        "on the edge 10": (edge(10), 4 + 8, 4 + 2 + 8),                 # bin 266 holds d = limit itself: partly; bin 246 = [-10, -9) holds -limit and nothing beyond: not
        "on the edge 11": (edge(11), 0, 4),                           # bin 267 holds its lower edge: partly; bin 245 = [-11, -10) holds -limit and nothing beyond: not
        "between: inside bin 256": (edge(0.5), 1 + 2 + 4 + 8, 31),
        "zero": (0.0, 1 + 2 + 4 + 8, 31),                             # bin 256 = [0, 1): d = 0 is not outside, the rest of it is
        "beyond everything": (edge(13), 0, 0),
        "on the edge 12": (edge(12), 0, 0),
    }
    for name, (limit, wholly, partly) in cases.items():
        rc, r = _report(pkg, h, m, limit=limit)
        want = _numpy_report(h, 0.0, limit)
        assert rc == pkg.lib.OK and r.centre_hz == 0.0, name
        assert (r.over_min, r.over_max) == (wholly / 31.0, partly / 31.0) == (want["over_min"], want["over_max"]), (name, r.over_min * 31, r.over_max * 31)
        assert r.peak_pos_hz == edge(12) and r.peak_neg_hz == edge(-11) and r.peak_hz == edge(12)
    # m NULL against m given on the same row: the centre moves from the record's mean to the histogram's, the peaks with it
    rc, r0 = _report(pkg, h)
    mid = K * (float((h.astype(np.float64) * (np.arange(BINS) - 255.5)).sum()) / 64.0 / 31.0)
    assert rc == pkg.lib.OK and r0.centre_hz == pytest.approx(mid, rel=1e-13) and r0.peak_pos_hz == edge(12) - r0.centre_hz and math.isnan(r0.mpx_power_dbr)
    want = _numpy_report(h, r0.centre_hz, 75e3)
    assert all(getattr(r0, k) == v for k, v in want.items()), want


def test_python_hist_report_and_edges(pkg):
    e = pkg.hist_edges_hz(FS, D)
    assert e.shape == (BINS + 1,) and e[256] == 0.0 and e[257] == pytest.approx(596.83, abs=0.01) and np.allclose(np.diff(e), K / 64.0, rtol=1e-12)
    h = np.zeros((3, BINS), np.uint32)
    h[0, 300], h[1, 54], h[1, 457] = 5, 3, 1
    rep = pkg.hist_report(h, None, FS, D)
    assert list(rep["n"]) == [5, 4, 0] and rep["peak_hz"][0] == pytest.approx(K / 128.0, rel=1e-9) and np.isnan(rep["peak_hz"][2])
    m = np.zeros(3, pkg.METER_DTYPE)
    m["n"] = (5, 4, 0)
    rep = pkg.hist_report(h, m, FS, D, limit_hz=100e3)
    assert rep["centre_hz"][0] == 0.0 and rep["over_min"][1] == 1.0 and rep["mpx_power_dbr"][0] == -np.inf
    m["n"][0] = 6
    with pytest.raises(pkg.SdrfmError) as err:
        pkg.hist_report(h, m, FS, D)
    assert err.value.status == pkg.lib.EINVAL


def test_deviation_quantile_brackets_the_truth(pkg):
    """known d's -> their histogram; the bracket holds the quantile of |f - centre| computed from the d's themselves"""
    rng = np.random.default_rng(5)
    d = np.concatenate([0.9 * np.sin(np.linspace(0, 40, 20000)) + 0.05, rng.normal(0.05, 0.01, 5000)]).astype(np.float32)
    dq = np.rint(d * np.float32(2.0 ** 24)).astype(np.int64)
    hist = np.bincount((dq >> 18) + 256, minlength=BINS).astype(np.uint32)[None, :]
    m = np.zeros(1, pkg.METER_DTYPE)
    m["n"], m["freq_q"] = d.size, int(dq.sum())
    centre = pkg.hist_report(hist, m, FS, D)["centre_hz"][0]
    dev = np.abs(K * dq.astype(np.float64) / 2.0 ** 24 - centre)
    for share in (0.0, 1e-4, 0.01, 0.1, 0.5, 0.999, 1.0):
        lo, hi = pkg.deviation_quantile(hist, m, FS, D, share)
        v = np.sort(dev)
        true = v[int(np.argmax((v.size - 1 - np.arange(v.size)) <= share * v.size))]   # the smallest value that at most share * n values exceed
        assert lo[0] <= true <= hi[0] and hi[0] - lo[0] <= 2 * K / 64.0 + 1e-9, (share, lo[0], true, hi[0])
    lo, hi = pkg.deviation_quantile(hist, m, FS, D, 0.0)
    assert hi[0] == pkg.hist_report(hist, m, FS, D)["peak_hz"][0]      # no d exceeds the peak
    lo, hi = pkg.deviation_quantile(np.zeros((2, BINS), np.uint32), None, FS, D, 0.01)
    assert np.isnan(lo).all() and np.isnan(hi).all()


def test_modulation_monitor_on_synthetic_calls(pkg):
    """three calls on two streams: stream 0 a 'station' whose second call alone passes the limit, stream 1 silent in the first call"""
    mon = pkg.ModulationMonitor(2, FS, D, limit_hz=75e3)

    def call(bins0, bins1):
        h = np.zeros((2, BINS), np.uint32)
        m = np.zeros(2, pkg.METER_DTYPE)
        for s, bins in enumerate((bins0, bins1)):
            for b, c in bins.items():
                h[s, b] = c
                m["n"][s] += c
                m["freq_q"][s] += c * (((b - 256) << 18) + (1 << 17))   # every d in the middle of its bin
                m["dev_q"][s] += c * int(round(((b - 255.5) / 64.0) ** 2 * 2 ** 24))
        return m, h

    in_ = {256 - 100: 10, 256 + 99: 10}                             # +-100 bins = +-59.7 kHz about 0
    out = {256 - 130: 10, 256 + 129: 10}                            # +-130 bins = +-77.6 kHz
    peaks = [mon.push(*call(in_, {})), mon.push(*call(out, in_)), mon.push(*call(in_, in_))]
    assert np.isnan(peaks[0][1]) and peaks[0][0] == pytest.approx(100 * K / 64.0, rel=1e-9) and peaks[1][0] == pytest.approx(130 * K / 64.0, rel=1e-9)
    s0, s1 = mon.summary()
    assert (s0["stream"], s0["n"], s0["calls"], s1["n"], s1["calls"]) == (0, 60, 3, 40, 2)
    assert s0["peak_hz"] == pytest.approx(130 * K / 64.0, rel=1e-9) and s0["calls_over"] == pytest.approx(1 / 3) and s0["over_min"] == s0["over_max"] == pytest.approx(1 / 3)
    assert s1["peak_hz"] == pytest.approx(100 * K / 64.0, rel=1e-9) and s1["calls_over"] == 0.0 and s1["over_max"] == 0.0
    assert s0["centre_hz"] == 0.0 and np.isfinite(s0["mpx_power_dbr"]) and s0["mpx_power_dbr"] > s1["mpx_power_dbr"]
    assert int(mon.hist.sum()) == 100 and mon.hist.dtype == np.uint64 and int(mon.meters["n"].sum()) == 100
    empty = pkg.ModulationMonitor(1, FS, D).summary()[0]
    assert empty["n"] == 0 and empty["calls"] == 0 and math.isnan(empty["peak_hz"]) and math.isnan(empty["over_max"])
