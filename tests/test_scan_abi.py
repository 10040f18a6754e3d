"""CPU checks of the sdrfm_scan_* C-ABI: exported, every invalid configuration refused before a device is looked for, NULL handles
harmless, and the two host-only functions of csrc/scan.c (sdrfm_scan_report, sdrfm_scan_meter_add) on hand-made records."""
import ctypes as C
import math

import numpy as np
import pytest

NAMES = ["sdrfm_scan_create", "sdrfm_scan_destroy", "sdrfm_scan_reset", "sdrfm_scan_tune", "sdrfm_scan_process_batch", "sdrfm_scan_set_stream",
         "sdrfm_scan_synchronize", "sdrfm_scan_kernel_name", "sdrfm_scan_report", "sdrfm_scan_meter_add"]
T, P, NS = 64, 101, 3


def test_scan_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
    for n in ("ScanDemod", "ScanConfig", "meter_report", "find_stations", "scan_capture", "pilot_gain"):
        assert hasattr(pkg, n) and n in pkg.__all__, n
    assert C.sizeof(pkg.lib.ScanMeter) == 64 == pkg.METER_DTYPE.itemsize
    assert [n for n, _ in pkg.lib.ScanMeter._fields_] == list(pkg.METER_DTYPE.names)


def _cfg(pkg, keep, **kw):
    lib = pkg.lib
    h = pkg.lowpass_taps(T, 120e3 / 2.4e6)
    ctaps = np.stack([pkg.tuned_channel_taps(h, f, 2.4e6) for f in (-400e3, 100e3, 600e3)])
    rot = np.array([pkg.tuned_rotation(f, 2.4e6, 10) for f in (-400e3, 100e3, 600e3)], np.float32)
    b = np.zeros(2 * P, np.float32)
    bz = pkg.stereo_pilot_taps(P, 240e3)
    b[0::2], b[1::2] = bz.real, bz.imag
    vals = dict(n_streams=NS, fir_taps=T, fir_decim=10, ctaps=ctaps, rot=rot, pilot_taps=P, b=b, pilot_min=0.05, max_bytes_per_call=0, device=0,
                flags=0, struct_size=C.sizeof(lib.ScanConfig))
    vals.update(kw)
    fp = C.POINTER(C.c_float)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    cc, rr, bb = arr(vals["ctaps"]), arr(vals["rot"]), arr(vals["b"])
    keep += [cc, rr, bb]
    ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
    c = lib.ScanConfig()
    c.struct_size, c.n_streams, c.fir_taps, c.fir_decim = vals["struct_size"], vals["n_streams"], vals["fir_taps"], vals["fir_decim"]
    c.ctaps, c.rot, c.pilot_taps, c.pilot_coeffs, c.pilot_min = ptr(cc), ptr(rr), vals["pilot_taps"], ptr(bb), vals["pilot_min"]
    c.max_bytes_per_call, c.device, c.flags = vals["max_bytes_per_call"], vals["device"], vals["flags"]
    return c


def _create(pkg, **kw):
    lib = pkg.load_library()
    keep = []
    c = _cfg(pkg, keep, **kw)
    hnd = C.c_void_p()
    rc = lib.sdrfm_scan_create(C.byref(c), C.byref(hnd))
    if rc == pkg.lib.OK:
        lib.sdrfm_scan_destroy(hnd)
    else:
        assert not hnd.value
    return rc


def _filled(n, v, idx=None, w=None):
    a = np.full(n, v, np.float32)
    if idx is not None:
        a[idx] = w
    return a


PI_F = np.float32(float.fromhex("0x1.921fb6p+1"))
OVER_PI = np.nextafter(PI_F, np.float32(4))
# the tap-sum bounds at their limits: 2T = 128 taps of 1/8 sum to 16 exactly, 2P = 202 taps of 8/202 ... are not exact, so the pilot
# limit is 128 taps of 1/16 (the rest 0): 8 exactly; one tap one ulp up crosses either bound
AT_16 = np.tile(_filled(2 * T, 0.125), (NS, 1))
ABOVE_16 = AT_16.copy()
ABOVE_16[NS - 1, 2 * T - 1] = np.nextafter(np.float32(0.125), np.float32(1))
AT_8 = np.concatenate([_filled(128, 0.0625), np.zeros(2 * P - 128, np.float32)])
ABOVE_8 = AT_8.copy()
ABOVE_8[2 * P - 1] = 1e-6

BAD = {
    "struct_size": dict(struct_size=8), "struct_size_plus": dict(struct_size=200), "streams_zero": dict(n_streams=0),
    "T_zero": dict(fir_taps=0), "T_over": dict(fir_taps=257, ctaps=np.zeros((NS, 2 * 257), np.float32)), "D_zero": dict(fir_decim=0),
    "D_over": dict(fir_decim=65), "P_even": dict(pilot_taps=100), "P_zero": dict(pilot_taps=0),
    "P_over_255": dict(pilot_taps=257, b=np.zeros(2 * 257, np.float32)),
    "null_ctaps": dict(ctaps=None), "null_rot": dict(rot=None), "null_b": dict(b=None),
    "nan_tap_first_stream": dict(ctaps=np.tile(_filled(2 * T, 0.01, 0, np.nan), (NS, 1))),
    "inf_tap_last_stream": dict(ctaps=np.concatenate([np.zeros((NS - 1, 2 * T), np.float32), _filled(2 * T, 0.01, 2 * T - 1, np.inf)[None]])),
    "nan_rot": dict(rot=np.array([0, np.nan, 0], np.float32)), "inf_rot": dict(rot=np.array([0, 0, -np.inf], np.float32)),
    "rot_over_pi": dict(rot=np.array([0, OVER_PI, 0], np.float32)), "rot_under_minus_pi": dict(rot=np.array([0, 0, -OVER_PI], np.float32)),
    "nan_pilot_tap": dict(b=_filled(2 * P, 0.01, 2 * P - 1, np.nan)), "inf_pilot_tap": dict(b=_filled(2 * P, 0.01, 0, np.inf)),
    "channel_tap_sum_above_16": dict(ctaps=ABOVE_16), "pilot_tap_sum_above_8": dict(b=ABOVE_8),
    "max_bytes_above_4MiB": dict(max_bytes_per_call=(4 << 20) + 2), "max_bytes_huge": dict(max_bytes_per_call=0xFFFFFFFE),
    "pilot_min_zero": dict(pilot_min=0.0), "pilot_min_negative": dict(pilot_min=-0.05), "pilot_min_nan": dict(pilot_min=float("nan")),
    "pilot_min_square_underflows": dict(pilot_min=2e-23),
    "flags_unknown": dict(flags=4), "flags_high": dict(flags=0x80000001),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_configs_are_refused_without_a_device(pkg, case):
    assert _create(pkg, **BAD[case]) == pkg.lib.EINVAL


@pytest.mark.parametrize("kw", [dict(), dict(flags=1), dict(flags=2), dict(flags=3), dict(ctaps=AT_16), dict(b=AT_8),
                                dict(max_bytes_per_call=4 << 20), dict(rot=np.array([PI_F, -PI_F, 0], np.float32)), dict(pilot_min=1e20)],
                         ids=["default", "force_generic", "shared_input", "both_flags", "channel_tap_sum_16", "pilot_tap_sum_8", "4MiB", "rot_pi",
                              "pmin2_inf"])
def test_valid_config_looks_for_the_device(pkg, kw):
    rc = _create(pkg, **kw)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    assert rc == (pkg.lib.OK if has_gpu else pkg.lib.NO_DEVICE)


def test_null_handles_are_harmless(pkg):
    lib = pkg.load_library()
    keep = []
    c = _cfg(pkg, keep)
    m = pkg.lib.ScanMeter()
    assert lib.sdrfm_scan_create(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_create(C.byref(c), None) == pkg.lib.EINVAL
    h = C.c_void_p(1)
    assert lib.sdrfm_scan_create(None, C.byref(h)) == pkg.lib.EINVAL and not h.value
    assert lib.sdrfm_scan_reset(None) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_tune(None, keep[0].ctypes.data, keep[1].ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_process_batch(None, None, 0, 100, C.addressof(m), 0) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_process_batch(None, None, 0, 101, C.addressof(m), 0) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_synchronize(None) == pkg.lib.EINVAL
    assert lib.sdrfm_scan_kernel_name(None) == b""
    lib.sdrfm_scan_destroy(None)


def test_python_mirror_raises_the_status(pkg):
    h = pkg.lowpass_taps(T, 120e3 / 2.4e6)
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=pkg.stereo_pilot_taps(P, 240e3)[:100], offsets_hz=[0.0, 1e5], h=h))
    assert e.value.status == pkg.lib.EINVAL


# ---- csrc/scan.c
def _meter(pkg, **kw):
    m = pkg.lib.ScanMeter()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _report(pkg, m, fs=2.4e6, D=10, gain=1.0):
    r = pkg.lib.ScanReport()
    rc = pkg.load_library().sdrfm_scan_report(C.addressof(m) if m is not None else None, fs, D, gain, C.byref(r))
    return rc, r


def test_report_on_hand_made_records(pkg):
    # 4 d's: p = 127.5^2 each (0 dBFS); d = 0.25 rad each (no deviation); pw = 2^-5 each (a steady pilot of 0.177 rad), all above the gate
    n = 4
    m = _meter(pkg, n=n, n_pilot=3, rf_q=int(n * 127.5 ** 2 * 2 ** 8), freq_q=n * (1 << 22), dev_q=n * (1 << 20), pilot_q=n * (1 << 19),
               pilot2_q=n * (1 << 10))
    rc, r = _report(pkg, m, gain=0.5)
    assert rc == pkg.lib.OK
    hz = 2.4e6 / (2 * math.pi * 10)
    assert abs(r.level_dbfs) < 1e-9 and r.freq_err_hz == pytest.approx(0.25 * hz, rel=1e-12) and r.dev_rms_hz == 0.0
    assert r.pilot_rms_rad == pytest.approx(2 ** -2.5, rel=1e-12) and r.pilot_dev_hz == pytest.approx(2 ** -2.5 * hz / 0.5, rel=1e-12)
    assert r.pilot_frac == 0.75 and r.pilot_steadiness == 1.0
    # d = +-0.5 in turn: mean 0, rms 0.5; negative sums are taken as they are
    m = _meter(pkg, n=2, freq_q=0, dev_q=2 * (1 << 22), rf_q=2 * 256, pilot_q=0, pilot2_q=0)
    rc, r = _report(pkg, m)
    assert rc == pkg.lib.OK and r.freq_err_hz == 0.0 and r.dev_rms_hz == pytest.approx(0.5 * hz, rel=1e-12)
    assert r.level_dbfs == pytest.approx(-20 * math.log10(127.5), rel=1e-12) and r.pilot_rms_rad == 0.0 and math.isnan(r.pilot_steadiness)
    m = _meter(pkg, n=1, freq_q=-(1 << 24), dev_q=1 << 24)
    rc, r = _report(pkg, m)
    assert rc == pkg.lib.OK and r.freq_err_hz == pytest.approx(-hz, rel=1e-12) and r.dev_rms_hz == 0.0 and r.level_dbfs == -math.inf


def test_report_of_no_d_is_nan_and_bad_arguments_are_refused(pkg):
    rc, r = _report(pkg, _meter(pkg))
    assert rc == pkg.lib.OK and all(math.isnan(getattr(r, f)) for f, _ in pkg.lib.ScanReport._fields_)
    m = _meter(pkg, n=1)
    assert _report(pkg, None)[0] == pkg.lib.EINVAL
    assert pkg.load_library().sdrfm_scan_report(C.addressof(m), 2.4e6, 10, 1.0, None) == pkg.lib.EINVAL
    for kw in (dict(D=0), dict(fs=0.0), dict(fs=-1.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(gain=0.0), dict(gain=float("nan"))):
        assert _report(pkg, m, **kw)[0] == pkg.lib.EINVAL, kw


def test_meter_add_sums_every_field(pkg):
    lib = pkg.load_library()
    a = _meter(pkg, n=5, n_pilot=2, rf_q=1 << 52, freq_q=-7, dev_q=9, pilot_q=1 << 55, pilot2_q=(1 << 61) + 3)
    b = _meter(pkg, n=1 << 21, n_pilot=1, rf_q=-(1 << 52), freq_q=-(1 << 46), dev_q=1, pilot_q=5, pilot2_q=1 << 61)
    assert lib.sdrfm_scan_meter_add(C.addressof(a), C.addressof(b)) == pkg.lib.OK
    assert (a.n, a.n_pilot, a.rf_q, a.freq_q, a.dev_q, a.pilot_q, a.pilot2_q, a.reserved) == (
        5 + (1 << 21), 3, 0, -7 - (1 << 46), 10, (1 << 55) + 5, (1 << 62) + 3, 0)
    assert lib.sdrfm_scan_meter_add(None, C.addressof(b)) == pkg.lib.EINVAL and lib.sdrfm_scan_meter_add(C.addressof(a), None) == pkg.lib.EINVAL
    acc = np.zeros(2, pkg.METER_DTYPE)
    one = np.zeros(2, pkg.METER_DTYPE)
    one["n"], one["freq_q"] = (3, 4), (-5, 6)
    pkg.meter_add(pkg.meter_add(acc, one), one)
    assert list(acc["n"]) == [6, 8] and list(acc["freq_q"]) == [-10, 12]
