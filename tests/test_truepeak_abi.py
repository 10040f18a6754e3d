"""CPU checks of the true-peak meter's C-ABI (include/sdrfm.h): the nine symbols exported, declared and listed, the record's
layout in the header, in ctypes and in numpy, and every refusal that needs no device.  (Those that need a sink are
tests/test_pcm_truepeak_gpu.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_NAMES = ["sdrfm_truepeak_default_coef", "sdrfm_truepeak_check_coef", "sdrfm_pcm_truepeak_s16", "sdrfm_truepeak_add", "sdrfm_truepeak_report",
             "sdrfm_pcm_stereo_sink_truepeak_enable", "sdrfm_pcm_stereo_sink_truepeak_disable", "sdrfm_pcm_stereo_sink_truepeak_read"]


def _header():
    with open(os.path.join(ROOT, "include", "sdrfm.h")) as fh:
        return fh.read()


def test_symbols_are_exported_declared_and_listed(pkg):
    lib, header = pkg.load_library(), _header()
    for n in INT_NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
        assert re.search(r"^int\s+%s\(" % n, header, re.M), n
    assert hasattr(lib, "sdrfm_truepeak_limit") and "sdrfm_truepeak_limit" in pkg.ABI_SYMBOLS
    assert re.search(r"^uint64_t\s+sdrfm_truepeak_limit\(double", header, re.M)
    assert len(set(pkg.ABI_SYMBOLS)) == len(pkg.ABI_SYMBOLS)
    assert re.search(r"^#define SDRFM_ABI_VERSION\s+1u?\b", header, re.M) and lib.sdrfm_abi_version() == 1
    for m in ("enable_truepeak", "disable_truepeak", "read_truepeak", "read_truepeak_device"):
        assert callable(getattr(pkg.StereoPcmSink, m)), m
    for f in ("truepeak_default_coef", "pcm_truepeak_host", "truepeak_add", "truepeak_report", "truepeak_limit", "truepeak_alarms", "headroom_gain_q15",
              "truepeak_coef", "TRUEPEAK_DTYPE"):
        assert hasattr(pkg, f) and f in pkg.__all__, f
    assert "DESIGN.md §4.23" in header and "BS.1770-4 Annex 2" in header and "KEEPS THE HISTORY" in header


def test_record_layout(pkg):
    L = pkg.lib
    assert C.sizeof(L.TruePeak) == 64 and C.alignment(L.TruePeak) == 8 and L.TRUEPEAK_DTYPE.itemsize == 64
    names = ["n", "peak_l", "peak_r", "at_l", "at_r", "over_l", "over_r", "reserved"]
    assert [n for n, _ in L.TruePeak._fields_] == list(L.TRUEPEAK_DTYPE.names) == names
    for k, name in enumerate(names):
        assert getattr(L.TruePeak, name).offset == L.TRUEPEAK_DTYPE.fields[name][1] == 8 * k, name
    body = re.search(r"typedef struct sdrfm_truepeak \{(.*?)\} sdrfm_truepeak;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert all(d.strip().startswith("uint64_t") for d in body.split(";") if d.strip())
    assert [n.strip() for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")] == names
    assert C.sizeof(L.TruePeakReport) == 8 * 7
    rep = re.search(r"typedef struct sdrfm_truepeak_report_t \{(.*?)\} sdrfm_truepeak_report_t;", _header(), re.S).group(1)
    assert [n.strip() for d in rep.split(";") if d.strip() for n in d.replace("double", "").split(",")] == [n for n, _ in L.TruePeakReport._fields_]


def test_refusals_that_need_no_device(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    rec = np.zeros(2, pkg.TRUEPEAK_DTYPE)
    rec["n"], rec["peak_l"] = 77, 5
    before = rec.tobytes()
    pcm = np.array([1, -1, 2, -2], np.int16)
    coef = pkg.truepeak_default_coef()
    hist = np.arange(22, dtype=np.int16)
    hist0 = hist.copy()
    call = lambda p, n, c, P, NT, lim, h, a: lib.sdrfm_pcm_truepeak_s16(p, n, c, P, NT, lim, h, a)
    ok = (pcm.ctypes.data, 2, coef.ctypes.data, 4, 12, 0, hist.ctypes.data, rec.ctypes.data)
    for k in (0, 2, 6, 7):                                                                  # pcm, coef, hist, acc
        assert call(*[None if j == k else v for j, v in enumerate(ok)]) == E, k
    for P, NT in ((0, 12), (1, 12), (3, 12), (16, 12), (4, 0), (4, 2), (4, 6), (4, 66), (4, 68)):
        assert call(pcm.ctypes.data, 2, coef.ctypes.data, P, NT, 0, hist.ctypes.data, rec.ctypes.data) == E, (P, NT)
    assert call(pcm.ctypes.data, 2, coef.ctypes.data, 4, 12, 1 << 32, hist.ctypes.data, rec.ctypes.data) == E
    assert call(None, 0, coef.ctypes.data, 4, 12, (1 << 32) - 1, hist.ctypes.data, rec.ctypes.data) == 0
    assert rec.tobytes() == before and np.array_equal(hist, hist0)                           # nothing was written
    assert lib.sdrfm_truepeak_add(None, rec.ctypes.data) == E and lib.sdrfm_truepeak_add(rec.ctypes.data, None) == E
    r = pkg.lib.TruePeakReport()
    assert lib.sdrfm_truepeak_report(None, 4, 48000.0, C.byref(r)) == E and lib.sdrfm_truepeak_report(rec.ctypes.data, 4, 48000.0, None) == E
    for P in (0, 1, 3, 16):
        assert lib.sdrfm_truepeak_report(rec.ctypes.data, P, 48000.0, C.byref(r)) == E
    for bad in (0.0, -48000.0, float("nan"), float("inf")):
        assert lib.sdrfm_truepeak_report(rec.ctypes.data, 4, bad, C.byref(r)) == E
    assert lib.sdrfm_truepeak_default_coef(None, None, None) == E and lib.sdrfm_truepeak_check_coef(None, 4, 12) == E
    # a NULL sink: before any device is looked for
    assert lib.sdrfm_pcm_stereo_sink_truepeak_enable(None, None, 0, 0, 0) == E
    assert lib.sdrfm_pcm_stereo_sink_truepeak_enable(None, coef.ctypes.data, 4, 12, 1 << 30) == E
    assert lib.sdrfm_pcm_stereo_sink_truepeak_disable(None) == E
    for flags in (0, 1, 8, 9, 2):
        assert lib.sdrfm_pcm_stereo_sink_truepeak_read(None, rec.ctypes.data, flags) == E
    assert rec.tobytes() == before
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_truepeak_host(pcm, 0, np.zeros((3, 12), np.int16))
    assert e.value.status == E
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_truepeak_host(pcm, -1)
    assert e.value.status == E
