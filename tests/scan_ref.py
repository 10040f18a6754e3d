"""Loader of tests/native/scan_ref.c — the scalar-C definition of a scan stream's record from the bytes of a stream's
start — compiled once per process into a temporary directory (gcc -O2 -ffp-contract=off), and the scan scenarios both test files use."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("n", "n_pilot", "rf_q", "freq_q", "dev_q", "pilot_q", "pilot2_q", "reserved")
_lib = None


def _load():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="scan_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libscan_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-Wall", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "native", "scan_ref.c"), "-lm"], check=True, cwd=ROOT, capture_output=True, text=True)
        lib = C.CDLL(so)
        lib.scan_ref.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32, C.c_float,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.scan_ref.restype = C.c_uint32
        _lib = lib
    return _lib


def pilot_floats(b):
    """complex taps (or 2P floats) -> 2P float32 (re, im)"""
    b = np.asarray(b)
    if np.iscomplexobj(b):
        out = np.empty(2 * b.size, np.float32)
        out[0::2], out[1::2] = b.real, b.imag
        return out
    return np.ascontiguousarray(b, np.float32)


def scan_ref(iq, hz, rot, D, b, pilot_min, m0=0, m1=None):
    """dict(rec: the record of the d's [m0, m1) as a dict of ints, d, p, pw: the stream's float32 arrays [M], pmin2)"""
    iq = np.ascontiguousarray(iq, np.uint8)
    hz = np.ascontiguousarray(hz, np.float32).reshape(-1)
    bf = pilot_floats(b)
    M = iq.size // 2 // D
    d, p, pw = (np.empty(M, np.float32) for _ in range(3))
    rec = np.zeros(8, np.int64)
    pmin2 = np.float32(pilot_min) * np.float32(pilot_min)
    n = _load().scan_ref(iq.ctypes.data, iq.size // 2, hz.ctypes.data, hz.size // 2, D, float(np.float32(rot)), bf.ctypes.data, bf.size // 2,
                         float(pmin2), m0, M if m1 is None else m1, d.ctypes.data, p.ctypes.data, pw.ctypes.data, rec.ctypes.data)
    assert n == M
    return dict(rec={f: int(v) for f, v in zip(FIELDS, rec)}, d=d, p=p, pw=pw, pmin2=pmin2)


def rec_of(meter):
    """one record of a METER_DTYPE array (or a dict) as a dict of ints"""
    return {f: int(meter[f]) for f in FIELDS}


def ambiguous(pw, pmin2):
    """d's whose pilot power lies within 1e-3 relative of the gate (the device's d may fall on either side)"""
    return np.abs(pw.astype(np.float64) - float(pmin2)) <= 1e-3 * float(pmin2)
