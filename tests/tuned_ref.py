"""Loader of tests/native/tuned_ref.c — the scalar-C definition of a tuned stream's d and, beside it, the frozen real-tap
d in the same style — and the composition of that d with tests/stereo_ref.py and tests/rds_ref.py into the broadcast handle's L, R and bb.
The C file is compiled once per process into a temporary directory (gcc -O2 -ffp-contract=off)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from rds_ref import rds_ref
from stereo_ref import stereo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI_F = np.float32(float.fromhex("0x1.921fb6p+1"))
_lib = None


def _load():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="tuned_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libtuned_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-Wall", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "native", "tuned_ref.c"), "-lm"], check=True, cwd=ROOT, capture_output=True, text=True)
        lib = C.CDLL(so)
        lib.tuned_ref_d_real.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.tuned_ref_d_real.restype = C.c_uint32
        lib.tuned_ref_d.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
        lib.tuned_ref_d.restype = C.c_uint32
        _lib = lib
    return _lib


def real_d(iq, h, D):
    """the frozen definition's d[0 .. M) of one stream's bytes from its start, real taps h"""
    iq = np.ascontiguousarray(iq, np.uint8)
    h = np.ascontiguousarray(h, np.float32)
    d = np.empty(iq.size // 2 // D, np.float32)
    n = _load().tuned_ref_d_real(iq.ctypes.data, iq.size // 2, h.ctypes.data, h.size, D, d.ctypes.data)
    assert n == d.size
    return d


def tuned_d(iq, hz, rot, D):
    """the tuned definition's d[0 .. M): hz = 2T floats, (hr[k], hi[k]) pairs"""
    iq = np.ascontiguousarray(iq, np.uint8)
    hz = np.ascontiguousarray(hz, np.float32).reshape(-1)
    assert hz.size % 2 == 0
    d = np.empty(iq.size // 2 // D, np.float32)
    n = _load().tuned_ref_d(iq.ctypes.data, iq.size // 2, hz.ctypes.data, hz.size // 2, D, float(np.float32(rot)), d.ctypes.data)
    assert n == d.size
    return d


def pairs(hr, hi=None):
    """(hr[k], hi[k]) pairs as 2T floats; hi = None: zeros"""
    hr = np.asarray(hr, np.float32)
    out = np.zeros(2 * hr.size, np.float32)
    out[0::2] = hr
    if hi is not None:
        out[1::2] = np.asarray(hi, np.float32)
    return out


def bcast_ref(d, b, ga, gr, pilot_min, diff_gain, rds_gain, Da, Dr):
    """the broadcast handle's outputs on d: dict(L, R, bb, stereo, rds) with the two references' own dicts"""
    st = stereo_ref(d, b, ga, pilot_min, diff_gain, Da)
    rd = rds_ref(d, b, gr, pilot_min, rds_gain, Dr)
    return dict(L=st["L"], R=st["R"], bb=rd["w"], stereo=st, rds=rd)


def ambiguous(ref_rds):
    """d's whose pilot power lies within 1e-3 relative of the gate (the device's d may fall on either side)"""
    return np.abs(ref_rds["pw"].astype(np.float64) - float(ref_rds["pmin2"])) <= 1e-3 * float(ref_rds["pmin2"])


def clean_outputs(flag, A, taps, decim, lead=0):
    """outputs j whose window of d's [(j + 1) decim - taps - lead, (j + 1) decim - 1] holds no flagged d"""
    c = np.concatenate([[0], np.cumsum(flag.astype(np.int64))])
    nj = (np.arange(A) + 1) * decim - 1
    lo = np.maximum(nj - taps + 1 - lead, 0)
    return (c[nj + 1] - c[lo]) == 0
