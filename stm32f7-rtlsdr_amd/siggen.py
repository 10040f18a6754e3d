"""Synthetic IQ byte streams (tools/siggen/siggen.c) — inputs only, shared by tests and bench."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"fm": 0, "random": 1, "const": 2, "counter": 3}
_lib = None


def _siggen():
    global _lib
    if _lib is None:
        path = os.path.join(os.path.dirname(_HERE), "tools", "siggen", "libsiggen.so")
        if not os.path.exists(path):
            raise ImportError("%s is missing: run __graft_entry__.build()" % path)
        lib = C.CDLL(path)
        lib.siggen_fill.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_double]
        lib.siggen_fill.restype = None
        lib.siggen_lowpass.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
        lib.siggen_lowpass.restype = None
        _lib = lib
    return _lib


def make_iq(n_streams, n_samples, mode="fm", fs=2.4e6, first_id=0, threads=None, out=None):
    """uint8 array [n_streams, 2*n_samples] of interleaved I/Q; stream s uses PRNG id first_id+s."""
    lib = _siggen()
    m = MODES[mode]
    if out is None:
        out = np.empty((n_streams, 2 * n_samples), dtype=np.uint8)
    assert out.shape == (n_streams, 2 * n_samples) and out.dtype == np.uint8 and out.flags.c_contiguous

    def one(s):
        lib.siggen_fill(out[s].ctypes.data, n_samples, first_id + s, m, float(fs))

    threads = threads or min(32, os.cpu_count() or 1)
    if n_streams == 1 or threads == 1:
        for s in range(n_streams):
            one(s)
    else:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(n_streams)))
    return out


def make_iq_stereo(n_streams, n_samples, left_hz, right_hz, deviation_hz, pilot=True, fs=2.4e6, first_id=0):
    """uint8 [n_streams, 2*n_samples] of a broadcast-FM stereo signal, in numpy: composite
    m = 0.9 [(L+R)/2 + (L-R)/2 sin 2φ] + 0.1 sin φ (φ the 19 kHz pilot's phase; without `pilot` the 0.1 sin φ term is left out and
    L-R is not transmitted: m = 0.9 (L+R)/2), L = sin(2 pi left_hz t), R = sin(2 pi right_hz t); frequency fc + deviation_hz * m with a
    per-stream carrier offset fc uniform in +-20 kHz, integrated by a float64 phase accumulator; I/Q = 127.5 + 100 (cos, sin) + N(0, 4)
    noise, rounded and clipped to u8 (the C generator's amplitude and noise).  left_hz / right_hz: scalars or one per stream.  Stream s
    draws from numpy's generator seeded with first_id + s."""
    lh = np.broadcast_to(np.asarray(left_hz, dtype=np.float64), (n_streams,))
    rh = np.broadcast_to(np.asarray(right_hz, dtype=np.float64), (n_streams,))
    out = np.empty((n_streams, 2 * n_samples), dtype=np.uint8)
    t = np.arange(n_samples, dtype=np.float64) / fs
    ph = 2.0 * np.pi * 19e3 * t
    for s in range(n_streams):
        rng = np.random.default_rng(first_id + s)
        fc = (rng.random() * 2.0 - 1.0) * 20000.0
        phi0 = rng.random() * 2.0 * np.pi
        L, R = np.sin(2.0 * np.pi * lh[s] * t), np.sin(2.0 * np.pi * rh[s] * t)
        if pilot:
            m = 0.9 * ((L + R) / 2 + (L - R) / 2 * np.sin(2.0 * ph)) + 0.1 * np.sin(ph)
        else:
            m = 0.9 * (L + R) / 2
        phase = phi0 + np.cumsum(2.0 * np.pi * (fc + deviation_hz * m) / fs)
        noise = rng.normal(0.0, 2.0, size=(2, n_samples))
        out[s, 0::2] = np.clip(np.rint(127.5 + 100.0 * np.cos(phase) + noise[0]), 0, 255)
        out[s, 1::2] = np.clip(np.rint(127.5 + 100.0 * np.sin(phase) + noise[1]), 0, 255)
    return out
