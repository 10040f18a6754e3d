"""The channel-tap sets the design-Q sweeps share (tests/test_q_tables.py on the CPU, tests/test_q_taps_gpu.py on the device): a Hamming low-pass of
100 kHz at the rate's sample rate for every tap count T = 1 .. 64 (the reference's RTLSDR_FIR at T = 16), and four sets whose first K-chunk follows
from the VALUES of the taps, not from T: sdrfm_q_build picks the first chunk in which a tap has a non-zero digit (csrc/qtaps.c: dig != 0)."""
import ctypes as C

import numpy as np

RATES = {10: (5, 2.4e6), 8: (8, 2.048e6), 16: (5, 3.2e6)}          # fir_decim -> (audio_decim, fs): the three instances sdrfm_create offers design Q
Q_HMAX = 127 * 65793                                                # SDRFM_Q_HMAX (csrc/sdrfm_q_host.h): the largest |H| three balanced base-256 digits hold
VALUE_SETS = ["32-tail-zero", "32-tail-tiny", "16-tail-zero", "64-head-zero"]


def plain_taps(pkg, T, D):
    """(h, g) of tap count T at the rate of fir_decim D"""
    Da, fs = RATES[D]
    return pkg.default_config(T, fs=fs, fir_decim=D, audio_taps=32, audio_decim=Da)


def first_chunk_by_count(T, D):
    """the first 128-byte K-chunk of a block's window that holds one of T non-zero taps: window byte 2 (9 D - T) is the oldest sample tap T - 1 meets"""
    return (9 * D - T) // 64


def value_taps(pkg, name):
    """(h, g, D, the first chunk the digits imply) of a value-dependent set"""
    if name == "32-tail-zero":                                      # 32 taps, the last six zero: the digits of 26 taps -> chunk 1 at D = 10
        h, g = plain_taps(pkg, 32, 10)
        h = h.copy(); h[26:] = 0.0
        return h, g, 10, first_chunk_by_count(26, 10)
    if name == "32-tail-tiny":                                      # ... a tenth of half a quantum: every one quantises to zero, the float taps are not zero
        h, g = plain_taps(pkg, 32, 10)
        h = h.copy()
        half_quantum = float(np.abs(h).max()) / (2.0 * Q_HMAX)
        h[26:] = np.float32(0.1 * half_quantum) * np.where(np.arange(6) % 2 == 0, 1.0, -1.0).astype(np.float32)
        assert np.all(h[26:] != 0.0)
        return h, g, 10, first_chunk_by_count(26, 10)
    if name == "16-tail-zero":                                      # 16 taps, the last eight zero: chunk 1 at D = 8 (the only way to k_mix<1,4,8,8,16,4>)
        h, g = plain_taps(pkg, 16, 8)
        h = h.copy(); h[8:] = 0.0
        return h, g, 8, first_chunk_by_count(8, 8)
    if name == "64-head-zero":                                      # zeros at the NEWEST samples' end change nothing: the oldest tap still sits in chunk 0
        h, g = plain_taps(pkg, 64, 10)
        h = h.copy(); h[:8] = 0.0
        return h, g, 10, first_chunk_by_count(64, 10)
    raise KeyError(name)


def q_build(pkg, h, D):
    """sdrfm_q_build through the library: (status, tables [chunk][digit][lane][slot], q, cst, first chunk)"""
    lib = pkg.load_library()
    h = np.ascontiguousarray(h, dtype=np.float32)
    A = np.zeros(((D + 3) // 4, 3, 64, 16), dtype=np.int8)
    q, cst, c0 = C.c_float(), C.c_float(), C.c_uint32()
    rc = lib.sdrfm_q_build(h.ctypes.data, h.size, D, A.ctypes.data, C.byref(q), C.byref(cst), C.byref(c0))
    return rc, A, np.float32(q.value), np.float32(cst.value), c0.value


def create_offers_design_q(pkg, h, g, D):
    """sdrfm_create's conditions on the taps (csrc/sdrfm_fm_plan.h: fm_tap_verdict, fm_plan_offers_q), on the CPU: the tables build, the performance rule sum|h| <= 2 |sum h|, and a guard
    radius that a carrier at an eighth of full scale clears."""
    lib = pkg.load_library()
    h = np.ascontiguousarray(h, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    r, a = C.c_float(), C.c_float()
    h64 = h.astype(np.float64)
    return (h.size <= 64 and h.size <= 9 * D and q_build(pkg, h, D)[0] == 0 and np.abs(h64).sum() <= 2.0 * abs(h64.sum()) and
            lib.sdrfm_q_guard2(h.ctypes.data, h.size, g.ctypes.data, g.size, 0, C.byref(r), C.byref(a)) == 0 and
            float(r.value) <= 0.125 * 127.5 * abs(h64.sum()) and a.value > 3.0)
