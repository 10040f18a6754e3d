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


def rds_waveform(bits, oversample=128):
    """The RDS data signal of `bits` (the standard's coder: differential coding e[n] = b[n] xor e[n-1], then per bit a pair of impulses
    +-(2e - 1) half a bit apart — the biphase symbol —, shaped by H(f) = cos(pi f Tb / 4), |f| <= 2 / Tb = 2375 Hz) on a grid of
    `oversample` points per bit, periodic over the bits given, peak 1.  Returns float64 [len(bits) * oversample]."""
    bits = np.asarray(bits, dtype=np.int64) & 1
    e = np.bitwise_xor.accumulate(bits)
    n = bits.size * oversample
    imp = np.zeros(n)
    imp[0::oversample] = 2.0 * e - 1.0
    imp[oversample // 2::oversample] = -(2.0 * e - 1.0)
    f = np.fft.rfftfreq(n, d=1.0 / oversample)                    # in units of 1 / Tb
    shape = np.where(f <= 2.0, np.cos(np.pi * f / 4.0), 0.0)
    w = np.fft.irfft(np.fft.rfft(imp) * shape, n)
    return w / np.abs(w).max()


def _rds_multiplex(n_samples, groups, rds_deviation_hz, rds_phase, clock_ppm, pilot, left_hz, right_hz, deviation_hz, fs):
    """the multiplex m(t) of make_iq_rds, float64 [n_samples]"""
    from .rds import rds_group_bits
    t = np.arange(n_samples, dtype=np.float64) / fs
    f_pilot = 19e3 * (1.0 + clock_ppm * 1e-6)
    ph = 2.0 * np.pi * f_pilot * t
    L, R = np.sin(2.0 * np.pi * left_hz * t), np.sin(2.0 * np.pi * right_hz * t)
    if pilot:
        n_bits = int(np.ceil(n_samples / fs * f_pilot / 16.0)) + 2
        cyc = [b for g in groups for b in rds_group_bits(g)]
        bits = (cyc * (n_bits // len(cyc) + 1))[:((n_bits + 103) // 104) * 104]
        ov = 128
        w = rds_waveform(bits, ov)
        pos = (f_pilot * t / 16.0) * ov                            # position on the waveform's grid
        i0 = np.floor(pos).astype(np.int64)
        fr = pos - i0
        r = w[i0 % w.size] * (1.0 - fr) + w[(i0 + 1) % w.size] * fr
        m = 0.87 * ((L + R) / 2 + (L - R) / 2 * np.sin(2.0 * ph)) + 0.09 * np.sin(ph) + (rds_deviation_hz / deviation_hz) * r * np.sin(3.0 * ph + rds_phase)
    else:
        m = 0.87 * (L + R) / 2
    return m


def make_iq_rds(n_streams, n_samples, groups, rds_deviation_hz=3e3, rds_phase=0.0, clock_ppm=0.0, pilot=True, left_hz=1e3, right_hz=3.1e3,
                deviation_hz=75e3, fs=2.4e6, first_id=0):
    """uint8 [n_streams, 2*n_samples] of a broadcast-FM station with RDS, in numpy: make_iq_stereo's multiplex with the pilot at 9 % and
    the RDS term added,
    m = 0.87 [(L+R)/2 + (L-R)/2 sin 2φ] + 0.09 sin φ + (rds_deviation_hz / deviation_hz) r(t) sin(3φ + rds_phase),
    r the data signal of `groups` (4-tuples of 16-bit blocks, repeated as long as the samples last; rds_waveform), its bit clock the
    pilot's frequency / 16, bit 0 starting at t = 0.  clock_ppm scales the pilot (and with it the subcarriers and the bit clock) as a
    transmitter-against-dongle crystal offset does.  Without `pilot` the station is mono: m = 0.87 (L+R)/2, no subcarriers at all.
    Carrier offset, start phase and noise per stream as in make_iq_stereo (generator seeded with first_id + s)."""
    m = _rds_multiplex(n_samples, groups, rds_deviation_hz, rds_phase, clock_ppm, pilot, left_hz, right_hz, deviation_hz, fs)
    out = np.empty((n_streams, 2 * n_samples), dtype=np.uint8)
    for s in range(n_streams):
        rng = np.random.default_rng(first_id + s)
        fc = (rng.random() * 2.0 - 1.0) * 20000.0
        phi0 = rng.random() * 2.0 * np.pi
        phase = phi0 + np.cumsum(2.0 * np.pi * (fc + deviation_hz * m) / fs)
        noise = rng.normal(0.0, 2.0, size=(2, n_samples))
        out[s, 0::2] = np.clip(np.rint(127.5 + 100.0 * np.cos(phase) + noise[0]), 0, 255)
        out[s, 1::2] = np.clip(np.rint(127.5 + 100.0 * np.sin(phase) + noise[1]), 0, 255)
    return out


def make_iq_stations(n_samples, stations, fs=2.4e6, seed=0):
    """uint8 [1, 2*n_samples]: one capture that holds several make_iq_rds-style stations.  `stations` is a list of dicts with the keys
    offset_hz (the station's carrier against the capture's centre), amplitude (in byte units; make_iq_rds has 100), left_hz, right_hz,
    groups and, optionally, rds_phase, clock_ppm, rds_deviation_hz, deviation_hz and pilot, which mean what they mean in make_iq_rds.
    Station i is amplitude * exp(j (phi_i + 2 pi cumsum(offset_hz + deviation_hz m_i) / fs)) with a start phase phi_i drawn from the
    generator seeded with `seed`; I/Q = 127.5 + the stations' sum + N(0, 2) noise, rounded and clipped to u8."""
    rng = np.random.default_rng(seed)
    z = np.zeros(n_samples, dtype=np.complex128)
    for st in stations:
        dev = float(st.get("deviation_hz", 75e3))
        m = _rds_multiplex(n_samples, st["groups"], float(st.get("rds_deviation_hz", 3e3)), float(st.get("rds_phase", 0.0)),
                           float(st.get("clock_ppm", 0.0)), bool(st.get("pilot", True)), float(st["left_hz"]), float(st["right_hz"]), dev, fs)
        phase = rng.random() * 2.0 * np.pi + np.cumsum(2.0 * np.pi * (float(st["offset_hz"]) + dev * m) / fs)
        z += float(st["amplitude"]) * np.exp(1j * phase)
    noise = rng.normal(0.0, 2.0, size=(2, n_samples))
    out = np.empty((1, 2 * n_samples), dtype=np.uint8)
    out[0, 0::2] = np.clip(np.rint(127.5 + z.real + noise[0]), 0, 255)
    out[0, 1::2] = np.clip(np.rint(127.5 + z.imag + noise[1]), 0, 255)
    return out


def impair_iq(iq_u8, dc_i=0.0, dc_q=0.0, gain_q=1.0, skew_rad=0.0, drive=1.0):
    """A capture as a zero-IF front end with DC offsets and I/Q imbalance would have handed it over, in numpy: the bytes centred on 127.5,
    I' = drive I + dc_i, Q' = drive gain_q (Q cos(skew_rad) + I sin(skew_rad)) + dc_q, put back on 127.5, rounded and clipped to 0 .. 255.
    For circular content the components then differ by gain_q in amplitude and correlate with sin(skew_rad).  iq_u8: uint8 [..., 2n]; returns
    uint8 of the same shape."""
    x = np.asarray(iq_u8)
    assert x.dtype == np.uint8 and x.shape[-1] % 2 == 0, (x.dtype, x.shape)
    i, q = x[..., 0::2].astype(np.float64) - 127.5, x[..., 1::2].astype(np.float64) - 127.5
    out = np.empty_like(x)
    out[..., 0::2] = np.clip(np.rint(127.5 + float(drive) * i + float(dc_i)), 0, 255)
    out[..., 1::2] = np.clip(np.rint(127.5 + float(drive) * float(gain_q) * (q * np.cos(float(skew_rad)) + i * np.sin(float(skew_rad))) + float(dc_q)), 0, 255)
    return out
