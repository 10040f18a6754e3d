"""StereoDemod — Python mirror of the sdrfm_stereo_* C entry points (broadcast FM stereo: pilot-derived L and R)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import lib as _l

CFG_FORCE_GENERIC = 1   # SDRFM_STEREO_CFG_FORCE_GENERIC (include/sdrfm.h)


@dataclass
class StereoConfig:
    fir_coeffs: np.ndarray            # h[0..T): channel low-pass at fs
    audio_coeffs: np.ndarray          # g[0..Ta): audio low-pass at fs/D
    pilot_coeffs: np.ndarray          # b[0..P): complex taps (complex array, or 2P floats re, im), P odd (taps.stereo_pilot_taps)
    pilot_min: float = 0.05           # |q| below this (radians) is "no pilot": c = 0, L = R
    diff_gain: float = 2.0            # 2 = textbook; taps.stereo_diff_gain(D, fs) compensates the discriminator's boxcar
    fir_decim: int = 10
    audio_decim: int = 5
    n_streams: int = 1
    max_bytes_per_call: int = 1 << 20
    device: int = 0
    force_generic: bool = False       # SDRFM_STEREO_CFG_FORCE_GENERIC (tests): never the fast kernel


def _pilot_floats(b):
    b = np.asarray(b)
    if np.iscomplexobj(b):
        out = np.empty(2 * b.size, np.float32)
        out[0::2], out[1::2] = b.real, b.imag
        return out
    return np.ascontiguousarray(b, dtype=np.float32).reshape(-1)


class StereoDemod(_l.StreamHandle):
    _destroy = "sdrfm_stereo_destroy"
    _prefix = "sdrfm_stereo"

    def __init__(self, cfg: StereoConfig):
        self._lib = _l.load_library()
        self.cfg = cfg
        self._hc = np.ascontiguousarray(cfg.fir_coeffs, dtype=np.float32)
        self._gc = np.ascontiguousarray(cfg.audio_coeffs, dtype=np.float32)
        self._bc = _pilot_floats(cfg.pilot_coeffs)
        fp = C.POINTER(C.c_float)
        c = _l.StereoConfig()
        c.struct_size = C.sizeof(_l.StereoConfig)
        c.n_streams = cfg.n_streams
        c.fir_taps, c.fir_decim, c.fir_coeffs = self._hc.size, cfg.fir_decim, self._hc.ctypes.data_as(fp)
        c.pilot_taps, c.pilot_coeffs = self._bc.size // 2, self._bc.ctypes.data_as(fp)
        c.pilot_min, c.diff_gain = float(cfg.pilot_min), float(cfg.diff_gain)
        c.audio_taps, c.audio_decim, c.audio_coeffs = self._gc.size, cfg.audio_decim, self._gc.ctypes.data_as(fp)
        c.max_bytes_per_call, c.device = cfg.max_bytes_per_call, cfg.device
        c.flags = CFG_FORCE_GENERIC if cfg.force_generic else 0
        self._h = C.c_void_p()
        st = self._lib.sdrfm_stereo_create(C.byref(c), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_stereo_create")

    def reset(self):
        self._ck(self._lib.sdrfm_stereo_reset(self._h), "sdrfm_stereo_reset")

    def audio_count(self, nbytes):
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_stereo_audio_count(self._h, int(nbytes), C.byref(n)), "sdrfm_stereo_audio_count")
        return n.value

    @property
    def kernel_name(self):
        return self._lib.sdrfm_stereo_kernel_name(self._h).decode()

    def process_batch(self, iq: np.ndarray):
        """host memory: iq [n_streams, nbytes] uint8 -> (L, R) [n_streams, n_audio] float32 and pilot_count [n_streams] uint32"""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == self.cfg.n_streams
        nbytes = iq.shape[1]
        cap = max(self.audio_count(nbytes & ~1), 1)
        left = np.zeros((iq.shape[0], cap), dtype=np.float32)
        right = np.zeros_like(left)
        pc = np.zeros(iq.shape[0], dtype=np.uint32)
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_stereo_process_batch(self._h, iq.ctypes.data, nbytes, nbytes, left.ctypes.data, right.ctypes.data,
                                                      cap, pc.ctypes.data, C.byref(n), 0), "sdrfm_stereo_process_batch")
        return left[:, : n.value], right[:, : n.value], pc

    def process_batch_device(self, iq, left, right, pilot_count=None, nbytes=None):
        """device tensors: iq uint8 [n_streams, >=nbytes], left / right float32 [n_streams, cap] (same strides), pilot_count int32 / uint32
        [n_streams] or None; enqueue only.  Returns n_audio."""
        assert iq.is_cuda and left.is_cuda and right.is_cuda and left.stride() == right.stride() and left.stride(1) == 1
        nbytes = iq.shape[1] if nbytes is None else int(nbytes)
        pc = C.c_void_p(pilot_count.data_ptr()) if pilot_count is not None else None
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_stereo_process_batch(self._h, C.c_void_p(iq.data_ptr()), iq.stride(0), nbytes, C.c_void_p(left.data_ptr()),
                                                      C.c_void_p(right.data_ptr()), left.stride(0), pc, C.byref(n), _l.F_DEVICE_PTRS),
                 "sdrfm_stereo_process_batch(device)")
        return n.value

    def process_batch_pcm(self, sink, iq: np.ndarray, with_audio=True):
        """sdrfm_stereo_process_batch_pcm on host memory: this call and, behind it, `sink` (a StereoPcmSink) over its L and R rows.
        Returns (L, R, pcm [n_streams, 2 n_audio] int16, pilot_count); with_audio=False passes no audio rows: L and R are None."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == self.cfg.n_streams
        nbytes = iq.shape[1]
        cap = max(self.audio_count(nbytes & ~1), 1)
        left = np.zeros((iq.shape[0], cap), dtype=np.float32) if with_audio else None
        right = np.zeros_like(left) if with_audio else None
        pcm = np.zeros((iq.shape[0], 2 * cap), dtype=np.int16)
        pc = np.zeros(iq.shape[0], dtype=np.uint32)
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_stereo_process_batch_pcm(self._h, sink._h, iq.ctypes.data, nbytes, nbytes, left.ctypes.data if with_audio else None,
                                                          right.ctypes.data if with_audio else None, cap, pcm.ctypes.data, 2 * cap, pc.ctypes.data,
                                                          C.byref(n), 0), "sdrfm_stereo_process_batch_pcm")
        if not with_audio:
            return None, None, pcm[:, : 2 * n.value], pc
        return left[:, : n.value], right[:, : n.value], pcm[:, : 2 * n.value], pc

    def process_batch_pcm_device(self, sink, iq, left, right, pcm, pilot_count=None, nbytes=None):
        """device tensors as process_batch_device takes them, pcm int16 [n_streams, >= 2 n_audio]; left = right = None: the sink reads the
        handle's own rows.  Enqueue only, sink included, on this handle's stream.  Returns n_audio."""
        assert iq.is_cuda and pcm.is_cuda and pcm.stride(1) == 1 and (left is None) == (right is None)
        if left is not None:
            assert left.is_cuda and right.is_cuda and left.stride() == right.stride() and left.stride(1) == 1
        nbytes = iq.shape[1] if nbytes is None else int(nbytes)
        pc = C.c_void_p(pilot_count.data_ptr()) if pilot_count is not None else None
        lp = C.c_void_p(left.data_ptr()) if left is not None else None
        rp = C.c_void_p(right.data_ptr()) if right is not None else None
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_stereo_process_batch_pcm(self._h, sink._h, C.c_void_p(iq.data_ptr()), iq.stride(0), nbytes, lp, rp,
                                                          left.stride(0) if left is not None else 0, C.c_void_p(pcm.data_ptr()), pcm.stride(0), pc,
                                                          C.byref(n), _l.F_DEVICE_PTRS), "sdrfm_stereo_process_batch_pcm(device)")
        return n.value
