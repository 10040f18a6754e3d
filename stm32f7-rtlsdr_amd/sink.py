"""PcmSink, StereoPcmSink — Python mirrors of the sdrfm_pcm_sink_* and sdrfm_pcm_stereo_sink_* C entry points: de-emphasis + int16 stereo
PCM on the device, in the layout BSP_AUDIO_OUT_Play takes (Utilities/STM32746G-Discovery/stm32746g_discovery_audio.c:224)."""
import ctypes as C

import numpy as np

from . import lib as _l


def pcm_deemph_s16_host(audio, alpha, gain, state=0.0):
    """sdrfm_pcm_deemph_s16 (the host-side C routine) on one stream: returns (pcm int16 [2n], new state)."""
    lib = _l.load_library()
    x = np.ascontiguousarray(audio, dtype=np.float32)
    st = C.c_float(state)
    pcm = np.zeros(2 * x.size, np.int16)
    rc = lib.sdrfm_pcm_deemph_s16(x.ctypes.data, x.size, alpha, gain, C.byref(st), pcm.ctypes.data)
    if rc != _l.OK:
        raise _l.SdrfmError(rc, "sdrfm_pcm_deemph_s16")
    return pcm, st.value


PCM_F_EXACT = 4   # SDRFM_PCM_F_EXACT (include/sdrfm.h)


class PcmSink(_l.StreamHandle):
    """exact=False (default): the blocked-scan kernel (PCM within 1 LSB of the exact form); exact=True: SDRFM_PCM_F_EXACT, one lane per stream,
    bit-identical to the host routine sdrfm_pcm_deemph_s16."""
    _destroy = "sdrfm_pcm_sink_destroy"
    _prefix = "sdrfm_pcm_sink"

    def __init__(self, n_streams, alpha, gain, device=0, exact=False):
        self._lib = _l.load_library()
        self._xf = PCM_F_EXACT if exact else 0
        self.n_streams = int(n_streams)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_pcm_sink_create(self.n_streams, alpha, gain, device, C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_pcm_sink_create")

    def reset(self):
        self._ck(self._lib.sdrfm_pcm_sink_reset(self._h), "sdrfm_pcm_sink_reset")

    def synchronize_status(self):
        """sdrfm_pcm_sink_synchronize's status as it is (0 = fine; SDRFM_FAIL when a run of a demodulator launch waited in vain for its predecessor's state)."""
        return int(self._lib.sdrfm_pcm_sink_synchronize(self._h))

    def state(self):
        out = np.zeros(self.n_streams, np.float32)
        self._ck(self._lib.sdrfm_pcm_sink_get_state(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "sdrfm_pcm_sink_get_state")
        return out

    def process_batch(self, audio: np.ndarray) -> np.ndarray:
        """host memory: audio [n_streams, n] float32 -> pcm [n_streams, 2n] int16 (L = R)"""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        assert a.shape[0] == self.n_streams
        n = a.shape[1]
        pcm = np.zeros((self.n_streams, 2 * n), np.int16)
        self._ck(self._lib.sdrfm_pcm_sink_process_batch(self._h, a.ctypes.data, n, n, pcm.ctypes.data, 2 * n, self._xf),
                 "sdrfm_pcm_sink_process_batch")
        return pcm

    def process_batch_device(self, audio, pcm, n=None):
        """torch tensors on the device: audio float32 [n_streams, >=n], pcm int16 [n_streams, >=2n]; only enqueues."""
        assert audio.is_cuda and pcm.is_cuda and audio.stride(1) == 1 and pcm.stride(1) == 1
        n = audio.shape[1] if n is None else int(n)
        self._ck(self._lib.sdrfm_pcm_sink_process_batch(self._h, C.c_void_p(audio.data_ptr()), audio.stride(0), n,
                                                        C.c_void_p(pcm.data_ptr()), pcm.stride(0), _l.F_DEVICE_PTRS | self._xf),
                 "sdrfm_pcm_sink_process_batch(device)")


def pcm_deemph_stereo_s16_host(left, right, alpha, gain, state=(0.0, 0.0)):
    """sdrfm_pcm_deemph_stereo_s16 (host-side C) on one stream: returns (pcm int16 [2n]: L, R interleaved, new (state_L, state_R))."""
    lib = _l.load_library()
    xl = np.ascontiguousarray(left, dtype=np.float32)
    xr = np.ascontiguousarray(right, dtype=np.float32)
    assert xl.shape == xr.shape and xl.ndim == 1
    st = (C.c_float * 2)(*state)
    pcm = np.zeros(2 * xl.size, np.int16)
    rc = lib.sdrfm_pcm_deemph_stereo_s16(xl.ctypes.data, xr.ctypes.data, xl.size, alpha, gain, st, pcm.ctypes.data)
    if rc != _l.OK:
        raise _l.SdrfmError(rc, "sdrfm_pcm_deemph_stereo_s16")
    return pcm, (st[0], st[1])


HICUT_MIN = 1024   # SDRFM_HICUT_MIN (include/sdrfm.h)


def pcm_deemph_stereo_hicut_s16_host(left, right, alpha, gain, h0, ht, slew, J=0, state=(0.0, 0.0)):
    """sdrfm_pcm_deemph_stereo_hicut_s16 (host-side C, the definition of the high-cut: DESIGN.md §4.17) on one stream whose ramp started at h0,
    goes to ht (Q15 ints in [1024, 32768]) at slew units per sample and has run for J samples: returns (pcm int16 [2n]: L, R interleaved,
    new (state_L, state_R)).  The caller carries J: the next call's is min(J + n, 65536)."""
    lib = _l.load_library()
    xl = np.ascontiguousarray(left, dtype=np.float32)
    xr = np.ascontiguousarray(right, dtype=np.float32)
    assert xl.shape == xr.shape and xl.ndim == 1
    for v in (h0, ht):
        if not 0 <= int(v) <= 65535:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_deemph_stereo_hicut_s16: a value outside [1024, 32768]")
    if not 0 <= int(slew) <= 0xFFFFFFFF or not 0 <= int(J) <= 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_deemph_stereo_hicut_s16: slew or J")
    st = (C.c_float * 2)(*state)
    pcm = np.zeros(2 * xl.size, np.int16)
    rc = lib.sdrfm_pcm_deemph_stereo_hicut_s16(xl.ctypes.data, xr.ctypes.data, xl.size, alpha, gain, int(h0), int(ht), int(slew), int(J), st, pcm.ctypes.data)
    if rc != _l.OK:
        raise _l.SdrfmError(rc, "sdrfm_pcm_deemph_stereo_hicut_s16")
    return pcm, (st[0], st[1])


def hicut_slew(ramp_ms, rate_hz=48000.0):
    """the slew of a ramp time, as BroadcastDemod.set_audio computes its own: a full-scale change takes ramp_ms of audio at most,
    slew = max(1, ceil(32768 / (ramp_ms rate_hz / 1000))); ramp_ms = 0 (or less than one sample) is a jump, 32768"""
    n = float(ramp_ms) * float(rate_hz) / 1000.0
    if not n >= 0.0:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_set_hicut: ramp_ms")
    return 32768 if n <= 1.0 else max(1, int(np.ceil(32768.0 / n)))


class StereoPcmSink(_l.StreamHandle):
    """The device sink for L and R rows (sdrfm_pcm_stereo_sink_*): pcm[2i] = L, pcm[2i + 1] = R, each channel de-emphasised on its own.
    exact=False (default): the blocked scan, per channel the mono PcmSink's default form bit for bit (PCM within 1 LSB of the exact form);
    exact=True: SDRFM_PCM_F_EXACT, one lane per stream, bit-identical to the host routine sdrfm_pcm_deemph_stereo_s16."""
    _destroy = "sdrfm_pcm_stereo_sink_destroy"
    _prefix = "sdrfm_pcm_stereo_sink"

    def __init__(self, n_streams, alpha, gain, device=0, exact=False):
        self._lib = _l.load_library()
        self._xf = PCM_F_EXACT if exact else 0
        self.n_streams = int(n_streams)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_pcm_stereo_sink_create(self.n_streams, alpha, gain, device, C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_pcm_stereo_sink_create")

    def reset(self):
        self._ck(self._lib.sdrfm_pcm_stereo_sink_reset(self._h), "sdrfm_pcm_stereo_sink_reset")

    def state(self):
        """[n_streams, 2] float32: the carried de-emphasis states (L, R) of every stream"""
        out = np.zeros((self.n_streams, 2), np.float32)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_get_state(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "sdrfm_pcm_stereo_sink_get_state")
        return out

    def _hq15(self, v):
        """floats in [1/32, 1] / Q15 ints in [1024, 32768] (one value or one per stream) -> uint16 [n_streams]; what a uint16 cannot hold is
        refused here with the C call's status, any other value outside the range by the C call itself"""
        a = np.array(np.broadcast_to(np.asarray(v), (self.n_streams,)))
        q = np.rint(a * 32768.0) if a.dtype.kind == "f" else a.astype(np.int64)
        if not np.all(np.isfinite(q)) or q.min() < 0 or q.max() > 65535:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_set_hicut: hicut outside [1/32, 1]")
        return np.ascontiguousarray(q, dtype=np.uint16)

    def set_hicut(self, hicut=None, ramp_ms=50.0, rate_hz=48000.0):
        """sdrfm_pcm_stereo_sink_set_hicut: the per-stream high-cut, the factor on the sink's alpha (1 = the plain de-emphasis,
        1/4 = a corner near 480 Hz at 75 us) as floats in [1/32, 1] or Q15 ints in [1024, 32768], one value or one per stream; None keeps the
        targets.  It moves to its target over ramp_ms of audio at rate_hz at most (hicut_slew); ramp_ms = 0 is a jump.  Returns the slew."""
        q = None if hicut is None else self._hq15(hicut)
        slew = hicut_slew(ramp_ms, rate_hz)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_set_hicut(self._h, q.ctypes.data if q is not None else None, slew), "sdrfm_pcm_stereo_sink_set_hicut")
        return slew

    def clear_hicut(self):
        """back to the plain kernels and their bits: hicut = 1"""
        self._ck(self._lib.sdrfm_pcm_stereo_sink_set_hicut(self._h, None, 0), "sdrfm_pcm_stereo_sink_set_hicut")

    def hicut_state(self):
        """sdrfm_pcm_stereo_sink_get_hicut: (hicut uint16 [n_streams]: what the next sample starts from, target uint16 [n_streams], slew: 0 on a
        sink that is not conditioned)"""
        h, t = np.zeros(self.n_streams, np.uint16), np.zeros(self.n_streams, np.uint16)
        slew = C.c_uint32()
        self._ck(self._lib.sdrfm_pcm_stereo_sink_get_hicut(self._h, h.ctypes.data, t.ctypes.data, C.byref(slew)), "sdrfm_pcm_stereo_sink_get_hicut")
        return h, t, int(slew.value)

    def condition(self, report, status, ramp_ms=50.0, **policy):
        """set_hicut(scan.hicut_policy(report, status, **policy), ramp_ms): the high-cut the records ask for.  Returns it."""
        from .scan import hicut_policy
        hicut = hicut_policy(report, status, **policy)
        self.set_hicut(hicut, ramp_ms)
        return hicut

    def process_batch(self, left: np.ndarray, right: np.ndarray) -> np.ndarray:
        """host memory: left, right [n_streams, n] float32 -> pcm [n_streams, 2n] int16 (L, R interleaved)"""
        xl = np.ascontiguousarray(left, dtype=np.float32)
        xr = np.ascontiguousarray(right, dtype=np.float32)
        if xl.ndim == 1:
            xl, xr = xl[None, :], xr[None, :]
        assert xl.shape == xr.shape and xl.shape[0] == self.n_streams
        n = xl.shape[1]
        pcm = np.zeros((self.n_streams, 2 * n), np.int16)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_process_batch(self._h, xl.ctypes.data, xr.ctypes.data, n, n, pcm.ctypes.data, 2 * n, self._xf),
                 "sdrfm_pcm_stereo_sink_process_batch")
        return pcm

    def process_batch_device(self, left, right, pcm, n=None):
        """torch tensors on the device: left, right float32 [n_streams, >=n] (same strides), pcm int16 [n_streams, >=2n]; only enqueues."""
        assert left.is_cuda and right.is_cuda and pcm.is_cuda and left.stride() == right.stride() and left.stride(1) == 1 and pcm.stride(1) == 1
        n = left.shape[1] if n is None else int(n)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_process_batch(self._h, C.c_void_p(left.data_ptr()), C.c_void_p(right.data_ptr()), left.stride(0), n,
                                                               C.c_void_p(pcm.data_ptr()), pcm.stride(0), _l.F_DEVICE_PTRS | self._xf),
                 "sdrfm_pcm_stereo_sink_process_batch(device)")

    # ---- the audio meter ----
    def enable_meter(self, quiet_lsb=0):
        """sdrfm_pcm_stereo_sink_meter_enable: from the next call on every launch of this sink is followed by the meter kernel, which joins the
        call's record onto each stream's; a sample is quiet when |x| <= quiet_lsb (0 .. 32767).  Enabling again zeroes the records."""
        if not 0 <= int(quiet_lsb) <= 0xFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_meter_enable: quiet_lsb")
        self._ck(self._lib.sdrfm_pcm_stereo_sink_meter_enable(self._h, int(quiet_lsb)), "sdrfm_pcm_stereo_sink_meter_enable")

    def disable_meter(self):
        self._ck(self._lib.sdrfm_pcm_stereo_sink_meter_disable(self._h), "sdrfm_pcm_stereo_sink_meter_disable")

    def read_meters(self, reset=True):
        """sdrfm_pcm_stereo_sink_meter_read into host memory: an AUDIO_METER_DTYPE array [n_streams], what the sink has written since the records
        were last zeroed; reset=True zeroes them behind the copy, so that successive reads join with audio_meter_add (AudioMonitor does)."""
        out = np.zeros(self.n_streams, dtype=AUDIO_METER_DTYPE)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_meter_read(self._h, out.ctypes.data, _l.AMETER_F_RESET if reset else 0), "sdrfm_pcm_stereo_sink_meter_read")
        return out

    def read_meters_device(self, out, reset=True):
        """the same into a torch tensor on the device of at least 192 * n_streams bytes (8-byte aligned); only enqueues on the sink's stream"""
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 192 * self.n_streams
        self._ck(self._lib.sdrfm_pcm_stereo_sink_meter_read(self._h, C.c_void_p(out.data_ptr()), _l.F_DEVICE_PTRS | (_l.AMETER_F_RESET if reset else 0)),
                 "sdrfm_pcm_stereo_sink_meter_read(device)")

    # ---- the loudness meter ----
    def enable_loudness(self, block_len=4800, cap_blocks=64, coef=None):
        """sdrfm_pcm_stereo_sink_loudness_enable: from the next call on every launch of this sink is followed by the loudness kernel, which leaves
        the K-weighted energies of every completed sub-block of block_len pairs in a ring of cap_blocks per stream.  coef: 10 doubles
        (loudness_default_coef() when None); a stable set outside the device's domain (sdrfm_loudness_check_domain) is refused with SDRFM_EINVAL
        and pcm_loudness_host serves it.  Enabling again starts over."""
        for v, what in ((block_len, "block_len"), (cap_blocks, "cap_blocks")):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_loudness_enable: " + what)
        c = None
        if coef is not None:
            c = np.ascontiguousarray(coef, dtype=np.float64)
            if c.shape != (10,):
                raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_loudness_enable: coef")
        self._ck(self._lib.sdrfm_pcm_stereo_sink_loudness_enable(self._h, None if c is None else c.ctypes.data, int(block_len), int(cap_blocks)),
                 "sdrfm_pcm_stereo_sink_loudness_enable")
        self._loud_cap = int(cap_blocks)

    def disable_loudness(self):
        self._ck(self._lib.sdrfm_pcm_stereo_sink_loudness_disable(self._h), "sdrfm_pcm_stereo_sink_loudness_disable")

    def read_loudness(self, out_cap_blocks=None):
        """sdrfm_pcm_stereo_sink_loudness_read: (first_block, energies float64 [n_streams, n_blocks, 2]) — the sub-blocks completed and not yet
        read, (e_l, e_r) in LSB^2; first_block is the stream-global index of the first.  Synchronises the sink's stream."""
        cap = getattr(self, "_loud_cap", 0) if out_cap_blocks is None else int(out_cap_blocks)
        buf = np.zeros((self.n_streams, max(cap, 1), 2), np.float64)
        first, nb = C.c_uint64(0), C.c_uint32(0)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_loudness_read(self._h, buf.ctypes.data, cap, C.byref(first), C.byref(nb), 0), "sdrfm_pcm_stereo_sink_loudness_read")
        return int(first.value), buf.reshape(-1)[:self.n_streams * nb.value * 2].reshape(self.n_streams, nb.value, 2).copy()

    def loudness_state(self):
        """sdrfm_pcm_stereo_sink_loudness_get_state: a LOUDNESS_STATE_DTYPE array [n_streams] (pos, z, e) from the device"""
        out = np.zeros(self.n_streams, dtype=_l.LOUDNESS_STATE_DTYPE)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_loudness_get_state(self._h, out.ctypes.data), "sdrfm_pcm_stereo_sink_loudness_get_state")
        return out

    # ---- the true-peak meter ----
    def enable_truepeak(self, limit_dbtp=-1.0, coef=None, limit=None):
        """sdrfm_pcm_stereo_sink_truepeak_enable: from the next call on every launch of this sink is followed by the true-peak kernel, which joins
        the call's record (peak of the 4 x oversampled waveform, where it is, and how many values lie over limit_dbtp) onto each stream's.  coef:
        int16 [n_phases, n_taps] in Q15 (the BS.1770-4 Annex 2 table when None; taps.truepeak_coef designs others).  limit, when given, is the limit in the record's units
        (0 dBTP = 2^30) and limit_dbtp is not looked at.  Enabling again starts over."""
        from .truepeak import truepeak_limit
        c, P, NT = None, 0, 0
        if coef is not None:
            c = np.ascontiguousarray(coef, dtype=np.int16)
            if c.ndim != 2 or not np.array_equal(c, np.asarray(coef)):
                raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_truepeak_enable: coef")
            P, NT = c.shape
        lim = truepeak_limit(limit_dbtp) if limit is None else int(limit)
        if not 0 <= lim <= 0xFFFFFFFFFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_stereo_sink_truepeak_enable: limit")
        self._ck(self._lib.sdrfm_pcm_stereo_sink_truepeak_enable(self._h, None if c is None else c.ctypes.data, P, NT, lim),
                 "sdrfm_pcm_stereo_sink_truepeak_enable")
        self.truepeak_phases = 4 if c is None else int(P)

    def disable_truepeak(self):
        self._ck(self._lib.sdrfm_pcm_stereo_sink_truepeak_disable(self._h), "sdrfm_pcm_stereo_sink_truepeak_disable")

    def read_truepeak(self, reset=True):
        """sdrfm_pcm_stereo_sink_truepeak_read into host memory: a TRUEPEAK_DTYPE array [n_streams], what the sink has written since the records
        were last zeroed; reset=True zeroes them behind the copy and keeps the history, so that successive reads join with truepeak_add."""
        out = np.zeros(self.n_streams, dtype=_l.TRUEPEAK_DTYPE)
        self._ck(self._lib.sdrfm_pcm_stereo_sink_truepeak_read(self._h, out.ctypes.data, _l.AMETER_F_RESET if reset else 0), "sdrfm_pcm_stereo_sink_truepeak_read")
        return out

    def read_truepeak_device(self, out, reset=True):
        """the same into a torch tensor on the device of at least 64 * n_streams bytes (8-byte aligned); only enqueues on the sink's stream"""
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 64 * self.n_streams
        self._ck(self._lib.sdrfm_pcm_stereo_sink_truepeak_read(self._h, C.c_void_p(out.data_ptr()), _l.F_DEVICE_PTRS | (_l.AMETER_F_RESET if reset else 0)),
                 "sdrfm_pcm_stereo_sink_truepeak_read(device)")


AUDIO_METER_DTYPE = _l.AUDIO_METER_DTYPE
AUDIO_REPORT_FIELDS = tuple(n for n, _ in _l.AudioReport._fields_)


def pcm_audio_meter_host(pcm, quiet_lsb=0, acc=None):
    """sdrfm_pcm_audio_meter_s16 (the host-side C routine, the definition of the record): pcm int16 [2n] or [streams, 2n], L and R interleaved
    -> an AUDIO_METER_DTYPE array, one record per row, joined onto acc (records of the pairs before) when that is given."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    if not 0 <= int(quiet_lsb) <= 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_audio_meter_s16: quiet_lsb")
    out = np.zeros(rows.shape[0], dtype=AUDIO_METER_DTYPE) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=AUDIO_METER_DTYPE).copy()
    assert out.shape == (rows.shape[0],), out.shape
    for k in range(rows.shape[0]):
        st = lib.sdrfm_pcm_audio_meter_s16(rows[k].ctypes.data if rows.shape[1] else None, rows.shape[1] // 2, int(quiet_lsb), out.ctypes.data + 192 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_audio_meter_s16")
    return out


def audio_meter_add(acc, m):
    """acc = acc then m through sdrfm_audio_meter_add, record by record (AUDIO_METER_DTYPE arrays of one shape).  The join is ordered: m holds
    the pairs that FOLLOW acc's.  Returns acc."""
    lib = _l.load_library()
    assert acc.dtype == AUDIO_METER_DTYPE and m.dtype == AUDIO_METER_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_audio_meter_add(acc.ctypes.data + 192 * k, m.ctypes.data + 192 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_audio_meter_add")
    return acc


def audio_meter_report(meters, fs_audio=48000.0):
    """records -> dict of float64 arrays, one entry per field of sdrfm_audio_report_t, through sdrfm_audio_meter_report"""
    lib = _l.load_library()
    meters = np.ascontiguousarray(np.atleast_1d(meters), dtype=AUDIO_METER_DTYPE)
    out = {n: np.empty(meters.size, np.float64) for n in AUDIO_REPORT_FIELDS}
    r = _l.AudioReport()
    for k in range(meters.size):
        st = lib.sdrfm_audio_meter_report(meters.ctypes.data + 192 * k, float(fs_audio), C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_audio_meter_report")
        for n in AUDIO_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


# audio_alarms' thresholds: a silence of two seconds; L and R at a correlation of -0.5 or below; a side signal 40 dB below the mid; one sample in
# ten thousand at a rail
SILENCE_S, PHASE_CORR, MONO_SIDE_DB, CLIP_SHARE = 2.0, -0.5, -40.0, 1e-4


def audio_alarms(report, silence_s=SILENCE_S, phase_corr=PHASE_CORR, mono_side_db=MONO_SIDE_DB, clip_share=CLIP_SHARE):
    """What an audio_meter_report says about the programme, one dict per stream:
      silent        both channels have been quiet for the last silence_s seconds or more (trail_both_s: the run is still going on)
      left_dead     L has been quiet that long and R has not;  right_dead likewise
      out_of_phase  the correlation of L and R is phase_corr or below
      mono          the side signal lies mono_side_db or more below the mid signal
      clipping      a share of clip_share or more of either channel's samples sits at a rail
    A NaN (no samples, a channel without power) raises nothing."""
    out = []
    with np.errstate(invalid="ignore"):
        for s in range(len(report["trail_both_s"])):
            tl, tr, tb = (float(report[k][s]) for k in ("trail_l_s", "trail_r_s", "trail_both_s"))
            silent = tb >= silence_s
            out.append(dict(silent=bool(silent), left_dead=bool(tl >= silence_s and not tr >= silence_s), right_dead=bool(tr >= silence_s and not tl >= silence_s),
                            out_of_phase=bool(report["correlation"][s] <= phase_corr), mono=bool(report["side_mid_db"][s] <= mono_side_db),
                            clipping=bool(max(report["rail_l"][s], report["rail_r"][s]) >= clip_share)))
    return out


class AudioMonitor:
    """Audio monitoring over the reads of a metered StereoPcmSink.  push(records) takes one read_meters(reset=True) and joins
    it BEHIND the running records (audio_meter_add), so a silence that spans many reads is one run; summary() reads them."""

    def __init__(self, n_streams, fs_audio=48000.0):
        self.n_streams, self.fs_audio = int(n_streams), float(fs_audio)
        self.meters = np.zeros(self.n_streams, dtype=AUDIO_METER_DTYPE)
        self.reads = 0

    def push(self, records):
        """returns the report of this read alone"""
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=AUDIO_METER_DTYPE)
        assert records.shape == (self.n_streams,), records.shape
        audio_meter_add(self.meters, records)
        self.reads += 1
        return audio_meter_report(records, self.fs_audio)

    def summary(self, **thresholds):
        """one dict per stream: stream, n, reads, every field of the running record's report, and alarms (audio_alarms(report, **thresholds))"""
        rep = audio_meter_report(self.meters, self.fs_audio)
        alarms = audio_alarms(rep, **thresholds)
        return [dict(stream=s, n=int(self.meters["n"][s]), reads=self.reads, alarms=alarms[s], **{k: float(rep[k][s]) for k in AUDIO_REPORT_FIELDS})
                for s in range(self.n_streams)]
