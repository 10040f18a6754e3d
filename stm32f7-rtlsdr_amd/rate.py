"""PcmRateMatcher — the Python mirror of the sdrfm_pcm_rate_* C entry points: the int16 stereo rows the PCM sinks leave,
resampled per stream by a 32.32 fixed-point step on the device; pcm_rate_host, the host routine that defines it; step_for and ClockServo, which
turn a pair of rates, a crystal's error or a playback ring's fill level into that step."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import lib as _l

ONE = 1 << 32                      # a step of one input pair per output pair
STEP_MIN, STEP_MAX = 1 << 30, 1 << 34
N_MAX = 1 << 20                    # pairs per call


def _table(coef):
    """int16 [(2^LOGPH + 1), NT] -> (contiguous array, NT, LOGPH); the C calls refuse what is out of range"""
    c = np.ascontiguousarray(coef, dtype=np.int16)
    if c.ndim != 2 or c.shape[0] < 2 or (c.shape[0] - 1) & (c.shape[0] - 2):
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_rate: the table is not [(2^LOGPH + 1), NT]")
    return c, c.shape[1], (c.shape[0] - 1).bit_length() - 1


def step_for(fs_in, fs_out, ppm=0.0):
    """the step, input pairs per output pair in 32.32, that turns fs_in into fs_out: round(2^32 fs_in (1 + ppm / 1e6) / fs_out), computed in
    exact rational arithmetic from the arguments as given.  fs_in is the NOMINAL rate of the rows (48000 behind the sinks) and ppm the error of
    the clock that counts them against the consumer's: a dongle whose crystal runs ppm fast delivers fs_in (1 + ppm / 1e6) pairs per second of
    the consumer's time.  The ppm of a dongle is stream_status's tuning error divided by the station's frequency (offset_hz / f_station * 1e6):
    the sampling clock and the tuner's synthesiser hang on the same crystal."""
    r = Fraction(fs_in) * (1 + Fraction(ppm) / 1000000) / Fraction(fs_out)
    step = int(r * ONE + Fraction(1, 2))
    if not STEP_MIN <= step <= STEP_MAX:
        raise _l.SdrfmError(_l.EINVAL, "step_for: %d lies outside [2^30, 2^34]" % step)
    return step


def pcm_rate_host(pcm, coef, step, pos=0, hist=None):
    """sdrfm_pcm_rate_s16 (the host-side C routine, the definition of the matcher) on one stream: pcm int16 [2n], L and R interleaved ->
    (out int16 [2 cnt], new pos, new hist int16 [2 (NT - 1)]).  pos and hist carry the stream from call to call; None is the state after reset."""
    lib = _l.load_library()
    c, nt, logph = _table(coef)
    x = np.ascontiguousarray(pcm, dtype=np.int16)
    assert x.ndim == 1 and x.size % 2 == 0, x.shape
    n = x.size // 2
    if not 0 <= int(step) < 1 << 64 or not 0 <= int(pos) < 1 << 64 or n > 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_rate_s16: step, pos or n")
    h = np.zeros(2 * (nt - 1), np.int16) if hist is None else np.array(hist, dtype=np.int16).reshape(-1)
    assert h.size == 2 * (nt - 1), h.shape
    cap = 0 if int(step) < STEP_MIN else (n * ONE) // int(step) + 1
    out = np.zeros(2 * cap, np.int16)
    p, cnt = C.c_uint64(int(pos)), C.c_uint32()
    st = lib.sdrfm_pcm_rate_s16(x.ctypes.data if n else None, n, c.ctypes.data, nt, logph, int(step), C.byref(p), h.ctypes.data,
                                out.ctypes.data if cap else None, cap, C.byref(cnt))
    if st != _l.OK:
        raise _l.SdrfmError(st, "sdrfm_pcm_rate_s16")
    return out[:2 * cnt.value].copy(), int(p.value), h


class PcmRateMatcher(_l.StreamHandle):
    """The device rate matcher behind the sinks (sdrfm_pcm_rate_*): per stream, out = the rows resampled by step / 2^32 input pairs per output
    pair through coef (taps.rate_coef), bit for bit pcm_rate_host.  Every step starts at 2^32."""
    _destroy = "sdrfm_pcm_rate_destroy"
    _prefix = "sdrfm_pcm_rate"

    def __init__(self, n_streams, coef, device=0):
        self._lib = _l.load_library()
        c, nt, logph = _table(coef)
        self.n_streams, self.n_taps, self.log2_phases = int(n_streams), nt, logph
        cfg = _l.PcmRateConfig(self.n_streams, nt, logph, 0, c.ctypes.data_as(C.POINTER(C.c_int16)), device)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_pcm_rate_create(C.byref(cfg), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_pcm_rate_create")

    @property
    def kernel_name(self):
        return self._lib.sdrfm_pcm_rate_kernel_name(self._h).decode()

    def reset(self):
        self._ck(self._lib.sdrfm_pcm_rate_reset(self._h), "sdrfm_pcm_rate_reset")

    def set_step(self, step):
        """one step (32.32, in [2^30, 2^34]) for every stream or one per stream; it takes effect at the next call's first output"""
        v = [int(x) for x in np.broadcast_to(np.asarray(step, dtype=object), (self.n_streams,))]
        if min(v) < 0 or max(v) >= 1 << 64:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_rate_set_step: a step outside [2^30, 2^34]")
        a = np.array(v, dtype=np.uint64)
        self._ck(self._lib.sdrfm_pcm_rate_set_step(self._h, a.ctypes.data), "sdrfm_pcm_rate_set_step")

    def state(self):
        """(steps uint64 [n_streams], the DEVICE's pos uint64 [n_streams]); synchronises the handle's stream"""
        step, pos = np.zeros(self.n_streams, np.uint64), np.zeros(self.n_streams, np.uint64)
        self._ck(self._lib.sdrfm_pcm_rate_get_state(self._h, step.ctypes.data, pos.ctypes.data), "sdrfm_pcm_rate_get_state")
        return step, pos

    @property
    def steps(self):
        return self.state()[0]

    def count(self, n):
        """what the next call of n pairs yields: (n_out uint32 [n_streams], their maximum)"""
        if not 0 <= int(n) <= 0xFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_rate_count: n")
        out, mx = np.zeros(self.n_streams, np.uint32), C.c_uint32()
        self._ck(self._lib.sdrfm_pcm_rate_count(self._h, int(n), out.ctypes.data, C.byref(mx)), "sdrfm_pcm_rate_count")
        return out, int(mx.value)

    def process_batch(self, pcm):
        """host memory: pcm int16 [n_streams, 2n] (L, R interleaved) -> a list of int16 arrays [2 cnt[s]], one per stream"""
        x = np.ascontiguousarray(pcm, dtype=np.int16)
        if x.ndim == 1:
            x = x[None, :]
        assert x.shape[0] == self.n_streams and x.shape[1] % 2 == 0, x.shape
        n = x.shape[1] // 2
        if n > N_MAX:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_rate_process_batch: n")
        mx = self.count(n)[1]
        out, cnt = np.zeros((self.n_streams, 2 * max(mx, 1)), np.int16), np.zeros(self.n_streams, np.uint32)   # (a row even when nothing comes out)
        self._ck(self._lib.sdrfm_pcm_rate_process_batch(self._h, x.ctypes.data if n else None, 2 * n, n, out.ctypes.data, out.shape[1],
                                                        cnt.ctypes.data, 0), "sdrfm_pcm_rate_process_batch")
        return [out[s, :2 * int(cnt[s])].copy() for s in range(self.n_streams)]

    def process_batch_device(self, pcm_in, pcm_out, n=None):
        """torch tensors on the device: pcm_in int16 [n_streams, >=2n], pcm_out int16 [n_streams, >=2 max cnt]; only enqueues on the handle's
        stream.  Returns n_out uint32 [n_streams], known at return from the host mirror."""
        assert pcm_in.is_cuda and pcm_out.is_cuda and pcm_in.stride(1) == 1 and pcm_out.stride(1) == 1
        n = pcm_in.shape[1] // 2 if n is None else int(n)
        cnt = np.zeros(self.n_streams, np.uint32)
        self._ck(self._lib.sdrfm_pcm_rate_process_batch(self._h, C.c_void_p(pcm_in.data_ptr()), pcm_in.stride(0), n, C.c_void_p(pcm_out.data_ptr()),
                                                        pcm_out.stride(0), cnt.ctypes.data, _l.F_DEVICE_PTRS), "sdrfm_pcm_rate_process_batch(device)")
        return cnt


class ClockServo:
    """A PI loop from a playback ring's fill level to the matcher's step.  The ring is filled by the matcher's output and emptied by the
    consumer's clock; update(fill_pairs) is called once per producer call with the pairs the ring holds and returns the step for the next call:

        e = (fill - target_pairs) / ring_pairs;   I += ki e;   step = nominal (1 + kp e + I)

    A ring that runs full means the consumer is slow, so the step grows and fewer pairs come out.  The defaults suit calls of about a fifth of
    the ring (0.1 s into 0.5 s): with g = call / ring the loop's poles lie at the double root of s^2 + g kp s + g ki, 2 / (g kp) = 333 calls, a
    200 ppm step of the consumer's clock moves the fill by about 0.5 % of the ring, and the integrator ends at the clock's error.  The
    correction is limited to +-limit_ppm."""

    def __init__(self, target_pairs, ring_pairs, nominal_step=ONE, kp=0.03, ki=4.5e-5, limit_ppm=1000.0):
        if not 0 <= target_pairs <= ring_pairs or ring_pairs <= 0 or not STEP_MIN <= int(nominal_step) <= STEP_MAX:
            raise ValueError("ClockServo: target_pairs, ring_pairs or nominal_step")
        self.target, self.ring, self.nominal = float(target_pairs), float(ring_pairs), int(nominal_step)
        self.kp, self.ki, self.limit = float(kp), float(ki), float(limit_ppm) * 1e-6
        self.integ = 0.0
        self.step = self.nominal

    def reset(self):
        self.integ, self.step = 0.0, self.nominal

    @property
    def ppm(self):
        """the correction in force, in ppm of the nominal step"""
        return (self.step / self.nominal - 1.0) * 1e6

    def update(self, fill_pairs):
        e = (float(fill_pairs) - self.target) / self.ring
        self.integ = min(self.limit, max(-self.limit, self.integ + self.ki * e))
        u = min(self.limit, max(-self.limit, self.kp * e + self.integ))
        self.step = min(STEP_MAX, max(STEP_MIN, int(round(self.nominal * (1.0 + u)))))
        return self.step
