"""PcmLimiter — the Python mirror of the sdrfm_pcm_limit_* C entry points: the int16 stereo rows the PCM sinks leave, raised by
a ramped make-up gain and held under a sample ceiling by a look-ahead limiter, per stream on the device; pcm_limit_host, the host routine that
defines it; the records' join and report; and normalise_gain_q12, the policy that turns a LoudnessMonitor reading into the make-up gain.
detect="truepeak" and pcm_limit_tp_host are the true-peak form: the detector sees the oversampled waveform."""
import ctypes as C

import numpy as np

from . import lib as _l

LIMIT_DTYPE = _l.LIMIT_DTYPE
LIMIT_PARAMS_DTYPE = _l.LIMIT_PARAMS_DTYPE
LIMIT_REPORT_FIELDS = tuple(n for n, _ in _l.PcmLimitReport._fields_)
TILE = 5120                        # SDRFM_PCM_LIMIT_TILE: pairs of a tile of k_pcm_limit
N_MAX = 1 << 20                    # pairs per call
GAIN_UNITY, GAIN_MAX = 4096, 65536  # Q12
ONE = 32768                        # Q15: no reduction
R_ONE = 1 << 23                    # the release's Q23
CEILING_DEFAULT, RELEASE_DEFAULT = 29204, 874
J_MAX = 65536


def limit_ceiling(dbfs):
    """sdrfm_pcm_limit_ceiling: a level in dBFS as a ceiling in LSB, floor(32768 10^(dbfs / 20)) clamped to 1 .. 32767; NaN gives 1"""
    return int(_l.load_library().sdrfm_pcm_limit_ceiling(float(dbfs)))


def limit_release(seconds, fs=48000):
    """the release delta (Q23 per pair) with which the gain climbs from 0 to 1 in `seconds`: round(2^23 / (seconds fs)) clamped to 1 .. 2^23"""
    pairs = float(seconds) * float(fs)
    if not pairs > 0.0:
        return R_ONE
    return int(min(R_ONE, max(1, round(R_ONE / pairs))))


def normalise_gain_q12(lufs, target=-23.0, max_boost_db=12.0):
    """The make-up gain that brings a programme read at `lufs` (LoudnessMonitor's integrated loudness) to `target` (EBU R 128: -23 LUFS):
    uint32 [n] in Q12 for PcmLimiter.set_gain.  round(4096 10^((target - lufs) / 20)), the boost limited to max_boost_db and the value clamped to
    [0, 65536]; -inf (silence) and NaN (nothing measured yet) give 4096."""
    d = np.atleast_1d(np.asarray(lufs, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        db = np.minimum(float(target) - d, float(max_boost_db))
        g = np.round(4096.0 * np.power(10.0, db / 20.0))
    g = np.where(np.isfinite(d), g, 4096.0)
    return np.ascontiguousarray(np.clip(g, 0, GAIN_MAX), dtype=np.uint32)


def limit_state_init(log2_window, n_streams=1):
    """the state before the start: int32 [n_streams, 4 D]"""
    lib = _l.load_library()
    words = int(lib.sdrfm_pcm_limit_state_words(int(log2_window)))
    if not words:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_state_words")
    st = np.zeros((int(n_streams), words), np.int32)
    for k in range(st.shape[0]):
        lib.sdrfm_pcm_limit_state_init(int(log2_window), st[k].ctypes.data)
    return st


def pcm_limit_host(pcm, log2_window=6, gain_slew=1, J=0, params=None, state=None, acc=None):
    """sdrfm_pcm_limit_s16 (the host-side C routine, the definition of the limiter): pcm int16 [2n] or [streams, 2n], L and R interleaved ->
    (out int16 of the same shape, state int32 [streams, 4 D], records LIMIT_DTYPE [streams]).  params: one (ceiling, release, gain0, gain_t) for
    every row or one per row (LIMIT_PARAMS_DTYPE or tuples), the values after create when None; state continues a stream, None is the state
    before the start; the call's records are joined onto acc (records of the pairs before) when that is given."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    ns, n = rows.shape[0], rows.shape[1] // 2
    if params is None:
        params = (CEILING_DEFAULT, RELEASE_DEFAULT, GAIN_UNITY, GAIN_UNITY)
    par = np.asarray(params)
    if par.dtype != LIMIT_PARAMS_DTYPE:
        v = np.broadcast_to(np.asarray(params, dtype=object), (ns, 4))
        if any(not 0 <= int(x) <= 0xFFFFFFFF for x in v.reshape(-1)):
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_s16: params")
        par = np.array([tuple(int(x) for x in r) for r in v], dtype=LIMIT_PARAMS_DTYPE)
    par = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(par), (ns,)))
    if not all(0 <= int(x) <= 0xFFFFFFFF for x in (log2_window, gain_slew, J)) or n > 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_s16: log2_window, gain_slew, J or n")
    words = int(lib.sdrfm_pcm_limit_state_words(int(log2_window)))
    if not words:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_s16: log2_window")
    st = limit_state_init(log2_window, ns) if state is None else np.ascontiguousarray(np.atleast_2d(state), dtype=np.int32).copy()
    rec = np.zeros(ns, LIMIT_DTYPE) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=LIMIT_DTYPE).copy()
    if acc is None:
        rec["min_gain"] = ONE
    assert st.shape == (ns, words) and rec.shape == (ns,), (st.shape, rec.shape)
    out = np.zeros_like(rows)
    for k in range(ns):
        rc = lib.sdrfm_pcm_limit_s16(rows[k].ctypes.data if n else None, n, int(log2_window), int(gain_slew), int(J), par.ctypes.data + 16 * k,
                                     st[k].ctypes.data, out[k].ctypes.data if n else None, rec.ctypes.data + 32 * k)
        if rc != _l.OK:
            raise _l.SdrfmError(rc, "sdrfm_pcm_limit_s16")
    return (out[0] if np.ndim(pcm) == 1 else out), st, rec


def _tp_table(coef):
    """(coef int16 [P, NT] contiguous or None for the default table, P, NT)"""
    if coef is None:
        return None, 4, 12
    c = np.ascontiguousarray(coef, dtype=np.int16)
    if c.ndim != 2:
        raise _l.SdrfmError(_l.EINVAL, "the true-peak limiter's table: int16 [n_phases, n_taps]")
    return c, c.shape[0], c.shape[1]


def limit_tp_state_init(log2_window, n_taps=12, n_streams=1):
    """the true-peak form's state before the start: int32 [n_streams, 4 D + n_taps]"""
    lib = _l.load_library()
    if not all(0 <= int(v) <= 0xFFFFFFFF for v in (log2_window, n_taps)):
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_state_words")
    words = int(lib.sdrfm_pcm_tplimit_state_words(int(log2_window), int(n_taps)))
    if not words:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_state_words")
    st = np.zeros((int(n_streams), words), np.int32)
    for k in range(st.shape[0]):
        lib.sdrfm_pcm_tplimit_state_init(int(log2_window), int(n_taps), st[k].ctypes.data)
    return st


def pcm_limit_tp_host(pcm, log2_window=6, gain_slew=1, J=0, params=None, state=None, acc=None, coef=None):
    """sdrfm_pcm_tplimit_s16 (the host-side C routine, the definition of the limiter's true-peak form): as pcm_limit_host, with the interpolator's
    table coef int16 [P, NT] (None: the BS.1770 table) -> (out, state int32 [streams, 4 D + NT], records LIMIT_DTYPE [streams]); the output is
    delayed by D + NT / 2 pairs"""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    ns, n = rows.shape[0], rows.shape[1] // 2
    if params is None:
        params = (CEILING_DEFAULT, RELEASE_DEFAULT, GAIN_UNITY, GAIN_UNITY)
    par = np.asarray(params)
    if par.dtype != LIMIT_PARAMS_DTYPE:
        v = np.broadcast_to(np.asarray(params, dtype=object), (ns, 4))
        if any(not 0 <= int(x) <= 0xFFFFFFFF for x in v.reshape(-1)):
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_s16: params")
        par = np.array([tuple(int(x) for x in r) for r in v], dtype=LIMIT_PARAMS_DTYPE)
    par = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(par), (ns,)))
    if not all(0 <= int(x) <= 0xFFFFFFFF for x in (log2_window, gain_slew, J)) or n > 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_s16: log2_window, gain_slew, J or n")
    c, P, NT = _tp_table(coef)
    if c is not None and lib.sdrfm_truepeak_check_coef(c.ctypes.data, P, NT) != _l.OK:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_s16: the table")
    words = int(lib.sdrfm_pcm_tplimit_state_words(int(log2_window), NT))
    if not words:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_tplimit_s16: log2_window against n_taps")
    st = limit_tp_state_init(log2_window, NT, ns) if state is None else np.ascontiguousarray(np.atleast_2d(state), dtype=np.int32).copy()
    rec = limit_identity(ns) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=LIMIT_DTYPE).copy()
    assert st.shape == (ns, words) and rec.shape == (ns,), (st.shape, rec.shape)
    out = np.zeros_like(rows)
    for k in range(ns):
        rc = lib.sdrfm_pcm_tplimit_s16(rows[k].ctypes.data if n else None, n, int(log2_window), int(gain_slew), int(J), par.ctypes.data + 16 * k,
                                       None if c is None else c.ctypes.data, P, NT, st[k].ctypes.data, out[k].ctypes.data if n else None,
                                       rec.ctypes.data + 32 * k)
        if rc != _l.OK:
            raise _l.SdrfmError(rc, "sdrfm_pcm_tplimit_s16")
    return (out[0] if np.ndim(pcm) == 1 else out), st, rec


def limit_identity(n_streams=1):
    """the records of no pairs: the join's identity (0, 0, 32768, 0)"""
    r = np.zeros(int(n_streams), LIMIT_DTYPE)
    r["min_gain"] = ONE
    return r


def limit_add(acc, m):
    """acc = acc then m through sdrfm_pcm_limit_add, record by record (LIMIT_DTYPE arrays of one shape).  The join is ordered: m holds the pairs
    that FOLLOW acc's.  Returns acc."""
    lib = _l.load_library()
    assert acc.dtype == LIMIT_DTYPE and m.dtype == LIMIT_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_pcm_limit_add(acc.ctypes.data + 32 * k, m.ctypes.data + 32 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_limit_add")
    return acc


def limit_report(records, fs_audio=48000.0):
    """records -> dict of float64 arrays, one entry per field of sdrfm_pcm_limit_report_t (reduction_db, limited_frac, at_seconds)"""
    lib = _l.load_library()
    records = np.ascontiguousarray(np.atleast_1d(records), dtype=LIMIT_DTYPE)
    out = {n: np.empty(records.size, np.float64) for n in LIMIT_REPORT_FIELDS}
    r = _l.PcmLimitReport()
    for k in range(records.size):
        st = lib.sdrfm_pcm_limit_report(records.ctypes.data + 32 * k, float(fs_audio), C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_limit_report")
        for n in LIMIT_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


class PcmLimiter(_l.StreamHandle):
    """The device limiter behind the sinks (sdrfm_pcm_limit_*): per stream, the rows under a ramped make-up gain and a look-ahead limiter with a
    window of 2^log2_window pairs, bit for bit pcm_limit_host.  After create: ceiling 29204, release 874, gain 4096.
    detect="truepeak" makes the true-peak form (sdrfm_pcm_tplimit_create), bit for bit pcm_limit_tp_host: the detector sees the waveform the
    table coef (int16 [P, NT], None: the BS.1770 table) interpolates between the samples, and the ceiling reads as dBTP.
    latency: pairs of delay; state_words: int32 words of state per stream; detector: (n_phases, n_taps), (0, 0) for the sample form."""
    _destroy = "sdrfm_pcm_limit_destroy"
    _prefix = "sdrfm_pcm_limit"

    def __init__(self, n_streams, log2_window=6, gain_slew=1, device=0, detect="sample", coef=None):
        if detect not in ("sample", "truepeak") or (detect == "sample" and coef is not None):
            raise ValueError("PcmLimiter: detect is 'sample' or 'truepeak', and only the latter takes a table")
        self._lib = _l.load_library()
        self.n_streams, self.log2_window, self.gain_slew = int(n_streams), int(log2_window), int(gain_slew)
        if not all(0 <= v <= 0xFFFFFFFF for v in (self.n_streams, self.log2_window, self.gain_slew)):
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_create")
        cfg = _l.PcmLimitConfig(self.n_streams, self.log2_window, self.gain_slew, 0, device)
        self._h = C.c_void_p()
        if detect == "truepeak":
            c, P, NT = _tp_table(coef)
            st = self._lib.sdrfm_pcm_tplimit_create(C.byref(cfg), None if c is None else c.ctypes.data, P, NT, C.byref(self._h))
        else:
            st = self._lib.sdrfm_pcm_limit_create(C.byref(cfg), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_pcm_tplimit_create" if detect == "truepeak" else "sdrfm_pcm_limit_create")
        P, NT, lat = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self._lib.sdrfm_pcm_tplimit_get_detector(self._h, C.byref(P), C.byref(NT), C.byref(lat)), "sdrfm_pcm_tplimit_get_detector")
        self.detect, self.detector, self.latency = detect, (int(P.value), int(NT.value)), int(lat.value)
        self.state_words = 4 * ((1 << self.log2_window) - 1) + int(NT.value)

    def _u32(self, v, where):
        x = [int(e) for e in np.broadcast_to(np.asarray(v, dtype=object), (self.n_streams,))]
        if min(x) < 0 or max(x) > 0xFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, where)
        return np.array(x, dtype=np.uint32)

    @property
    def kernel_name(self):
        return self._lib.sdrfm_pcm_limit_kernel_name(self._h).decode()

    def reset(self):
        self._ck(self._lib.sdrfm_pcm_limit_reset(self._h), "sdrfm_pcm_limit_reset")

    def set_params(self, ceiling=None, release=None):
        """one ceiling (LSB, 1 .. 32767) and one release (Q23 per pair, 1 .. 2^23) for every stream or one per stream; None keeps what is set.
        They apply to the pairs that enter from the next call on."""
        c = None if ceiling is None else self._u32(ceiling, "sdrfm_pcm_limit_set_params: ceiling")
        r = None if release is None else self._u32(release, "sdrfm_pcm_limit_set_params: release")
        self._ck(self._lib.sdrfm_pcm_limit_set_params(self._h, None if c is None else c.ctypes.data, None if r is None else r.ctypes.data),
                 "sdrfm_pcm_limit_set_params")

    def set_gain(self, gain_q12, jump=False):
        """the make-up gain's target in Q12 (4096 = unity, at most 65536), one for every stream or one per stream: every ramp restarts where it
        has got to and moves by gain_slew per pair from the next call's first pair on; jump=True sets the gain to the target at once"""
        g = self._u32(gain_q12, "sdrfm_pcm_limit_set_gain")
        self._ck(self._lib.sdrfm_pcm_limit_set_gain(self._h, g.ctypes.data, 1 if jump else 0), "sdrfm_pcm_limit_set_gain")

    def get_params(self):
        """(params LIMIT_PARAMS_DTYPE [n_streams] as the next call uses them, J)"""
        par, J = np.zeros(self.n_streams, LIMIT_PARAMS_DTYPE), C.c_uint32()
        self._ck(self._lib.sdrfm_pcm_limit_get_params(self._h, par.ctypes.data, C.byref(J)), "sdrfm_pcm_limit_get_params")
        return par, int(J.value)

    def state(self):
        """the DEVICE's state int32 [n_streams, state_words]; synchronises the handle's stream"""
        st = np.zeros((self.n_streams, self.state_words), np.int32)
        self._ck(self._lib.sdrfm_pcm_limit_get_state(self._h, st.ctypes.data), "sdrfm_pcm_limit_get_state")
        return st

    def read(self, reset=False):
        """the streams' records LIMIT_DTYPE [n_streams]; reset=True sets them to the identity behind the copy and keeps the state"""
        rec = np.zeros(self.n_streams, LIMIT_DTYPE)
        self._ck(self._lib.sdrfm_pcm_limit_read(self._h, rec.ctypes.data, _l.AMETER_F_RESET if reset else 0), "sdrfm_pcm_limit_read")
        return rec

    def read_device(self, out, reset=False):
        """the same into a device tensor of 4 n_streams int64 (or uint64), enqueued on the handle's stream"""
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 32 * self.n_streams
        self._ck(self._lib.sdrfm_pcm_limit_read(self._h, C.c_void_p(out.data_ptr()), _l.F_DEVICE_PTRS | (_l.AMETER_F_RESET if reset else 0)),
                 "sdrfm_pcm_limit_read(device)")

    def process_batch(self, pcm):
        """host memory: pcm int16 [n_streams, 2n] (L, R interleaved) -> int16 [n_streams, 2n], delayed by `latency` pairs"""
        x = np.ascontiguousarray(pcm, dtype=np.int16)
        if x.ndim == 1:
            x = x[None, :]
        assert x.shape[0] == self.n_streams and x.shape[1] % 2 == 0, x.shape
        n = x.shape[1] // 2
        if n > N_MAX:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_limit_process_batch: n")
        out = np.zeros_like(x)
        self._ck(self._lib.sdrfm_pcm_limit_process_batch(self._h, x.ctypes.data if n else None, 2 * n, n, out.ctypes.data if n else None, 2 * n, 0),
                 "sdrfm_pcm_limit_process_batch")
        return out

    def process_batch_device(self, pcm_in, pcm_out=None, n=None):
        """torch tensors on the device: pcm_in int16 [n_streams, >=2n], pcm_out likewise or None for in place; only enqueues on the handle's
        stream"""
        pcm_out = pcm_in if pcm_out is None else pcm_out
        assert pcm_in.is_cuda and pcm_out.is_cuda and pcm_in.stride(1) == 1 and pcm_out.stride(1) == 1
        n = pcm_in.shape[1] // 2 if n is None else int(n)
        self._ck(self._lib.sdrfm_pcm_limit_process_batch(self._h, C.c_void_p(pcm_in.data_ptr()), pcm_in.stride(0), n, C.c_void_p(pcm_out.data_ptr()),
                                                         pcm_out.stride(0), _l.F_DEVICE_PTRS), "sdrfm_pcm_limit_process_batch(device)")

