"""The true-peak meter's host side (include/sdrfm.h): the BS.1770-4 Annex 2 table, the host-side C routine that defines the
record, the ordered join, the report in dBTP, and what a report says about a programme — truepeak_alarms against a maximum true peak, and
headroom_gain_q15, the output gain that brings a stream under it (BroadcastDemod.set_audio takes it)."""
import ctypes as C

import numpy as np

from . import lib as _l

TRUEPEAK_DTYPE = _l.TRUEPEAK_DTYPE
TRUEPEAK_REPORT_FIELDS = tuple(n for n, _ in _l.TruePeakReport._fields_)
LIMIT_MAX = 0xFFFFFFFF


def truepeak_default_coef():
    """sdrfm_truepeak_default_coef: int16 [4, 12] in Q15, the 4 x oversampling FIR of ITU-R BS.1770-4 Annex 2"""
    out = np.zeros(48, np.int16)
    P, NT = C.c_uint32(), C.c_uint32()
    st = _l.load_library().sdrfm_truepeak_default_coef(out.ctypes.data, C.byref(P), C.byref(NT))
    if st != _l.OK:
        raise _l.SdrfmError(st, "sdrfm_truepeak_default_coef")
    return out.reshape(P.value, NT.value)


def truepeak_limit(dbtp):
    """sdrfm_truepeak_limit: a level in dBTP in the record's units (0 dBTP = 2^30), floor, clamped to 0 .. 2^32 - 1; NaN gives 0"""
    return int(_l.load_library().sdrfm_truepeak_limit(float(dbtp)))


def _table(coef):
    c = truepeak_default_coef() if coef is None else np.ascontiguousarray(coef, dtype=np.int16)
    if c.ndim != 2 or (coef is not None and not np.array_equal(c, np.asarray(coef))):
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_truepeak_s16: coef")
    return c


def pcm_truepeak_host(pcm, limit=None, coef=None, hist=None, acc=None, limit_dbtp=-1.0):
    """sdrfm_pcm_truepeak_s16 (the host-side C routine, the definition of the record): pcm int16 [2n] or [streams, 2n], L and R interleaved ->
    (records, hist): a TRUEPEAK_DTYPE array, one record per row, joined onto acc (records of the pairs before) when that is given, and the
    rows' histories int16 [streams, 2 (n_taps - 1)] behind the call, continued from hist when that is given (zero otherwise).  limit is in the
    record's units; None takes truepeak_limit(limit_dbtp).  coef: int16 [n_phases, n_taps], the default table when None."""
    lib = _l.load_library()
    c = _table(coef)
    P, NT = c.shape
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    lim = truepeak_limit(limit_dbtp) if limit is None else int(limit)
    if not 0 <= lim <= 0xFFFFFFFFFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_truepeak_s16: limit")
    out = np.zeros(rows.shape[0], dtype=TRUEPEAK_DTYPE) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=TRUEPEAK_DTYPE).copy()
    hw = 2 * max(NT - 1, 1)
    h = np.zeros((rows.shape[0], hw), np.int16) if hist is None else np.ascontiguousarray(np.atleast_2d(hist), dtype=np.int16).copy()
    assert out.shape == (rows.shape[0],) and h.shape == (rows.shape[0], hw), (out.shape, h.shape)
    for k in range(rows.shape[0]):
        st = lib.sdrfm_pcm_truepeak_s16(rows[k].ctypes.data if rows.shape[1] else None, rows.shape[1] // 2, c.ctypes.data, P, NT, lim,
                                        h[k].ctypes.data, out.ctypes.data + 64 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_truepeak_s16")
    return out, h


def truepeak_add(acc, m):
    """acc = acc then m through sdrfm_truepeak_add, record by record (TRUEPEAK_DTYPE arrays of one shape).  The join is ordered: m holds the
    pairs that FOLLOW acc's.  Returns acc."""
    lib = _l.load_library()
    assert acc.dtype == TRUEPEAK_DTYPE and m.dtype == TRUEPEAK_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_truepeak_add(acc.ctypes.data + 64 * k, m.ctypes.data + 64 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_truepeak_add")
    return acc


def truepeak_report(records, n_phases=4, fs_audio=48000.0):
    """records -> dict of float64 arrays, one entry per field of sdrfm_truepeak_report_t, through sdrfm_truepeak_report"""
    lib = _l.load_library()
    records = np.ascontiguousarray(np.atleast_1d(records), dtype=TRUEPEAK_DTYPE)
    out = {n: np.empty(records.size, np.float64) for n in TRUEPEAK_REPORT_FIELDS}
    r = _l.TruePeakReport()
    for k in range(records.size):
        st = lib.sdrfm_truepeak_report(records.ctypes.data + 64 * k, int(n_phases), float(fs_audio), C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_truepeak_report")
        for n in TRUEPEAK_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def truepeak_alarms(report, max_dbtp=-1.0):
    """What a truepeak_report says about the programmes against a maximum true peak (-1 dBTP: EBU R 128), one dict per stream:
      over        the true peak of either channel lies above max_dbtp
      over_l      the left channel's does;  over_r likewise
      overshoot   it lies above 0 dBTP: the reconstructed waveform passes full scale, and an interpolator that saturates clips it
    A NaN (no samples) raises nothing."""
    out = []
    with np.errstate(invalid="ignore"):
        for s in range(len(report["dbtp"])):
            l, r, m = (float(report[k][s]) for k in ("dbtp_l", "dbtp_r", "dbtp"))
            out.append(dict(over=bool(m > max_dbtp), over_l=bool(l > max_dbtp), over_r=bool(r > max_dbtp), overshoot=bool(m > 0.0)))
    return out


def headroom_gain_q15(report, target_dbtp=-1.0):
    """The output gain that brings every stream's true peak to target_dbtp or below: uint16 [n_streams] in Q15 for BroadcastDemod.set_audio
    (gain=...).  A stream at or under the target keeps 32768; one that is x dB over gets floor(32768 10^(-x / 20)) — rounded down, so the
    scaled peak does not come out above the target.  Relative to the gain the report was measured under: multiply it into a gain already
    set.  A NaN (no samples) and -inf (silence) keep 32768."""
    d = np.asarray(report["dbtp"], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        over = np.where(np.isfinite(d), d - float(target_dbtp), 0.0)
        g = np.floor(32768.0 * np.power(10.0, -np.maximum(over, 0.0) / 20.0))
    return np.ascontiguousarray(np.clip(g, 0, 32768), dtype=np.uint16)
