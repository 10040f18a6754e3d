"""IqMeter — the Python mirror of the sdrfm_iq_meter_* C entry points: what the raw capture's bytes say in front of every filter —
ADC level, rail hits, DC and I/Q imbalance — per stream on the device, as sums of small integers; iq_meter_host, the host routine that defines them;
the joins and reports of records and histogram rows; and the policy that turns a report into a tuner gain step (gain_advice, nearest_gain)."""
import ctypes as C
import math

import numpy as np

from . import lib as _l

IQ_METER_DTYPE = _l.IQ_METER_DTYPE
IQ_HIST_BINS = _l.IQ_HIST_BINS
IQ_REPORT_FIELDS = tuple(n for n, _ in _l.IqReport._fields_)
IQ_HIST_REPORT_FIELDS = tuple(n for n, _ in _l.IqHistReport._fields_)
MAX_BYTES = 64 << 20               # SDRFM_IQ_MAX_BYTES
NT, VEC, MAX_ITERS, GRID_TARGET = 256, 16, 4096, 2048   # csrc/sdrfm_iq_meter.h: IQM_NT, IQM_VEC, IQM_MAX_ITERS, IQM_GRID_TARGET
CHUNK = NT * VEC


def iq_meter_geometry(n_streams, nbytes):
    """iqm_grid of csrc/sdrfm_iq_meter.h: (workgroups per stream, vectors of 16 bytes per workgroup) of a call"""
    steps = (int(nbytes) // VEC + NT - 1) // NT
    want = min((GRID_TARGET + int(n_streams) - 1) // int(n_streams), steps)
    want = max(want, (steps + MAX_ITERS - 1) // MAX_ITERS, 1)
    return want, (steps + want - 1) // want * NT


def iq_meter_host(iq, acc=None, hist=None, with_hist=False):
    """sdrfm_iq_meter_u8 (the host-side C routine, the definition of the meter): iq uint8 [2n] or [streams, 2n] -> records IQ_METER_DTYPE [streams],
    and with with_hist (or hist given) also the counts uint64 [streams, 512].  The call's sums are ADDED onto acc and hist where those are given."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(iq), dtype=np.uint8)
    assert rows.ndim == 2, rows.shape
    ns, nbytes = rows.shape
    rec = np.zeros(ns, IQ_METER_DTYPE) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=IQ_METER_DTYPE).copy()
    want_hist = with_hist or hist is not None
    h = None
    if want_hist:
        h = np.zeros((ns, IQ_HIST_BINS), np.uint64) if hist is None else np.ascontiguousarray(np.atleast_2d(hist), dtype=np.uint64).copy()
        assert h.shape == (ns, IQ_HIST_BINS), h.shape
    assert rec.shape == (ns,), rec.shape
    for k in range(ns):
        st = lib.sdrfm_iq_meter_u8(rows[k].ctypes.data if nbytes else None, nbytes, rec.ctypes.data + 64 * k, None if h is None else h[k].ctypes.data)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_iq_meter_u8")
    return (rec, h) if want_hist else rec


def iq_meter_add(acc, m):
    """acc += m through sdrfm_iq_meter_add, record by record (IQ_METER_DTYPE arrays of one shape).  Returns acc."""
    lib = _l.load_library()
    assert acc.dtype == IQ_METER_DTYPE and m.dtype == IQ_METER_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_iq_meter_add(acc.ctypes.data + 64 * k, m.ctypes.data + 64 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_iq_meter_add")
    return acc


def iq_hist_add(acc, rows):
    """acc (uint64 [streams, 512]) += rows (uint32 [streams, 512], a call's) through sdrfm_iq_hist_add.  Returns acc."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.uint32)
    a = acc.reshape(-1, IQ_HIST_BINS)
    assert acc.dtype == np.uint64 and acc.flags.c_contiguous and a.shape == rows.shape, (acc.dtype, acc.shape, rows.shape)
    for k in range(a.shape[0]):
        st = lib.sdrfm_iq_hist_add(a[k].ctypes.data, rows[k].ctypes.data)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_iq_hist_add")
    return acc


def iq_meter_report(records):
    """records -> dict of float64 arrays, one entry per field of sdrfm_iq_report_t"""
    lib = _l.load_library()
    records = np.ascontiguousarray(np.atleast_1d(records), dtype=IQ_METER_DTYPE)
    out = {n: np.empty(records.size, np.float64) for n in IQ_REPORT_FIELDS}
    r = _l.IqReport()
    for k in range(records.size):
        st = lib.sdrfm_iq_meter_report(records.ctypes.data + 64 * k, C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_iq_meter_report")
        for n in IQ_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def iq_hist_report(hist):
    """accumulated rows uint64 [streams, 512] (or [512]) -> dict of arrays, one entry per field of sdrfm_iq_hist_report_t (n is uint64)"""
    lib = _l.load_library()
    h = np.ascontiguousarray(np.atleast_2d(hist), dtype=np.uint64)
    assert h.shape[1] == IQ_HIST_BINS, h.shape
    out = {n: np.empty(h.shape[0], np.uint64 if n == "n" else np.float64) for n in IQ_HIST_REPORT_FIELDS}
    r = _l.IqHistReport()
    for k in range(h.shape[0]):
        st = lib.sdrfm_iq_hist_report(h[k].ctypes.data, C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_iq_hist_report")
        for n in IQ_HIST_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def gain_advice(report, target_dbfs=-12.0, max_rail_share=1e-4, max_step_db=6.0):
    """The step in dB a tuner's gain should take, per stream, from iq_meter_report's dict: the distance from rms_dbfs to target_dbfs clamped to
    +-max_step_db; -max_step_db where either component's rail share is over max_rail_share (a clipped capture reads low, so its level is not
    trusted); 0 where nothing was measured (NaN).  A capture with no variance at all (-inf) gets +max_step_db."""
    lvl = np.atleast_1d(np.asarray(report["rms_dbfs"], dtype=np.float64))
    ri = np.atleast_1d(np.asarray(report["rail_share_i"], dtype=np.float64))
    rq = np.atleast_1d(np.asarray(report["rail_share_q"], dtype=np.float64))
    with np.errstate(invalid="ignore"):
        step = np.clip(float(target_dbfs) - lvl, -float(max_step_db), float(max_step_db))
        step = np.where(np.isnan(lvl), 0.0, step)
        step = np.where((ri > float(max_rail_share)) | (rq > float(max_rail_share)), -float(max_step_db), step)
    return step


def nearest_gain(gains_tenth_db, current, step_db):
    """The entry of the caller's gain list (tenths of a dB, as a tuner reports them) nearest to current + 10 step_db; of two equally near the
    lower.  Returns the value from the list."""
    gains = sorted(int(g) for g in gains_tenth_db)
    if not gains:
        raise ValueError("nearest_gain: an empty gain list")
    want = float(current) + 10.0 * float(step_db)
    if math.isnan(want):
        raise ValueError("nearest_gain: NaN")
    return min(gains, key=lambda g: (abs(g - want), g))


class IqMeter(_l.StreamHandle):
    """The device meter over raw capture rows (sdrfm_iq_meter_*): per stream the record, and where asked for the 2 x 256 counts of the byte values,
    integer for integer iq_meter_host's.  No stream state: every call stands alone, and calls add up through iq_meter_add / iq_hist_add."""
    _destroy = "sdrfm_iq_meter_destroy"
    _prefix = "sdrfm_iq_meter"

    def __init__(self, n_streams, max_bytes_per_call=0, device=0):
        self._lib = _l.load_library()
        self.n_streams, self.max_bytes_per_call = int(n_streams), int(max_bytes_per_call)
        if not all(0 <= v <= 0xFFFFFFFF for v in (self.n_streams, self.max_bytes_per_call)):
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_iq_meter_create")
        cfg = _l.IqMeterConfig(C.sizeof(_l.IqMeterConfig), self.n_streams, self.max_bytes_per_call, device, 0)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_iq_meter_create")

    @property
    def kernel_name(self):
        return self._lib.sdrfm_iq_meter_kernel_name(self._h).decode()

    def process_batch(self, iq, hist=False):
        """host memory: iq uint8 [n_streams, nbytes] (or [nbytes] for one stream) -> records IQ_METER_DTYPE [n_streams], and with hist=True also
        the rows uint32 [n_streams, 512]; synchronous"""
        x = np.ascontiguousarray(iq, dtype=np.uint8)
        if x.ndim == 1:
            x = x[None, :]
        assert x.ndim == 2 and x.shape[0] == self.n_streams, x.shape
        nbytes = x.shape[1]
        rec = np.zeros(self.n_streams, IQ_METER_DTYPE)
        rows = np.zeros((self.n_streams, IQ_HIST_BINS), np.uint32) if hist else None
        self._ck(self._lib.sdrfm_iq_meter_process_batch(self._h, x.ctypes.data if nbytes else None, nbytes, nbytes, rec.ctypes.data,
                                                        None if rows is None else rows.ctypes.data, 0), "sdrfm_iq_meter_process_batch")
        return (rec, rows) if hist else rec

    def process_batch_ptr(self, iq_ptr, iq_stride, nbytes, meters_ptr, hist_ptr=None, flags=_l.F_DEVICE_PTRS):
        """the C call as it stands, on raw addresses: device memory with the default flags, only enqueued on the handle's stream"""
        self._ck(self._lib.sdrfm_iq_meter_process_batch(self._h, C.c_void_p(iq_ptr), int(iq_stride), int(nbytes), C.c_void_p(meters_ptr),
                                                        C.c_void_p(hist_ptr) if hist_ptr else None, int(flags)), "sdrfm_iq_meter_process_batch(ptr)")

    def process_batch_device(self, iq, meters, hist=None, nbytes=None):
        """torch tensors on the device: iq uint8 [n_streams, >= nbytes] (rows contiguous), meters int64 of 8 n_streams elements, hist int32 of
        512 n_streams elements or None for the record alone; only enqueues on the handle's stream"""
        if iq.dim() == 1:
            iq = iq[None, :]
        assert iq.is_cuda and meters.is_cuda and iq.element_size() == 1 and iq.stride(1) == 1 and iq.shape[0] == self.n_streams
        assert meters.is_contiguous() and meters.numel() * meters.element_size() >= 64 * self.n_streams
        assert hist is None or (hist.is_cuda and hist.is_contiguous() and hist.numel() * hist.element_size() >= 4 * IQ_HIST_BINS * self.n_streams)
        nbytes = iq.shape[1] if nbytes is None else int(nbytes)
        self.process_batch_ptr(iq.data_ptr(), iq.stride(0) if self.n_streams > 1 else nbytes, nbytes, meters.data_ptr(),
                               None if hist is None else hist.data_ptr())
