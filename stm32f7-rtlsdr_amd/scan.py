"""ScanDemod — Python mirror of the sdrfm_scan_* C entry points (the scan handle): one integer record per candidate
offset of a capture, and on top of it what the records say (meter_report), which candidates are stations (find_stations) and the three
steps in one (scan_capture), whose result feeds BroadcastDemod.tune.  stream_status reads the same records where they come from a running
receiver (BroadcastDemod.process_batch_metered): find_stations' policy, per tuned stream.  The hist call
(process_batch_hist) adds a deviation histogram per stream; hist_report, deviation_quantile and ModulationMonitor read it."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import lib as _l
from .stereo import _pilot_floats
from .taps import pilot_gain, stereo_pilot_taps, tuned_channel_taps, tuned_rotation

CFG_FORCE_GENERIC = 1   # SDRFM_SCAN_CFG_FORCE_GENERIC (include/sdrfm.h)
CFG_SHARED_INPUT = 2    # SDRFM_SCAN_CFG_SHARED_INPUT
MAX_BYTES_PER_CALL = 4 << 20

# sdrfm_scan_meter as a structured dtype: process_batch returns an array of these
METER_DTYPE = np.dtype([("n", "<u8"), ("n_pilot", "<u8"), ("rf_q", "<i8"), ("freq_q", "<i8"), ("dev_q", "<i8"), ("pilot_q", "<i8"),
                        ("pilot2_q", "<i8"), ("reserved", "<u8")])
assert METER_DTYPE.itemsize == C.sizeof(_l.ScanMeter) == 64
REPORT_FIELDS = tuple(n for n, _ in _l.ScanReport._fields_)
HIST_BINS = 512         # SDRFM_SCAN_HIST_BINS: bin b spans (b - 256) / 64 .. (b - 255) / 64 rad of d
HIST_REPORT_FIELDS = tuple(n for n, _ in _l.ScanHistReport._fields_)


@dataclass
class ScanConfig:
    pilot_coeffs: np.ndarray              # b[0..P): complex taps (complex array, or 2P floats re, im), P odd (taps.stereo_pilot_taps)
    offsets_hz: Optional[np.ndarray] = None   # one candidate per stream, with h and fs ...
    h: Optional[np.ndarray] = None        # ... the channel low-pass at fs that taps.tuned_channel_taps moves to every offset
    fs: float = 2.4e6
    ctaps: Optional[np.ndarray] = None    # or the caller's own [n_streams, 2T] ...
    rot: Optional[np.ndarray] = None      # ... and [n_streams]
    pilot_min: float = 0.05
    fir_decim: int = 10
    shared_input: bool = False            # every stream reads row 0 of the input
    max_bytes_per_call: int = 1 << 20     # at most 4 MiB
    device: int = 0
    force_generic: bool = False           # SDRFM_SCAN_CFG_FORCE_GENERIC (tests): never the fast kernel


def _tuning(offsets_hz, h, fs, D):
    off = np.atleast_1d(np.asarray(offsets_hz, dtype=np.float64))
    ctaps = np.stack([tuned_channel_taps(h, f, fs) for f in off])
    rot = np.array([tuned_rotation(f, fs, D) for f in off], dtype=np.float32)
    return ctaps, rot


class ScanDemod(_l.StreamHandle):
    _destroy = "sdrfm_scan_destroy"
    _prefix = "sdrfm_scan"

    def __init__(self, cfg: ScanConfig):
        self._lib = _l.load_library()
        self.cfg = cfg
        if cfg.offsets_hz is not None:
            assert cfg.ctaps is None and cfg.rot is None and cfg.h is not None, "offsets_hz with h, or ctaps with rot"
            self._hc = np.ascontiguousarray(cfg.h, dtype=np.float32)
            ctaps, rot = _tuning(cfg.offsets_hz, self._hc, cfg.fs, cfg.fir_decim)
        else:
            assert cfg.ctaps is not None and cfg.rot is not None, "offsets_hz with h, or ctaps with rot"
            self._hc = None if cfg.h is None else np.ascontiguousarray(cfg.h, dtype=np.float32)
            ctaps, rot = cfg.ctaps, cfg.rot
        rot = np.ascontiguousarray(rot, dtype=np.float32).reshape(-1)
        ctaps = np.ascontiguousarray(ctaps, dtype=np.float32).reshape(rot.size, -1)
        assert ctaps.shape[1] % 2 == 0, ctaps.shape
        self.n_streams, self._T = rot.size, ctaps.shape[1] // 2
        self._bc = _pilot_floats(cfg.pilot_coeffs)
        fp = C.POINTER(C.c_float)
        c = _l.ScanConfig()
        c.struct_size = C.sizeof(_l.ScanConfig)
        c.n_streams, c.fir_taps, c.fir_decim = self.n_streams, self._T, cfg.fir_decim
        c.ctaps, c.rot = ctaps.ctypes.data_as(fp), rot.ctypes.data_as(fp)
        c.pilot_taps, c.pilot_coeffs, c.pilot_min = self._bc.size // 2, self._bc.ctypes.data_as(fp), float(cfg.pilot_min)
        c.max_bytes_per_call, c.device = cfg.max_bytes_per_call, cfg.device
        c.flags = (CFG_FORCE_GENERIC if cfg.force_generic else 0) | (CFG_SHARED_INPUT if cfg.shared_input else 0)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_scan_create(C.byref(c), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_scan_create")

    def reset(self):
        self._ck(self._lib.sdrfm_scan_reset(self._h), "sdrfm_scan_reset")

    def tune(self, offsets_hz=None, fs=None, ctaps=None, rot=None):
        """sdrfm_scan_tune: new candidates — offsets_hz (moved from the handle's h at fs, the configuration's by default) or the caller's
        own ctaps [n_streams, 2T] and rot [n_streams] — and a restart of every stream."""
        if offsets_hz is not None:
            assert ctaps is None and rot is None and self._hc is not None, "offsets_hz needs the h the handle was made with"
            ctaps, rot = _tuning(np.broadcast_to(np.asarray(offsets_hz, np.float64), (self.n_streams,)), self._hc,
                                 self.cfg.fs if fs is None else fs, self.cfg.fir_decim)
        ctaps = np.ascontiguousarray(ctaps, dtype=np.float32)
        rot = np.ascontiguousarray(rot, dtype=np.float32)
        assert ctaps.size == self.n_streams * 2 * self._T and rot.size == self.n_streams, (ctaps.shape, rot.shape)
        self._ck(self._lib.sdrfm_scan_tune(self._h, ctaps.ctypes.data, rot.ctypes.data), "sdrfm_scan_tune")

    @property
    def kernel_name(self):
        return self._lib.sdrfm_scan_kernel_name(self._h).decode()

    def process_batch(self, iq: np.ndarray):
        """host memory: iq [n_streams, nbytes] uint8 (one row with shared_input) -> records, a METER_DTYPE array [n_streams]"""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == (1 if self.cfg.shared_input else self.n_streams), iq.shape
        nbytes = iq.shape[1]
        meters = np.zeros(self.n_streams, dtype=METER_DTYPE)
        self._ck(self._lib.sdrfm_scan_process_batch(self._h, iq.ctypes.data, nbytes, nbytes, meters.ctypes.data, 0), "sdrfm_scan_process_batch")
        return meters

    def process_batch_device(self, iq, meters, nbytes=None):
        """device tensors: iq uint8 [n_streams, >= nbytes] (row 0 alone is read with shared_input), meters int64 [n_streams, 8]
        (sdrfm_scan_meter's eight words); enqueue only"""
        assert iq.is_cuda and meters.is_cuda and meters.is_contiguous() and meters.element_size() * meters.numel() >= 64 * self.n_streams
        nbytes = iq.shape[-1] if nbytes is None else int(nbytes)
        stride = iq.stride(0) if iq.dim() > 1 else nbytes
        self._ck(self._lib.sdrfm_scan_process_batch(self._h, C.c_void_p(iq.data_ptr()), stride, nbytes, C.c_void_p(meters.data_ptr()),
                                                    _l.F_DEVICE_PTRS), "sdrfm_scan_process_batch(device)")

    def process_batch_hist(self, iq: np.ndarray):
        """host memory: iq as process_batch takes it -> (records, a METER_DTYPE array [n_streams]; the deviation histograms of the call's
        new d's, uint32 [n_streams, HIST_BINS]).  The records are process_batch's; the two calls may alternate on a handle."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == (1 if self.cfg.shared_input else self.n_streams), iq.shape
        nbytes = iq.shape[1]
        meters = np.zeros(self.n_streams, dtype=METER_DTYPE)
        hist = np.zeros((self.n_streams, HIST_BINS), dtype=np.uint32)
        self._ck(self._lib.sdrfm_scan_process_batch_hist(self._h, iq.ctypes.data, nbytes, nbytes, meters.ctypes.data, hist.ctypes.data, HIST_BINS, 0),
                 "sdrfm_scan_process_batch_hist")
        return meters, hist

    def process_batch_hist_device(self, iq, meters, hist, nbytes=None):
        """device tensors: iq and meters as process_batch_device takes them, hist 32-bit integers [n_streams, >= HIST_BINS] with unit stride
        along a row (a row's first HIST_BINS words are overwritten, the rest is left alone); enqueue only"""
        assert iq.is_cuda and meters.is_cuda and meters.is_contiguous() and meters.element_size() * meters.numel() >= 64 * self.n_streams
        assert hist.is_cuda and hist.element_size() == 4 and hist.dim() == 2 and hist.shape[0] >= self.n_streams and hist.stride(1) == 1, hist.shape
        nbytes = iq.shape[-1] if nbytes is None else int(nbytes)
        stride = iq.stride(0) if iq.dim() > 1 else nbytes
        hist_stride = hist.stride(0) if self.n_streams > 1 else max(hist.stride(0), hist.shape[1])
        self._ck(self._lib.sdrfm_scan_process_batch_hist(self._h, C.c_void_p(iq.data_ptr()), stride, nbytes, C.c_void_p(meters.data_ptr()),
                                                         C.c_void_p(hist.data_ptr()), hist_stride, _l.F_DEVICE_PTRS), "sdrfm_scan_process_batch_hist(device)")


def meter_add(acc, m):
    """acc += m through sdrfm_scan_meter_add, record by record (METER_DTYPE arrays of one shape); returns acc"""
    lib = _l.load_library()
    assert acc.dtype == METER_DTYPE and m.dtype == METER_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_scan_meter_add(acc.ctypes.data + 64 * k, m.ctypes.data + 64 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_scan_meter_add")
    return acc


def meter_report(meters, fs, D):
    """records -> dict of float64 arrays, one entry per field of sdrfm_scan_report_t, through sdrfm_scan_report with
    pilot_gain = taps.pilot_gain(D, fs)"""
    lib = _l.load_library()
    meters = np.ascontiguousarray(np.atleast_1d(meters), dtype=METER_DTYPE)
    out = {n: np.empty(meters.size, np.float64) for n in REPORT_FIELDS}
    r = _l.ScanReport()
    for k in range(meters.size):
        st = lib.sdrfm_scan_report(meters.ctypes.data + 64 * k, float(fs), int(D), pilot_gain(int(D), float(fs)), C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_scan_report")
        for n in REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def hist_add(acc, hist):
    """acc += hist through sdrfm_scan_hist_add, row by row: acc uint64 [..., HIST_BINS], hist uint32 of the same shape (a hist call's);
    returns acc"""
    lib = _l.load_library()
    assert acc.dtype == np.uint64 and acc.flags.c_contiguous and acc.shape[-1] == HIST_BINS and acc.shape == np.shape(hist), (acc.shape, np.shape(hist))
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    for k in range(acc.size // HIST_BINS):
        st = lib.sdrfm_scan_hist_add(acc.ctypes.data + 8 * HIST_BINS * k, hist.ctypes.data + 4 * HIST_BINS * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_scan_hist_add")
    return acc


def hist_edges_hz(fs, D):
    """the HIST_BINS + 1 bin edges in Hz about the tuned offset: bin b spans edges[b] .. edges[b + 1] (596.8 Hz at 2.4 MS/s and D = 10)"""
    return float(fs) / (2.0 * np.pi * int(D)) * ((np.arange(HIST_BINS + 1, dtype=np.float64) - 256.0) / 64.0)


def _hist_rows(hist):
    hist = np.asarray(hist)
    assert hist.shape[-1] == HIST_BINS and hist.dtype.kind in "ui", (hist.shape, hist.dtype)
    return np.ascontiguousarray(hist.reshape(-1, HIST_BINS), dtype=np.uint64)


def hist_report(hist, meters, fs, D, limit_hz=75e3):
    """histograms [n, HIST_BINS] (a call's uint32 rows, or rows summed with hist_add) and the records of the same calls (a METER_DTYPE array
    [n], or None) -> dict of arrays, one entry per field of sdrfm_scan_hist_report_t, through sdrfm_scan_hist_report"""
    lib = _l.load_library()
    rows = _hist_rows(hist)
    if meters is not None:
        meters = np.ascontiguousarray(np.atleast_1d(meters), dtype=METER_DTYPE)
        assert meters.size == rows.shape[0], (meters.size, rows.shape)
    out = {n: np.empty(rows.shape[0], np.uint64 if n == "n" else np.float64) for n in HIST_REPORT_FIELDS}
    r = _l.ScanHistReport()
    for k in range(rows.shape[0]):
        st = lib.sdrfm_scan_hist_report(rows.ctypes.data + 8 * HIST_BINS * k, None if meters is None else meters.ctypes.data + 64 * k, float(fs), int(D),
                                        float(limit_hz), C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_scan_hist_report")
        for n in HIST_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def deviation_quantile(hist, meters, fs, D, share):
    """The deviation that the share `share` of the d's exceeds (share 0.01: the deviation passed 1 % of the time), bracketed: returns
    (lo_hz, hi_hz), float64 arrays [n] with lo <= the true value <= hi.  A d in bin b lies between the bin's nearest and its farthest point
    from the centre (hist_report's centre_hz); the quantile of the nearest points is lo, that of the farthest is hi — quantiles are monotone
    in the values.  The quantile of values v with counts c is the smallest v with (count of values above v) <= share * n.  NaN for n = 0."""
    assert 0.0 <= float(share) <= 1.0, share
    rows = _hist_rows(hist)
    centre = hist_report(rows, meters, fs, D)["centre_hz"]
    edges = hist_edges_hz(fs, D)
    lo, hi = np.full(rows.shape[0], np.nan), np.full(rows.shape[0], np.nan)

    def quantile(values, counts):
        order = np.argsort(values, kind="stable")
        v, c = values[order], counts[order].astype(np.float64)
        above = c.sum() - np.cumsum(c)                              # the count of values above v[k] (ties in v count as above: conservative)
        return v[int(np.argmax(above <= share * c.sum()))]

    for k in range(rows.shape[0]):
        use = np.flatnonzero(rows[k])
        if use.size == 0:
            continue
        a, b = edges[use] - centre[k], edges[use + 1] - centre[k]
        near = np.where((a <= 0.0) & (b >= 0.0), 0.0, np.minimum(np.abs(a), np.abs(b)))
        far = np.maximum(np.abs(a), np.abs(b))
        lo[k], hi[k] = quantile(near, rows[k][use]), quantile(far, rows[k][use])
    return lo, hi


class ModulationMonitor:
    """Modulation monitoring over the hist calls of a ScanDemod.  push(meters, hist) takes one call's outputs — 50 ms of
    capture a call is ITU-R SM.1268's observation interval —, keeps the running record (meter_add), the running 64-bit histogram (hist_add)
    and the call's peak_hz per stream; summary() reads them."""

    def __init__(self, n_streams, fs, D, limit_hz=75e3):
        self.n_streams, self.fs, self.D, self.limit_hz = int(n_streams), float(fs), int(D), float(limit_hz)
        self.meters = np.zeros(self.n_streams, dtype=METER_DTYPE)
        self.hist = np.zeros((self.n_streams, HIST_BINS), dtype=np.uint64)
        self.peaks = []                                           # one float64 [n_streams] per call

    def push(self, meters, hist):
        meters = np.ascontiguousarray(np.atleast_1d(meters), dtype=METER_DTYPE)
        hist = np.ascontiguousarray(hist, dtype=np.uint32).reshape(self.n_streams, HIST_BINS)
        assert meters.shape == (self.n_streams,), meters.shape
        peak = hist_report(hist, meters, self.fs, self.D, self.limit_hz)["peak_hz"]
        meter_add(self.meters, meters)
        hist_add(self.hist, hist)
        self.peaks.append(peak)
        return peak

    def summary(self):
        """one dict per stream: stream, n, calls (those with any d), peak_hz (the largest of the calls' peaks, each about its own call's
        centre), calls_over (the share of those calls whose peak passed limit_hz), and centre_hz, over_min, over_max and mpx_power_dbr of
        the running histogram and record; NaN where there is no d"""
        rep = hist_report(self.hist, self.meters, self.fs, self.D, self.limit_hz)
        peaks = np.array(self.peaks, np.float64).reshape(len(self.peaks), self.n_streams)
        out = []
        for s in range(self.n_streams):
            p = peaks[:, s][~np.isnan(peaks[:, s])]
            out.append(dict(stream=s, n=int(rep["n"][s]), calls=int(p.size), peak_hz=float(p.max()) if p.size else float("nan"),
                            calls_over=float((p > self.limit_hz).mean()) if p.size else float("nan"), centre_hz=float(rep["centre_hz"][s]),
                            over_min=float(rep["over_min"][s]), over_max=float(rep["over_max"][s]), mpx_power_dbr=float(rep["mpx_power_dbr"][s])))
        return out


# the thresholds of find_stations and stream_status, and the two rules both apply to entry c of a meter_report
MAX_DEV_RMS_HZ, MAX_STEADINESS, PILOT_MIN = 55e3, 1.3, 0.05


def _fm_like(report, c, max_dev_rms_hz):
    """an FM station's rms deviation and not noise's"""
    return bool(report["dev_rms_hz"][c] <= max_dev_rms_hz)


def _stereo(report, c, max_steadiness, pilot_min):
    """a steady pilot, at least pilot_min strong"""
    return bool(report["pilot_steadiness"][c] <= max_steadiness and report["pilot_rms_rad"][c] >= pilot_min)


def find_stations(report, offsets_hz, grid_hz, max_dev_rms_hz=MAX_DEV_RMS_HZ, max_steadiness=MAX_STEADINESS, pilot_min=PILOT_MIN):
    """The candidates of a meter_report that hold a station.  Candidate c is one iff its rms deviation is an FM station's and not noise's
    (dev_rms_hz <= max_dev_rms_hz: 40 - 46 kHz against 65 kHz and more on an empty channel or beside a station) and its carrier lies
    nearer to this candidate than to the next (|freq_err_hz| < grid_hz / 2); it is stereo iff its pilot is steady besides
    (pilot_steadiness <= max_steadiness: 1 for a tone, 2 for noise) and at least pilot_min strong.  Returns a list of dicts:
    offset_hz (the candidate's offset plus its error), level_dbfs, stereo, candidate."""
    off = np.atleast_1d(np.asarray(offsets_hz, np.float64))
    found = []
    for c in range(off.size):
        if not (_fm_like(report, c, max_dev_rms_hz) and abs(report["freq_err_hz"][c]) < grid_hz / 2):
            continue
        stereo = _stereo(report, c, max_steadiness, pilot_min)
        found.append(dict(offset_hz=float(off[c] + report["freq_err_hz"][c]), level_dbfs=float(report["level_dbfs"][c]), stereo=stereo, candidate=c))
    return found


def stream_status(report, offsets_hz, max_dev_rms_hz=MAX_DEV_RMS_HZ, max_steadiness=MAX_STEADINESS, pilot_min=PILOT_MIN, max_err_hz=None):
    """find_stations' policy for the streams of a tuned receiver: report is the meter_report of its records (a metered broadcast call's, or
    several added up), offsets_hz the offsets the streams are tuned to.  One dict per stream, none dropped: present (the deviation rule of
    find_stations and, where max_err_hz is given, |freq_err_hz| < max_err_hz), stereo (find_stations' rule, on a present stream),
    offset_hz (the tuned offset plus the error where present, the tuned offset as it is otherwise), level_dbfs, stream.
    [s["offset_hz"] for s in status] goes straight back into BroadcastDemod.tune(offsets_hz=...)."""
    off = np.atleast_1d(np.asarray(offsets_hz, np.float64))
    status = []
    for c in range(off.size):
        err = float(report["freq_err_hz"][c])
        present = _fm_like(report, c, max_dev_rms_hz) and (max_err_hz is None or abs(err) < max_err_hz)
        status.append(dict(present=present, stereo=present and _stereo(report, c, max_steadiness, pilot_min),
                           offset_hz=float(off[c] + err) if present else float(off[c]), level_dbfs=float(report["level_dbfs"][c]), stream=c))
    return status


def follow_selection(status, tuned_hz, deadband_hz=200.0):
    """Which streams of a tuned receiver a drift correction moves (BroadcastDemod.follow): status is stream_status' list,
    tuned_hz the offsets the streams are tuned to.  A stream moves iff it is present and its offset_hz lies more than deadband_hz from its
    tuned offset; an absent stream never moves.  Returns (the stream indexes that move, the new offsets: offset_hz of those, the tuned
    offset as it is of the others)."""
    tuned = np.atleast_1d(np.asarray(tuned_hz, np.float64))
    assert len(status) == tuned.size, (len(status), tuned.size)
    new, moved = tuned.copy(), []
    for st in status:
        s = int(st["stream"])
        if st["present"] and abs(float(st["offset_hz"]) - tuned[s]) > deadband_hz:
            new[s] = float(st["offset_hz"])
            moved.append(s)
    return moved, new


def pilot_snr_db(report):
    """The pilot's signal-to-noise ratio (dB) in the pilot filter's band, per entry of a meter_report, from pilot_steadiness alone.  The
    steadiness is E|q|^4 / (E|q|^2)^2 of the pilot filter's output q; for a tone in complex Gaussian noise at power ratio rho it is
    s = 1 + (2 rho + 1) / (rho + 1)^2 — 1 for the tone alone, 2 for noise alone — and with u = 1 / (rho + 1) that is s = 1 + 2 u - u^2,
    so u = 1 - sqrt(2 - s) and rho = 1 / u - 1.  s <= 1 gives +inf, s >= 2 (or no steadiness at all) -inf."""
    s = np.atleast_1d(np.asarray(report["pilot_steadiness"], np.float64))
    out = np.full(s.shape, -np.inf)
    out[s <= 1.0] = np.inf
    mid = (s > 1.0) & (s < 2.0)
    u = 1.0 - np.sqrt(2.0 - s[mid])
    out[mid] = 10.0 * np.log10(1.0 / u - 1.0)
    return out


# audio_policy's two corners (dB of pilot_snr_db): full stereo from STEREO_FULL_DB up, mono from STEREO_OFF_DB down.  From the ladder of
# tools/audio_ladder.py (profiles/audio_ladder.txt): at 24 dB the stereo decoder still costs nothing against mono, at 18 dB it has lost
STEREO_FULL_DB, STEREO_OFF_DB = 22.0, 12.0


def audio_policy(report, status, stereo_full_db=STEREO_FULL_DB, stereo_off_db=STEREO_OFF_DB, mute_absent=True):
    """What BroadcastDemod.set_audio should be given for the streams of a tuned receiver: report is the meter_report of its records,
    status stream_status' list of the same streams.  Returns (blend_q15, gain_q15), uint16 [n_streams].  The blend is 0 where the stream is
    not stereo, else rint(32768 clamp((pilot_snr_db - stereo_off_db) / (stereo_full_db - stereo_off_db), 0, 1)); the gain is 0 where the
    stream is not present and mute_absent is set, else 32768.  No hysteresis: the ramps of set_audio are what keeps a change smooth."""
    assert stereo_full_db > stereo_off_db, (stereo_full_db, stereo_off_db)
    snr = pilot_snr_db(report)
    assert len(status) == snr.size, (len(status), snr.size)
    blend, gain = np.zeros(snr.size, np.uint16), np.full(snr.size, 32768, np.uint16)
    for st in status:
        s = int(st["stream"])
        if st["stereo"]:
            blend[s] = int(np.rint(32768.0 * np.clip((snr[s] - stereo_off_db) / (stereo_full_db - stereo_off_db), 0.0, 1.0)))
        if mute_absent and not st["present"]:
            gain[s] = 0
    return blend, gain


# hicut_policy's floor (dB of pilot_snr_db, Q15): from the ladder of tools/hicut_ladder.py (profiles/hicut_ladder.txt) by the rule written there
HICUT_FLOOR_DB, HICUT_FLOOR_Q15 = 10.0, 16384


def hicut_policy(report, status, full_db=STEREO_OFF_DB, floor_db=HICUT_FLOOR_DB, floor_q15=HICUT_FLOOR_Q15):
    """What StereoPcmSink.set_hicut should be given for the streams of a tuned receiver: report is the meter_report of its
    records, status stream_status' list of the same streams.  Returns hicut_q15, uint16 [n_streams].  A stereo stream gets 32768 where
    pilot_snr_db >= full_db, floor_q15 where pilot_snr_db <= floor_db and in between the value linear in dB, rounded to nearest.  full_db
    defaults to STEREO_OFF_DB: the high-cut begins where audio_policy's blend has reached mono.  A stream that is not stereo, or not
    present, gets 32768: the only quality measure here is the pilot's, and a mono station has no pilot to judge it by — a weak mono
    station is not treated, and an absent stream is audio_policy's to mute.  No hysteresis: the ramp of set_hicut is what keeps a change
    smooth."""
    assert full_db > floor_db, (full_db, floor_db)
    assert 1024 <= int(floor_q15) <= 32768, floor_q15
    snr = pilot_snr_db(report)
    assert len(status) == snr.size, (len(status), snr.size)
    hicut = np.full(snr.size, 32768, np.uint16)
    for st in status:
        s = int(st["stream"])
        if st["present"] and st["stereo"]:
            w = float(np.clip((snr[s] - floor_db) / (full_db - floor_db), 0.0, 1.0))
            hicut[s] = int(np.rint(int(floor_q15) + w * (32768 - int(floor_q15))))
    return hicut


def scan_grid(fs, grid_hz=100e3, span_hz=None):
    """the candidate offsets of scan_capture: the multiples of grid_hz within +-span_hz (fs / 2 less one grid step by default)"""
    span = fs / 2 - grid_hz if span_hz is None else float(span_hz)
    k = int(np.floor(span / grid_hz + 1e-9))
    return grid_hz * np.arange(-k, k + 1, dtype=np.float64)


def scan_capture(iq_row, fs, h, grid_hz=100e3, span_hz=None, fir_decim=10, pilot_taps=101, pilot_min=0.05, device=0, details=False):
    """One capture row (uint8, interleaved I/Q at fs) -> the stations in it: a ScanDemod over scan_grid's candidates with the row shared
    by all of them, walked in calls of at most 4 MiB whose records add up exactly, then meter_report and find_stations.  The result's
    offsets go straight into BroadcastDemod.tune(offsets_hz=[s["offset_hz"] for s in found], fs=fs, shared_input=True).
    details=True returns (stations, report, offsets_hz, records) instead."""
    row = np.ascontiguousarray(iq_row, dtype=np.uint8).reshape(-1)
    row = row[:row.size & ~1]
    offsets = scan_grid(fs, grid_hz, span_hz)
    chunk = min(MAX_BYTES_PER_CALL, max(row.size, 2))
    cfg = ScanConfig(pilot_coeffs=stereo_pilot_taps(pilot_taps, fs / fir_decim), offsets_hz=offsets, h=h, fs=fs, pilot_min=pilot_min,
                     fir_decim=fir_decim, shared_input=True, max_bytes_per_call=chunk, device=device)
    total = np.zeros(offsets.size, dtype=METER_DTYPE)
    with ScanDemod(cfg) as sc:
        for pos in range(0, row.size, chunk):
            meter_add(total, sc.process_batch(row[pos:pos + chunk]))
    report = meter_report(total, fs, fir_decim)
    found = find_stations(report, offsets, grid_hz, pilot_min=pilot_min)
    return (found, report, offsets, total) if details else found
