"""BroadcastDemod — Python mirror of the sdrfm_bcast_* C entry points (the broadcast receiver): the stereo handle's L
and R and the RDS handle's complex baseband of the same streams from one kernel launch, bit for bit what StereoDemod and RdsDemod give.
The metered calls add the scan handle's record of every stream from that launch: scan.meter_add, scan.meter_report and
scan.stream_status read it.  set_audio / clear_audio / audio_state / condition give every stream a stereo blend and an output
gain, ramped per audio output inside the launch; scan.audio_policy makes them from the records.  The hist calls add the
scan handle's deviation histogram of every stream from that launch as well: scan.hist_add, scan.hist_report, scan.deviation_quantile and
scan.ModulationMonitor read it."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import lib as _l
from .scan import HIST_BINS, METER_DTYPE
from .stereo import _pilot_floats

CFG_FORCE_GENERIC = 1   # SDRFM_BCAST_CFG_FORCE_GENERIC (include/sdrfm.h)


@dataclass
class BroadcastConfig:
    fir_coeffs: np.ndarray            # h[0..T): channel low-pass at fs
    audio_coeffs: np.ndarray          # g[0..Ta): audio low-pass at fs/D (StereoConfig.audio_coeffs)
    rds_coeffs: np.ndarray            # g[0..Tr): low-pass at fs/D behind the 57 kHz mixer (RdsConfig.rds_coeffs)
    pilot_coeffs: np.ndarray          # b[0..P): complex taps (complex array, or 2P floats re, im), P odd (taps.stereo_pilot_taps)
    pilot_min: float = 0.05           # |q| below this (radians) is "no pilot": L = R, bb = 0
    diff_gain: float = 2.0            # taps.stereo_diff_gain(D, fs) compensates the discriminator's boxcar at 38 kHz
    rds_gain: float = 2.0             # taps.rds_gain(D, fs) does at 57 kHz
    fir_decim: int = 10
    audio_decim: int = 5
    rds_decim: int = 25
    n_streams: int = 1
    max_bytes_per_call: int = 1 << 20
    device: int = 0
    force_generic: bool = False       # SDRFM_BCAST_CFG_FORCE_GENERIC (tests): never the fast kernel


class BroadcastDemod(_l.StreamHandle):
    _destroy = "sdrfm_bcast_destroy"
    _prefix = "sdrfm_bcast"

    def __init__(self, cfg: BroadcastConfig):
        self._lib = _l.load_library()
        self.cfg = cfg
        self._hc = np.ascontiguousarray(cfg.fir_coeffs, dtype=np.float32)
        self._gac = np.ascontiguousarray(cfg.audio_coeffs, dtype=np.float32)
        self._grc = np.ascontiguousarray(cfg.rds_coeffs, dtype=np.float32)
        self._bc = _pilot_floats(cfg.pilot_coeffs)
        fp = C.POINTER(C.c_float)
        c = _l.BcastConfig()
        c.struct_size = C.sizeof(_l.BcastConfig)
        c.n_streams = cfg.n_streams
        c.fir_taps, c.fir_decim, c.fir_coeffs = self._hc.size, cfg.fir_decim, self._hc.ctypes.data_as(fp)
        c.pilot_taps, c.pilot_coeffs = self._bc.size // 2, self._bc.ctypes.data_as(fp)
        c.pilot_min, c.diff_gain, c.rds_gain = float(cfg.pilot_min), float(cfg.diff_gain), float(cfg.rds_gain)
        c.audio_taps, c.audio_decim, c.audio_coeffs = self._gac.size, cfg.audio_decim, self._gac.ctypes.data_as(fp)
        c.rds_taps, c.rds_decim, c.rds_coeffs = self._grc.size, cfg.rds_decim, self._grc.ctypes.data_as(fp)
        c.max_bytes_per_call, c.device = cfg.max_bytes_per_call, cfg.device
        c.flags = CFG_FORCE_GENERIC if cfg.force_generic else 0
        self._shared_input = False
        self._untuned()
        self._h = C.c_void_p()
        st = self._lib.sdrfm_bcast_create(C.byref(c), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_bcast_create")

    def reset(self):
        self._ck(self._lib.sdrfm_bcast_reset(self._h), "sdrfm_bcast_reset")

    def _untuned(self):
        """what the handle remembers of its tuning: the offsets of its last tune / retune (0 on an untuned handle, None after raw ctaps), the
        fs they were given at, and the taps and rotations themselves (None on an untuned handle: (h, 0) and 0)"""
        self._offsets_hz, self._fs, self._ctaps, self._rot = np.zeros(self.cfg.n_streams, np.float64), 2.4e6, None, None

    def _tuning(self, offsets_hz, fs, ctaps, rot):
        """(offsets [n_streams] or None, ctaps [n_streams, 2T], rot [n_streams]) of tune's and retune's arguments"""
        from .taps import tuned_channel_taps, tuned_rotation
        ns, off = self.cfg.n_streams, None
        if offsets_hz is not None:
            assert ctaps is None and rot is None, "offsets_hz or ctaps / rot, not both"
            off = np.array(np.broadcast_to(np.asarray(offsets_hz, dtype=np.float64), (ns,)))
            ctaps = np.stack([tuned_channel_taps(self._hc, f, fs) for f in off])
            rot = np.array([tuned_rotation(f, fs, self.cfg.fir_decim) for f in off], dtype=np.float32)
        if ctaps is not None:
            ctaps = np.ascontiguousarray(ctaps, dtype=np.float32)
            assert ctaps.size == ns * 2 * self._hc.size, (ctaps.shape, ns, self._hc.size)
        if rot is not None:
            rot = np.ascontiguousarray(rot, dtype=np.float32)
            assert rot.size == ns, (rot.shape, ns)
        return off, ctaps, rot

    def tune(self, offsets_hz=None, fs=2.4e6, shared_input=False, ctaps=None, rot=None):
        """sdrfm_bcast_tune: stream s receives the station at offsets_hz[s] of its input (taps.tuned_channel_taps of
        the handle's fir_coeffs and taps.tuned_rotation at fs), or the caller's own ctaps [n_streams, 2T] and rot [n_streams];
        shared_input: every stream reads row 0 of the input.  No argument at all returns the handle to the untuned kernels.  The carried
        state is zeroed either way."""
        off, ctaps, rot = self._tuning(offsets_hz, fs, ctaps, rot)
        self._ck(self._lib.sdrfm_bcast_tune(self._h, ctaps.ctypes.data if ctaps is not None else None, rot.ctypes.data if rot is not None else None,
                                            _l.TUNE_SHARED_INPUT if shared_input else 0), "sdrfm_bcast_tune")
        self._shared_input = bool(shared_input) and ctaps is not None
        if ctaps is None:
            self._untuned()
        else:
            self._offsets_hz, self._fs, self._ctaps, self._rot = off, float(fs), ctaps.reshape(self.cfg.n_streams, -1).copy(), rot.reshape(-1).copy()

    def retune(self, offsets_hz=None, fs=2.4e6, restart=None, shared_input=None, ctaps=None, rot=None, carry=None):
        """sdrfm_bcast_retune: new taps and rotations between two calls, the streams kept running — offsets_hz at fs as
        tune takes them, or the caller's own ctaps and rot.  restart: [n_streams] of 0 / 1, the streams whose state is zeroed (None: none).
        carry: [n_streams, 2] (cr, ci); None with offsets_hz on a handle that remembers its offsets: taps.retune_carry of the old and the
        new offset per stream; None otherwise: (1, 0).  shared_input=None keeps the current setting.  An untuned handle becomes a tuned one."""
        from .taps import retune_carry
        ns = self.cfg.n_streams
        off, ctaps, rot = self._tuning(offsets_hz, fs, ctaps, rot)
        if carry is None and off is not None and self._offsets_hz is not None:
            carry = np.stack([retune_carry(o, n, self._hc.size, fs) for o, n in zip(self._offsets_hz, off)])
        if carry is not None:
            carry = np.ascontiguousarray(carry, dtype=np.float32)
            assert carry.size == 2 * ns, (carry.shape, ns)
        if restart is not None:
            restart = np.ascontiguousarray(np.broadcast_to(np.asarray(restart), (ns,)), dtype=np.uint8)
        shared = self._shared_input if shared_input is None else bool(shared_input)
        self._ck(self._lib.sdrfm_bcast_retune(self._h, ctaps.ctypes.data if ctaps is not None else None, rot.ctypes.data if rot is not None else None,
                                              carry.ctypes.data if carry is not None else None, restart.ctypes.data if restart is not None else None,
                                              _l.TUNE_SHARED_INPUT if shared else 0), "sdrfm_bcast_retune")
        self._shared_input = shared
        self._offsets_hz, self._fs, self._ctaps, self._rot = off, float(fs), ctaps.reshape(ns, -1).copy(), rot.reshape(-1).copy()

    def follow(self, status, deadband_hz=200.0):
        """One drift correction of a running receiver: status is scan.stream_status' list of this handle's streams.  The
        streams scan.follow_selection picks — present, and more than deadband_hz from their tuned offset — are re-tuned to their offset_hz with
        their state kept; the others keep their taps bit for bit and get carry (1, 0).  Returns the list of stream indexes it moved."""
        from .scan import follow_selection
        from .taps import retune_carry, tuned_channel_taps, tuned_rotation
        assert self._offsets_hz is not None, "the handle was last tuned with raw ctaps: it does not know its offsets"
        ns, fs = self.cfg.n_streams, self._fs
        moved, new = follow_selection(status, self._offsets_hz, deadband_hz)
        if not moved:
            return moved
        if self._ctaps is None:                                      # an untuned handle: (h, 0) and rot 0
            ctaps, rot = np.stack([tuned_channel_taps(self._hc, 0.0, fs)] * ns), np.zeros(ns, np.float32)
        else:
            ctaps, rot = self._ctaps.copy(), self._rot.copy()
        carry = np.tile(np.array([1.0, 0.0], np.float32), (ns, 1))
        for s in moved:
            ctaps[s], rot[s] = tuned_channel_taps(self._hc, new[s], fs), tuned_rotation(new[s], fs, self.cfg.fir_decim)
            carry[s] = retune_carry(self._offsets_hz[s], new[s], self._hc.size, fs)
        self.retune(fs=fs, ctaps=ctaps, rot=rot, carry=carry)
        self._offsets_hz = new
        return moved

    def _q15(self, v, what):
        """None, or floats in [0, 1] / Q15 ints in [0, 32768] (one value or one per stream) -> uint16 [n_streams]; what a uint16 cannot
        hold is refused here with the C call's status, a value above 32768 that it can hold by the C call itself"""
        if v is None:
            return None
        a = np.array(np.broadcast_to(np.asarray(v), (self.cfg.n_streams,)))
        q = np.rint(a * 32768.0) if a.dtype.kind == "f" else a.astype(np.int64)
        if not np.all(np.isfinite(q)) or q.min() < 0 or q.max() > 65535:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_bcast_set_audio: %s outside [0, 1]" % what)
        return np.ascontiguousarray(q, dtype=np.uint16)

    def set_audio(self, blend=None, gain=None, ramp_ms=50.0):
        """sdrfm_bcast_set_audio: per-stream stereo blend (1 = full stereo, 0 = mono) and output gain (0 = muted), floats
        in [0, 1] or Q15 ints in [0, 32768], one value or one per stream; None keeps that kind's targets.  Both move to their targets
        over ramp_ms of audio at most (a full-scale change takes that long): slew = max(1, ceil(32768 / (ramp_ms audio rate / 1000))) with
        the audio rate 2.4 MS/s / (fir_decim audio_decim), or the rate of the last tune; ramp_ms = 0 is a jump."""
        b, g = self._q15(blend, "blend"), self._q15(gain, "gain")
        rate = self._fs / (self.cfg.fir_decim * self.cfg.audio_decim)
        n = float(ramp_ms) * rate / 1000.0
        if not n >= 0.0:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_bcast_set_audio: ramp_ms")
        slew = 32768 if n <= 1.0 else max(1, int(np.ceil(32768.0 / n)))
        self._ck(self._lib.sdrfm_bcast_set_audio(self._h, b.ctypes.data if b is not None else None, g.ctypes.data if g is not None else None, slew),
                 "sdrfm_bcast_set_audio")
        return slew

    def clear_audio(self):
        """back to the plain kernels, their name and their bits: blend = gain = 1"""
        self._ck(self._lib.sdrfm_bcast_set_audio(self._h, None, None, 0), "sdrfm_bcast_set_audio")

    def audio_state(self):
        """sdrfm_bcast_get_audio: dict of uint16 [n_streams] arrays — blend, gain (what the next output starts from), blend_target, gain_target"""
        out = {k: np.zeros(self.cfg.n_streams, np.uint16) for k in ("blend", "gain", "blend_target", "gain_target")}
        self._ck(self._lib.sdrfm_bcast_get_audio(self._h, *(out[k].ctypes.data for k in ("blend", "gain", "blend_target", "gain_target"))),
                 "sdrfm_bcast_get_audio")
        return out

    def condition(self, report, status, ramp_ms=50.0, **policy):
        """set_audio(*scan.audio_policy(report, status, **policy), ramp_ms): the blend and gain the records ask for.  Returns (blend, gain)."""
        from .scan import audio_policy
        blend, gain = audio_policy(report, status, **policy)
        self.set_audio(blend, gain, ramp_ms)
        return blend, gain

    def counts(self, nbytes):
        """(audio outputs per channel, complex RDS outputs) per stream of the NEXT call of nbytes"""
        na, nr = C.c_uint32(), C.c_uint32()
        self._ck(self._lib.sdrfm_bcast_counts(self._h, int(nbytes), C.byref(na), C.byref(nr)), "sdrfm_bcast_counts")
        return na.value, nr.value

    @property
    def kernel_name(self):
        return self._lib.sdrfm_bcast_kernel_name(self._h).decode()

    def hist_kernel_name(self):
        """the kernel a hist call launches now: kernel_name and " + hist" (its step may be the generic one where the plain call's is fast)"""
        return self._lib.sdrfm_bcast_hist_kernel_name(self._h).decode()

    def _entry(self, name, sink, iq, audio, pcm, bb, pc, meters, flags, hist=(None, 0)):
        """one call of the C entry `name` on addresses: iq (address, row stride, nbytes), audio (left, right, row stride), pcm, bb and hist
        (address, row stride).  Raises SdrfmError with the entry's status, returns (n_audio, n_rds)."""
        na, nr = C.c_uint32(), C.c_uint32()
        front, back, counts = (*iq, *audio), (*bb, pc), (C.byref(na), C.byref(nr), flags)
        if name == "sdrfm_bcast_process_batch":
            st = self._lib.sdrfm_bcast_process_batch(self._h, *front, *back, *counts)
        elif name == "sdrfm_bcast_process_batch_pcm":
            st = self._lib.sdrfm_bcast_process_batch_pcm(self._h, sink._h, *front, *pcm, *back, *counts)
        elif name == "sdrfm_bcast_process_batch_metered":
            st = self._lib.sdrfm_bcast_process_batch_metered(self._h, sink._h if sink is not None else None, *front, *pcm, *back, meters, *counts)
        else:
            st = self._lib.sdrfm_bcast_process_batch_metered_hist(self._h, sink._h if sink is not None else None, *front, *pcm, *back, meters, *hist,
                                                                  *counts)
        self._ck(st, name + ("(device)" if flags else ""))
        return na.value, nr.value

    def _host_call(self, name, iq, sink=None, with_audio=True):
        """a host-memory call of the C entry `name`: (L, R, pcm, bb, pilot_count, meters, hist) trimmed to the call's counts, None what the
        call has not — L and R without with_audio, pcm without a sink, meters of any entry but the metered ones, hist of any but the hist one"""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        ns = self.cfg.n_streams
        assert iq.shape[0] == (1 if self._shared_input else ns)                # (a shared capture is one row)
        nbytes = iq.shape[1]
        ca, cr = (max(v, 1) for v in self.counts(nbytes & ~1))
        left = np.zeros((ns, ca), dtype=np.float32) if with_audio else None
        right = np.zeros_like(left) if with_audio else None
        pcm = np.zeros((ns, 2 * ca), dtype=np.int16) if sink is not None else None
        bb = np.zeros((ns, 2 * cr), dtype=np.float32)
        pc = np.zeros(ns, dtype=np.uint32)
        meters = np.zeros(ns, dtype=METER_DTYPE) if "_metered" in name else None
        hist = np.zeros((ns, HIST_BINS), dtype=np.uint32) if name.endswith("_hist") else None
        adr = lambda a: a.ctypes.data if a is not None else None
        na, nr = self._entry(name, sink, (adr(iq), nbytes, nbytes), (adr(left), adr(right), ca), (adr(pcm), 2 * ca), (adr(bb), 2 * cr), adr(pc),
                             adr(meters), 0, (adr(hist), HIST_BINS))
        trim = lambda a, n: a[:, :n] if a is not None else None
        return trim(left, na), trim(right, na), trim(pcm, 2 * na), np.ascontiguousarray(bb[:, : 2 * nr]).view(np.complex64), pc, meters, hist

    def _device_call(self, name, iq, left, right, bb, pilot_count, nbytes, sink=None, pcm=None, meters=None, hist=(None, 0)):
        """a device-tensor call of the C entry `name`, enqueue only: (n_audio, n_rds).  A tensor that is None goes as NULL with stride 0;
        meters is an address, hist an (address, row stride)"""
        adr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        row = lambda t: t.stride(0) if t is not None else 0
        nbytes = iq.shape[1] if nbytes is None else int(nbytes)
        return self._entry(name, sink, (adr(iq), iq.stride(0), nbytes), (adr(left), adr(right), row(left)), (adr(pcm), row(pcm)),
                           (adr(bb), bb.stride(0)), adr(pilot_count), meters, _l.F_DEVICE_PTRS, hist)

    def process_batch(self, iq: np.ndarray):
        """host memory: iq [n_streams, nbytes] uint8 -> (L, R [n_streams, n_audio] float32, bb [n_streams, n_rds] complex64,
        pilot_count [n_streams] uint32)"""
        left, right, _, bb, pc, _, _ = self._host_call("sdrfm_bcast_process_batch", iq)
        return left, right, bb, pc

    def process_batch_device(self, iq, left, right, bb, pilot_count=None, nbytes=None):
        """device tensors: iq uint8 [n_streams, >=nbytes], left / right float32 [n_streams, >= n_audio] (same strides), bb float32
        [n_streams, >= 2 n_rds] ((re, im) pairs), pilot_count int32 / uint32 [n_streams] or None; enqueue only.  Returns (n_audio, n_rds)."""
        assert iq.is_cuda and left.is_cuda and right.is_cuda and bb.is_cuda
        assert left.stride() == right.stride() and left.stride(1) == 1 and bb.stride(1) == 1
        return self._device_call("sdrfm_bcast_process_batch", iq, left, right, bb, pilot_count, nbytes)

    def process_batch_pcm(self, sink, iq: np.ndarray, with_audio=True):
        """sdrfm_bcast_process_batch_pcm on host memory: this call and, behind it, `sink` (a StereoPcmSink) over its L and R rows.
        Returns (L, R, pcm [n_streams, 2 n_audio] int16, bb, pilot_count); with_audio=False passes no audio rows: L and R are None."""
        return self._host_call("sdrfm_bcast_process_batch_pcm", iq, sink, with_audio)[:5]

    def process_batch_pcm_device(self, sink, iq, left, right, pcm, bb, pilot_count=None, nbytes=None):
        """device tensors as process_batch_device takes them, pcm int16 [n_streams, >= 2 n_audio]; left = right = None: the sink reads the
        handle's own rows.  Enqueue only, sink included, on this handle's stream.  Returns (n_audio, n_rds)."""
        assert iq.is_cuda and pcm.is_cuda and bb.is_cuda and pcm.stride(1) == 1 and bb.stride(1) == 1 and (left is None) == (right is None)
        if left is not None:
            assert left.is_cuda and right.is_cuda and left.stride() == right.stride() and left.stride(1) == 1
        return self._device_call("sdrfm_bcast_process_batch_pcm", iq, left, right, bb, pilot_count, nbytes, sink, pcm)

    def process_batch_metered(self, iq: np.ndarray, sink=None, with_audio=True):
        """sdrfm_bcast_process_batch_metered on host memory: what process_batch (sink=None) or process_batch_pcm(sink, iq, with_audio)
        returns and, behind it, the streams' records of the same launch: a scan.METER_DTYPE array [n_streams]."""
        assert with_audio or sink is not None, "without a sink the audio rows are all the audio there is"
        out = self._host_call("sdrfm_bcast_process_batch_metered", iq, sink, with_audio)[:6]
        return out if sink is not None else out[:2] + out[3:]

    def _metered_device_args(self, iq, left, right, bb, meters, sink, pcm):
        """the checks of a metered device call's tensors; returns the address of the records"""
        assert iq.is_cuda and bb.is_cuda and bb.stride(1) == 1 and (left is None) == (right is None)
        assert (sink is None) == (pcm is None) and (sink is not None or left is not None)
        if left is not None:
            assert left.is_cuda and right.is_cuda and left.stride() == right.stride() and left.stride(1) == 1
        if pcm is not None:
            assert pcm.is_cuda and pcm.stride(1) == 1
        if hasattr(meters, "data_ptr"):
            assert meters.is_cuda and meters.is_contiguous() and meters.element_size() * meters.numel() >= 64 * self.cfg.n_streams
            mp = C.c_void_p(meters.data_ptr())
        else:
            mp = C.c_void_p(int(meters)) if meters else None
        return mp

    def process_batch_metered_device(self, iq, left, right, bb, meters, pilot_count=None, nbytes=None, sink=None, pcm=None):
        """device tensors as process_batch_device (sink=None: left and right given, no pcm) or process_batch_pcm_device (sink and pcm given;
        left = right = None: the sink reads the handle's own rows) takes them, and meters: int64 [n_streams, 8] (sdrfm_scan_meter's eight
        words) or the address of n_streams records in device memory, 8-byte aligned.  Enqueue only.  Returns (n_audio, n_rds)."""
        mp = self._metered_device_args(iq, left, right, bb, meters, sink, pcm)
        return self._device_call("sdrfm_bcast_process_batch_metered", iq, left, right, bb, pilot_count, nbytes, sink, pcm, mp)

    def process_batch_metered_hist(self, iq: np.ndarray, sink=None, with_audio=True):
        """sdrfm_bcast_process_batch_metered_hist on host memory: process_batch_metered's tuple and, behind it, the streams' deviation
        histograms of the same launch: uint32 [n_streams, scan.HIST_BINS], what ScanDemod.process_batch_hist gives of the same bytes and
        tuning."""
        assert with_audio or sink is not None, "without a sink the audio rows are all the audio there is"
        out = self._host_call("sdrfm_bcast_process_batch_metered_hist", iq, sink, with_audio)
        return out if sink is not None else out[:2] + out[3:]

    def process_batch_metered_hist_device(self, iq, left, right, bb, meters, hist, pilot_count=None, nbytes=None, sink=None, pcm=None):
        """process_batch_metered_device's tensors and hist: 32-bit integers [n_streams, >= scan.HIST_BINS] with unit stride along a row (a
        row's first HIST_BINS words are overwritten, the rest is left alone).  Enqueue only.  Returns (n_audio, n_rds)."""
        mp = self._metered_device_args(iq, left, right, bb, meters, sink, pcm)
        ns = self.cfg.n_streams
        assert hist.is_cuda and hist.element_size() == 4 and hist.dim() == 2 and hist.shape[0] >= ns and hist.stride(1) == 1, hist.shape
        hist_stride = hist.stride(0) if ns > 1 else max(hist.stride(0), hist.shape[1])
        return self._device_call("sdrfm_bcast_process_batch_metered_hist", iq, left, right, bb, pilot_count, nbytes, sink, pcm, mp,
                                 (C.c_void_p(hist.data_ptr()), hist_stride))
