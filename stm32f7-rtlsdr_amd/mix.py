"""PcmMixer — the Python mirror of the sdrfm_pcm_mix_* C entry points: n_bus stereo rows formed from n_in stereo rows on the
device, every bus from n_slots slots that each name a source row, a channel mode and a ramped Q15 gain — station selection and crossfade without
a click; pcm_mix_host, the host routine that defines it; the records' join and report; and the small policies around it: slew_for, fade_pairs
and dead_channel_modes, the actuator for the audio meter's dead-channel alarms."""
import ctypes as C

import numpy as np

from . import lib as _l
from . import taps as _taps

MIX_DTYPE = _l.MIX_DTYPE
MIX_SLOT_DTYPE = _l.MIX_SLOT_DTYPE
MIX_REPORT_FIELDS = tuple(n for n, _ in _l.PcmMixReport._fields_)
SPAN = _l.MIX_SPAN                 # SDRFM_PCM_MIX_SPAN: pairs of a workgroup of k_pcm_mix
NONE = _l.MIX_NONE                 # SDRFM_PCM_MIX_NONE: a slot without a source
N_MAX = 1 << 20                    # pairs per call
ONE = 32768                        # Q15: unity
J_MAX = 65536
SLOTS_MAX = 8
MODES = {"stereo": 0, "mono": 1, "left": 2, "right": 3, "swap": 4}
STEREO, MONO, LEFT, RIGHT, SWAP = 0, 1, 2, 3, 4


def mix_geometry(n_bus, n):
    """the launch geometry of k_pcm_mix (pmix_spans in csrc/sdrfm_pcm_mix.h): (n_bus, spans) workgroups of 256 lanes"""
    return int(n_bus), (int(n) + SPAN - 1) // SPAN


def slew_for(seconds, fs=48000):
    """the slew (Q15 units per pair) with which a gain crosses 0 .. 32768 in `seconds`: round(32768 / (seconds fs)) clamped to 1 .. 32768"""
    pairs = float(seconds) * float(fs)
    if not pairs > 0.0:
        return ONE
    return int(min(ONE, max(1, round(ONE / pairs))))


def fade_pairs(slew):
    """the pairs a full-scale fade takes at `slew`: cdiv(32768, slew)"""
    slew = int(slew)
    if not 1 <= slew <= ONE:
        raise ValueError("fade_pairs: slew %d is outside 1 .. 32768" % slew)
    return -(-ONE // slew)


def dead_channel_modes(alarms):
    """audio_alarms' list -> uint32 [streams] of channel modes: RIGHT where the left channel is dead (the live one on both sides), LEFT where
    the right one is, STEREO elsewhere — a stream that is silent altogether stays STEREO"""
    return np.array([RIGHT if a["left_dead"] else LEFT if a["right_dead"] else STEREO for a in alarms], dtype=np.uint32)


def _mode(m):
    if isinstance(m, str):
        if m not in MODES:
            raise ValueError("PcmMixer: mode %r is none of %s" % (m, ", ".join(MODES)))
        return MODES[m]
    return int(m)


def _curve(curve):
    """None, a name taps.mix_curve knows, or 129 values -> (uint16 [129] contiguous or None)"""
    if curve is None:
        return None
    if isinstance(curve, str):
        return np.ascontiguousarray(_taps.mix_curve(curve))
    c = np.asarray(curve)
    if c.shape != (_l.MIX_CURVE_LEN,) or (c.astype(np.int64) < 0).any() or (c.astype(np.int64) > 0xFFFF).any():
        raise _l.SdrfmError(_l.EINVAL, "the mix bus's curve: 129 uint16 values")
    return np.ascontiguousarray(c, dtype=np.uint16)


def mix_check_curve(curve):
    """sdrfm_pcm_mix_check_curve: True for 129 values that start at 0, end at 32768 and do not decrease"""
    c = np.asarray(curve)
    if c.shape != (_l.MIX_CURVE_LEN,) or (c.astype(np.int64) < 0).any() or (c.astype(np.int64) > 0xFFFF).any():
        return False
    c = np.ascontiguousarray(c, dtype=np.uint16)
    return _l.load_library().sdrfm_pcm_mix_check_curve(c.ctypes.data) == _l.OK


def mix_slots(rows):
    """(src, mode, g0, gt) tuples, or a MIX_SLOT_DTYPE array -> MIX_SLOT_DTYPE, values outside uint32 refused"""
    a = np.asarray(rows)
    if a.dtype == MIX_SLOT_DTYPE:
        return np.ascontiguousarray(a)
    v = np.asarray(rows, dtype=object).reshape(-1, 4)
    if any(not 0 <= int(x) <= 0xFFFFFFFF for x in v.reshape(-1)):
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_mix_slot: a value outside uint32")
    return np.array([tuple(int(x) for x in r) for r in v], dtype=MIX_SLOT_DTYPE)


def pcm_mix_host(pcm, slots, slew=1, J=0, curve=None, acc=None):
    """sdrfm_pcm_mix_s16 (the host-side C routine, the definition of the mix bus), once per bus: pcm int16 [n_in, 2n], L and R interleaved;
    slots [n_bus, n_slots] of (src, mode, g0, gt) (MIX_SLOT_DTYPE or tuples) -> (out int16 [n_bus, 2n], records MIX_DTYPE [n_bus]).  The call's
    records are joined onto acc when that is given."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    n_in, n = rows.shape[0], rows.shape[1] // 2
    sl = np.asarray(slots)
    if sl.dtype != MIX_SLOT_DTYPE:
        shape = np.asarray(slots, dtype=object).shape[:-1]
        sl = mix_slots(slots).reshape(shape)
    sl = np.ascontiguousarray(np.atleast_2d(sl))
    n_bus, n_slots = sl.shape
    if not all(0 <= int(x) <= 0xFFFFFFFF for x in (slew, J)) or n > 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_mix_s16: slew, J or n")
    c = _curve(curve)
    rec = np.zeros(n_bus, MIX_DTYPE) if acc is None else np.ascontiguousarray(np.atleast_1d(acc), dtype=MIX_DTYPE).copy()
    assert rec.shape == (n_bus,), rec.shape
    out = np.zeros((n_bus, 2 * n), np.int16)
    for b in range(n_bus):
        rc = lib.sdrfm_pcm_mix_s16(rows.ctypes.data if n else None, 2 * n, n_in, n, sl[b].ctypes.data, n_slots, int(slew), int(J),
                                   None if c is None else c.ctypes.data, out[b].ctypes.data if n else None, rec.ctypes.data + 32 * b)
        if rc != _l.OK:
            raise _l.SdrfmError(rc, "sdrfm_pcm_mix_s16")
    return out, rec


def mix_add(acc, m):
    """acc = acc joined with m through sdrfm_pcm_mix_add, record by record (MIX_DTYPE arrays of one shape).  Returns acc."""
    lib = _l.load_library()
    assert acc.dtype == MIX_DTYPE and m.dtype == MIX_DTYPE and acc.shape == m.shape and acc.flags.c_contiguous
    m = np.ascontiguousarray(m)
    for k in range(acc.size):
        st = lib.sdrfm_pcm_mix_add(acc.ctypes.data + 32 * k, m.ctypes.data + 32 * k)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_mix_add")
    return acc


def mix_report(records):
    """records -> dict of float64 arrays, one entry per field of sdrfm_pcm_mix_report_t (peak_dbfs, clipped_frac)"""
    lib = _l.load_library()
    records = np.ascontiguousarray(np.atleast_1d(records), dtype=MIX_DTYPE)
    out = {n: np.empty(records.size, np.float64) for n in MIX_REPORT_FIELDS}
    r = _l.PcmMixReport()
    for k in range(records.size):
        st = lib.sdrfm_pcm_mix_report(records.ctypes.data + 32 * k, C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_pcm_mix_report")
        for n in MIX_REPORT_FIELDS:
            out[n][k] = getattr(r, n)
    return out


def crossfade_plan(slots, J, slew, bus, src, mode="stereo"):
    """PcmMixer.crossfade's choice on plain values: slots MIX_SLOT_DTYPE [n_bus, n_slots] and J as get_slots gives them -> (slot, src [n_bus,
    n_slots], mode likewise, target likewise).  The slot is the first of `bus` whose value and target are both 0; it is routed to (src, mode)
    and sent to 32768, the bus's other slots to 0, every other bus keeps its targets.  ValueError where the bus has no such slot."""
    slots = np.asarray(slots)
    n_bus, n_slots = slots.shape
    bus = int(bus)
    if not 0 <= bus < n_bus:
        raise ValueError("crossfade: bus %d of %d" % (bus, n_bus))
    free = None
    for k in range(n_slots):
        s = slots[bus, k]
        g0, gt = int(s["g0"]), int(s["gt"])
        run = min(int(J), J_MAX) * int(slew)                      # audio_ctl_ramp, on Python integers
        now = g0 + min(run, gt - g0) if gt >= g0 else g0 - min(run, g0 - gt)
        if now == 0 and gt == 0:
            free = k
            break
    if free is None:
        raise ValueError("crossfade: every slot of bus %d is in use or still fading" % bus)
    srcs, modes, target = slots["src"].copy(), slots["mode"].copy(), slots["gt"].copy()
    srcs[bus, free], modes[bus, free] = int(src), _mode(mode)
    target[bus, :] = 0
    target[bus, free] = ONE
    return free, srcs, modes, target


class PcmMixer(_l.StreamHandle):
    """The device mix bus (sdrfm_pcm_mix_*): n_bus rows from n_in rows, bit for bit pcm_mix_host.  After create every slot is
    (NONE, stereo, 0, 0): the buses are silent until routed.  curve: None (c = g), "equal_power", "linear" or 129 uint16 values."""
    _destroy = "sdrfm_pcm_mix_destroy"
    _prefix = "sdrfm_pcm_mix"

    def __init__(self, n_in, n_bus, n_slots=2, slew=32, curve=None, device=0):
        self._lib = _l.load_library()
        self.n_in, self.n_bus, self.n_slots, self.slew = int(n_in), int(n_bus), int(n_slots), int(slew)
        if not all(0 <= v <= 0xFFFFFFFF for v in (self.n_in, self.n_bus, self.n_slots, self.slew)):
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_mix_create")
        self.curve = _curve(curve)
        cfg = _l.PcmMixConfig(self.n_in, self.n_bus, self.n_slots, self.slew, 0, device)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_pcm_mix_create(C.byref(cfg), None if self.curve is None else self.curve.ctypes.data, C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_pcm_mix_create")

    def _u32(self, v, where):
        x = [int(e) for e in np.broadcast_to(np.asarray(v, dtype=object), (self.n_bus, self.n_slots)).reshape(-1)]
        if min(x) < 0 or max(x) > 0xFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, where)
        return np.array(x, dtype=np.uint32)

    def kernel_name(self):
        return self._lib.sdrfm_pcm_mix_kernel_name(self._h).decode()

    def reset(self):
        """the records to the identity; the slots, the ramps and J stay"""
        self._ck(self._lib.sdrfm_pcm_mix_reset(self._h), "sdrfm_pcm_mix_reset")

    def set_routes(self, src=None, mode=None):
        """src (a row below n_in, or NONE) and mode (0 .. 4 or a name) per slot, [n_bus, n_slots] or one value for all; None keeps what is set.
        Gains and J are untouched; takes effect with the next call."""
        if mode is not None:
            mode = np.vectorize(_mode, otypes=[object])(np.asarray(mode, dtype=object))
        s = None if src is None else self._u32(src, "sdrfm_pcm_mix_set_routes: src")
        m = None if mode is None else self._u32(mode, "sdrfm_pcm_mix_set_routes: mode")
        self._ck(self._lib.sdrfm_pcm_mix_set_routes(self._h, None if s is None else s.ctypes.data, None if m is None else m.ctypes.data),
                 "sdrfm_pcm_mix_set_routes")

    def set_gains(self, target, jump=False):
        """the gains' targets in Q15 (at most 32768) per slot, [n_bus, n_slots] or one value for all: every ramp restarts where it has got to and
        moves by slew per pair from the next call's first pair on; jump=True sets the gains to their targets at once"""
        g = self._u32(target, "sdrfm_pcm_mix_set_gains")
        self._ck(self._lib.sdrfm_pcm_mix_set_gains(self._h, g.ctypes.data, 1 if jump else 0), "sdrfm_pcm_mix_set_gains")

    def slots(self):
        """(slots MIX_SLOT_DTYPE [n_bus, n_slots] as the next call uses them, J)"""
        sl, J = np.zeros((self.n_bus, self.n_slots), MIX_SLOT_DTYPE), C.c_uint32()
        self._ck(self._lib.sdrfm_pcm_mix_get_slots(self._h, sl.ctypes.data, C.byref(J)), "sdrfm_pcm_mix_get_slots")
        return sl, int(J.value)

    def crossfade(self, bus, src, mode="stereo"):
        """fade `bus` over to (src, mode): a slot of that bus whose value and target are both 0 is routed and sent to 32768, the bus's other
        slots to 0, in one set_gains; the other buses' ramps go on towards their targets.  Returns the slot; ValueError where the bus has
        none free (a fade still running on every slot)."""
        sl, J = self.slots()
        free, srcs, modes, target = crossfade_plan(sl, J, self.slew, bus, src, mode)
        self.set_routes(srcs, modes)
        self.set_gains(target)
        return free

    def read(self, reset=False):
        """the buses' records MIX_DTYPE [n_bus]; reset=True zeroes them behind the copy"""
        rec = np.zeros(self.n_bus, MIX_DTYPE)
        self._ck(self._lib.sdrfm_pcm_mix_read(self._h, rec.ctypes.data, _l.AMETER_F_RESET if reset else 0), "sdrfm_pcm_mix_read")
        return rec

    def read_device(self, out, reset=False):
        """the same into a device tensor of 4 n_bus int64, enqueued on the handle's stream"""
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 32 * self.n_bus
        self._ck(self._lib.sdrfm_pcm_mix_read(self._h, C.c_void_p(out.data_ptr()), _l.F_DEVICE_PTRS | (_l.AMETER_F_RESET if reset else 0)),
                 "sdrfm_pcm_mix_read(device)")

    def process_batch(self, pcm, out=None, n=None):
        """numpy host rows: pcm int16 [n_in, 2n] (L, R interleaved) -> int16 [n_bus, 2n], synchronous.  torch device tensors: pcm int16
        [n_in, >= 2n] and out int16 [n_bus, >= 2n], only enqueued on the handle's stream; returns out."""
        if hasattr(pcm, "is_cuda"):
            return self.process_batch_device(pcm, out, n)
        x = np.ascontiguousarray(pcm, dtype=np.int16)
        if x.ndim == 1:
            x = x[None, :]
        assert x.shape[0] == self.n_in and x.shape[1] % 2 == 0, x.shape
        n = x.shape[1] // 2
        if n > N_MAX:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_mix_process_batch: n")
        y = np.zeros((self.n_bus, 2 * n), np.int16)
        self._ck(self._lib.sdrfm_pcm_mix_process_batch(self._h, x.ctypes.data if n else None, 2 * n, n, y.ctypes.data if n else None, 2 * n, 0),
                 "sdrfm_pcm_mix_process_batch")
        return y

    def process_batch_device(self, pcm_in, pcm_out, n=None):
        assert pcm_in.is_cuda and pcm_out.is_cuda and pcm_in.stride(1) == 1 and pcm_out.stride(1) == 1
        assert pcm_in.shape[0] == self.n_in and pcm_out.shape[0] == self.n_bus, (pcm_in.shape, pcm_out.shape)
        n = min(pcm_in.shape[1], pcm_out.shape[1]) // 2 if n is None else int(n)
        self.process_batch_ptr(pcm_in.data_ptr(), pcm_in.stride(0), n, pcm_out.data_ptr(), pcm_out.stride(0))
        return pcm_out

    def process_batch_ptr(self, in_ptr, in_stride, n, out_ptr, out_stride, flags=_l.F_DEVICE_PTRS):
        """the C call on raw addresses (device memory unless flags says otherwise): rows at any 4-byte aligned address"""
        self._ck(self._lib.sdrfm_pcm_mix_process_batch(self._h, C.c_void_p(int(in_ptr) if in_ptr else None), int(in_stride), int(n),
                                                       C.c_void_p(int(out_ptr) if out_ptr else None), int(out_stride), int(flags)),
                 "sdrfm_pcm_mix_process_batch(ptr)")
