"""RDS reception: RdsDemod mirrors the sdrfm_rds_* C entry points (IQ bytes -> complex RDS baseband on the GPU),
RdsSync mirrors sdrfm_rds_sync_* (baseband -> groups, plain C on the host), rds_parse reads PI / PTY / PS / radio text out of
groups, and rds_encode_groups / rds_group_bits make a payload for siggen.make_iq_rds (pure Python, independent of the C code)."""
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import lib as _l
from .stereo import _pilot_floats

CFG_FORCE_GENERIC = 1   # SDRFM_RDS_CFG_FORCE_GENERIC (include/sdrfm.h)
BITRATE = 1187.5
POLY = 0x5B9
OFFSET_WORDS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)   # A B C C' D


@dataclass
class RdsConfig:
    fir_coeffs: np.ndarray            # h[0..T): channel low-pass at fs
    pilot_coeffs: np.ndarray          # b[0..P): complex taps, P odd (taps.stereo_pilot_taps)
    rds_coeffs: np.ndarray            # g[0..Tr): low-pass at fs/D behind the 57 kHz mixer (taps.rds_lowpass_taps)
    pilot_min: float = 0.05           # |q| below this (radians) is "no pilot": w = 0
    rds_gain: float = 2.0             # taps.rds_gain(D, fs) compensates the discriminator's boxcar
    fir_decim: int = 10
    rds_decim: int = 25
    n_streams: int = 1
    max_bytes_per_call: int = 1 << 20
    device: int = 0
    force_generic: bool = False       # SDRFM_RDS_CFG_FORCE_GENERIC (tests): never the fast kernel


class RdsDemod(_l.StreamHandle):
    _destroy = "sdrfm_rds_destroy"
    _prefix = "sdrfm_rds"

    def __init__(self, cfg: RdsConfig):
        self._lib = _l.load_library()
        self.cfg = cfg
        self._hc = np.ascontiguousarray(cfg.fir_coeffs, dtype=np.float32)
        self._gc = np.ascontiguousarray(cfg.rds_coeffs, dtype=np.float32)
        self._bc = _pilot_floats(cfg.pilot_coeffs)
        fp = C.POINTER(C.c_float)
        c = _l.RdsConfig()
        c.struct_size = C.sizeof(_l.RdsConfig)
        c.n_streams = cfg.n_streams
        c.fir_taps, c.fir_decim, c.fir_coeffs = self._hc.size, cfg.fir_decim, self._hc.ctypes.data_as(fp)
        c.pilot_taps, c.pilot_coeffs = self._bc.size // 2, self._bc.ctypes.data_as(fp)
        c.pilot_min, c.rds_gain = float(cfg.pilot_min), float(cfg.rds_gain)
        c.rds_taps, c.rds_decim, c.rds_coeffs = self._gc.size, cfg.rds_decim, self._gc.ctypes.data_as(fp)
        c.max_bytes_per_call, c.device = cfg.max_bytes_per_call, cfg.device
        c.flags = CFG_FORCE_GENERIC if cfg.force_generic else 0
        self._h = C.c_void_p()
        st = self._lib.sdrfm_rds_create(C.byref(c), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_rds_create")

    def reset(self):
        self._ck(self._lib.sdrfm_rds_reset(self._h), "sdrfm_rds_reset")

    def count(self, nbytes):
        """complex outputs per stream of the NEXT call of nbytes"""
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_rds_count(self._h, int(nbytes), C.byref(n)), "sdrfm_rds_count")
        return n.value

    @property
    def kernel_name(self):
        return self._lib.sdrfm_rds_kernel_name(self._h).decode()

    def process_batch(self, iq: np.ndarray):
        """host memory: iq [n_streams, nbytes] uint8 -> (bb [n_streams, n_out] complex64, pilot_count [n_streams] uint32)"""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == self.cfg.n_streams
        nbytes = iq.shape[1]
        cap = max(self.count(nbytes & ~1), 1)
        bb = np.zeros((iq.shape[0], 2 * cap), dtype=np.float32)
        pc = np.zeros(iq.shape[0], dtype=np.uint32)
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_rds_process_batch(self._h, iq.ctypes.data, nbytes, nbytes, bb.ctypes.data, 2 * cap, pc.ctypes.data,
                                                   C.byref(n), 0), "sdrfm_rds_process_batch")
        return np.ascontiguousarray(bb[:, : 2 * n.value]).view(np.complex64), pc

    def process_batch_device(self, iq, bb, pilot_count=None, nbytes=None):
        """device tensors: iq uint8 [n_streams, >=nbytes], bb float32 [n_streams, >= 2 n_out] ((re, im) pairs), pilot_count int32 /
        uint32 [n_streams] or None; enqueue only.  Returns n_out."""
        assert iq.is_cuda and bb.is_cuda and bb.stride(1) == 1
        nbytes = iq.shape[1] if nbytes is None else int(nbytes)
        pc = C.c_void_p(pilot_count.data_ptr()) if pilot_count is not None else None
        n = C.c_uint32()
        self._ck(self._lib.sdrfm_rds_process_batch(self._h, C.c_void_p(iq.data_ptr()), iq.stride(0), nbytes, C.c_void_p(bb.data_ptr()),
                                                   bb.stride(0), pc, C.byref(n), _l.F_DEVICE_PTRS), "sdrfm_rds_process_batch(device)")
        return n.value


RdsGroup = namedtuple("RdsGroup", "blocks ok_mask version_b")


class RdsSync:
    """one stream's bit clock, differential decoder and block synchronisation (sdrfm_rds_sync_*); no GPU"""

    def __init__(self, sample_rate_hz=9600.0):
        self._lib = _l.load_library()
        self.sample_rate_hz = float(sample_rate_hz)
        self._h = C.c_void_p()
        st = self._lib.sdrfm_rds_sync_create(self.sample_rate_hz, C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_rds_sync_create")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdrfm_rds_sync_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        st = self._lib.sdrfm_rds_sync_reset(self._h)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_rds_sync_reset")

    def push(self, bb):
        """bb: complex64 [n] (or float32 [2n] of (re, im) pairs) -> list of RdsGroup"""
        bb = np.asarray(bb)
        if np.iscomplexobj(bb):
            bb = np.ascontiguousarray(bb, dtype=np.complex64).view(np.float32)
        bb = np.ascontiguousarray(bb, dtype=np.float32).reshape(-1)
        n = bb.size // 2
        cap = int(n / (104 * self.sample_rate_hz / BITRATE)) + 3
        out = (_l.RdsGroup * cap)()
        got = C.c_uint32()
        st = self._lib.sdrfm_rds_sync_push(self._h, bb.ctypes.data, n, out, cap, C.byref(got))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_rds_sync_push")
        return [RdsGroup(tuple(int(v) for v in out[i].block), int(out[i].ok_mask), int(out[i].version_b)) for i in range(got.value)]

    def stats(self):
        info = _l.RdsSyncInfo()
        st = self._lib.sdrfm_rds_sync_stats(self._h, C.byref(info))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_rds_sync_stats")
        return dict(bits=info.bits, blocks_ok=info.blocks_ok, blocks_failed=info.blocks_failed, in_sync=bool(info.in_sync), groups=info.groups)


# ---- the payload side, in Python (what a transmitter does; used by siggen.make_iq_rds and as the tests' known answers) ----------
def rds_checkword(info, offset):
    """(info x^10 mod g(x)) xor offset word; offset 0..4 = A, B, C, C', D"""
    r = (int(info) & 0xFFFF) << 10
    for i in range(25, 9, -1):
        if r & (1 << i):
            r ^= POLY << (i - 10)
    return (r & 0x3FF) ^ OFFSET_WORDS[offset]


def rds_group_bits(blocks):
    """the 104 bits of one group, first transmitted first: 4 x (16 information bits, msb first, + 10 check bits); block 3 takes
    offset C' in a version B group (bit 11 of block 2)"""
    ver_b = (int(blocks[1]) >> 11) & 1
    bits = []
    for i, info in enumerate(blocks):
        off = (0, 1, 3 if ver_b else 2, 4)[i]
        word = ((int(info) & 0xFFFF) << 10) | rds_checkword(info, off)
        bits += [(word >> (25 - k)) & 1 for k in range(26)]
    return bits


def rds_encode_groups(pi, ps, text="", pty=0):
    """the groups of one cycle: four 0A groups carrying the 8-character PS name, then one 2A group per 4 characters of the radio text
    (a text shorter than 64 characters ends with a carriage return, as the standard asks, and is padded to whole groups)"""
    ps = (ps + " " * 8)[:8].encode("latin-1")
    groups = []
    for seg in range(4):
        b2 = (0 << 12) | (0 << 11) | ((pty & 31) << 5) | (1 << 3) | (((3 - seg) == 0) << 2) | seg
        groups.append((pi & 0xFFFF, b2, 0xE0CD, (ps[2 * seg] << 8) | ps[2 * seg + 1]))
    rt = text.encode("latin-1")[:64]
    if rt:
        if len(rt) < 64:
            rt += b"\r"
        rt += b" " * (-len(rt) % 4)
        for seg in range(len(rt) // 4):
            b2 = (2 << 12) | (0 << 11) | ((pty & 31) << 5) | seg
            groups.append((pi & 0xFFFF, b2, (rt[4 * seg] << 8) | rt[4 * seg + 1], (rt[4 * seg + 2] << 8) | rt[4 * seg + 3]))
    return groups


def rds_parse(groups):
    """PI, PTY, the PS name (groups 0A / 0B) and the radio text (2A) out of RdsGroups, only from blocks whose ok_mask bit is set.
    Returns dict(pi, pty, ps, text): pi / pty the most frequent values (None without any), ps None until all 8 characters came,
    text up to the carriage return (or all 64 characters, trailing blanks dropped); None until every segment before the end came."""
    pis, ptys = {}, {}
    ps = [None] * 8
    rt = [None] * 64
    for g in groups:
        b, ok = g.blocks, g.ok_mask
        if ok & 1:
            pis[b[0]] = pis.get(b[0], 0) + 1
        if not ok & 2:
            continue
        gtype, ver = b[1] >> 12, (b[1] >> 11) & 1
        p = (b[1] >> 5) & 31
        ptys[p] = ptys.get(p, 0) + 1
        if gtype == 0 and ok & 8:
            seg = b[1] & 3
            ps[2 * seg], ps[2 * seg + 1] = b[3] >> 8, b[3] & 0xFF
        elif gtype == 2 and ver == 0:
            seg = b[1] & 15
            if ok & 4:
                rt[4 * seg], rt[4 * seg + 1] = b[2] >> 8, b[2] & 0xFF
            if ok & 8:
                rt[4 * seg + 2], rt[4 * seg + 3] = b[3] >> 8, b[3] & 0xFF
    top = lambda d: max(d, key=d.get) if d else None
    text = None
    end = rt.index(0x0D) if 0x0D in rt else 64
    if all(c is not None for c in rt[:end]) and (end < 64 or rt[0] is not None):
        text = bytes(rt[:end]).decode("latin-1")
        if end == 64:
            text = text.rstrip(" ")
    return dict(pi=top(pis), pty=top(ptys), ps=bytes(ps).decode("latin-1") if all(c is not None for c in ps) else None, text=text)
