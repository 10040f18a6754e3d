"""K-weighted loudness (ITU-R BS.1770-4 / EBU R 128) over the C library: the host routine that defines the sub-block energies,
the gate that turns them into momentary, short-term and integrated loudness and loudness range, and a monitor over the reads of a
StereoPcmSink with loudness enabled."""
import ctypes as C

import numpy as np

from . import lib as _l

LOUDNESS_STATE_DTYPE = _l.LOUDNESS_STATE_DTYPE
LOUDNESS_REPORT_FIELDS = tuple(n for n, _ in _l.LoudnessReport._fields_)


def loudness_default_coef():
    """sdrfm_loudness_default_coef: the 48 kHz K-weighting of BS.1770-4 as float64 [10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2"""
    out = np.zeros(10, np.float64)
    st = _l.load_library().sdrfm_loudness_default_coef(out.ctypes.data)
    if st != _l.OK:
        raise _l.SdrfmError(st, "sdrfm_loudness_default_coef")
    return out


def pcm_loudness_host(pcm, block_len=4800, coef=None, state=None):
    """sdrfm_pcm_loudness_s16 (the host-side C routine, the definition of the sub-block energies): pcm int16 [2n] or [streams, 2n], L and R
    interleaved -> (energies float64 [streams, n_blocks, 2], state LOUDNESS_STATE_DTYPE [streams]).  state: what an earlier call returned
    (zero when None); every row must be at the same pos."""
    lib = _l.load_library()
    rows = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.int16)
    assert rows.ndim == 2 and rows.shape[1] % 2 == 0, rows.shape
    ns, n = rows.shape[0], rows.shape[1] // 2
    c = loudness_default_coef() if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    if c.shape != (10,) or not 0 <= int(block_len) <= 0xFFFFFFFF:
        raise _l.SdrfmError(_l.EINVAL, "sdrfm_pcm_loudness_s16: coef or block_len")
    st = np.zeros(ns, dtype=LOUDNESS_STATE_DTYPE) if state is None else np.ascontiguousarray(np.atleast_1d(state), dtype=LOUDNESS_STATE_DTYPE).copy()
    assert st.shape == (ns,) and (st["pos"] == st["pos"][0]).all(), st.shape
    cap = n // max(int(block_len), 1) + 1
    out = np.zeros((ns, cap, 2), np.float64)
    nb = C.c_uint32(0)
    for s in range(ns):
        rc = lib.sdrfm_pcm_loudness_s16(rows[s].ctypes.data if n else None, n, c.ctypes.data, int(block_len), st.ctypes.data + 88 * s,
                                        out[s].ctypes.data, cap, C.byref(nb))
        if rc != _l.OK:
            raise _l.SdrfmError(rc, "sdrfm_pcm_loudness_s16")
    return np.ascontiguousarray(out[:, :nb.value]), st


class LoudnessGate:
    """One stream's gate (sdrfm_loudness_gate_*): push(energies [n, 2]) takes CONSECUTIVE sub-block energies, report() gives a dict of m, s, i,
    lra, max_m, max_s (LUFS, LU) and the block counts.  The windows of 4 and 30 sub-blocks are 400 ms and 3 s only when block_len is a tenth
    of a second."""

    def __init__(self, block_len=4800):
        self._lib = _l.load_library()
        self._h = C.c_void_p()
        if not 0 <= int(block_len) <= 0xFFFFFFFF:
            raise _l.SdrfmError(_l.EINVAL, "sdrfm_loudness_gate_create: block_len")
        st = self._lib.sdrfm_loudness_gate_create(int(block_len), C.byref(self._h))
        if st != _l.OK:
            self._h = None
            raise _l.SdrfmError(st, "sdrfm_loudness_gate_create")
        self.block_len = int(block_len)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdrfm_loudness_gate_free(self._h)
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

    def push(self, energies):
        e = np.ascontiguousarray(energies, dtype=np.float64).reshape(-1, 2)
        st = self._lib.sdrfm_loudness_gate_push(self._h, e.ctypes.data if e.shape[0] else None, e.shape[0])
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_loudness_gate_push")

    def reset(self):
        st = self._lib.sdrfm_loudness_gate_reset(self._h)
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_loudness_gate_reset")

    def report(self):
        r = _l.LoudnessReport()
        st = self._lib.sdrfm_loudness_gate_report(self._h, C.byref(r))
        if st != _l.OK:
            raise _l.SdrfmError(st, "sdrfm_loudness_gate_report")
        return {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in _l.LoudnessReport._fields_}


# loudness_alarms' tolerance around the target, in LU: EBU R 128 allows +-1 LU for live programmes
LOUDNESS_TOL = 1.0


def loudness_alarms(summary, target=-23.0, tol=LOUDNESS_TOL):
    """What a LoudnessMonitor.summary() says about the programmes against a target integrated loudness, one dict per stream:
      too_loud   the integrated loudness lies more than tol LU above target
      too_quiet  it lies more than tol LU below (a programme that never passed the absolute gate, i = -inf, is too quiet)
      gap        sub-blocks were lost between two reads, so i and lra cover less than the programme
    A NaN (too few sub-blocks yet) raises neither level alarm."""
    out = []
    with np.errstate(invalid="ignore"):
        for s in summary:
            i = float(s["i"])
            out.append(dict(too_loud=bool(i > target + tol), too_quiet=bool(i < target - tol), gap=bool(s.get("gaps", 0))))
    return out


class LoudnessMonitor:
    """Loudness monitoring over the reads of a StereoPcmSink with loudness enabled: push(first_block, energies) takes one
    read_loudness() and feeds every stream's LoudnessGate; summary() reads them.  A gap in first_block — the ring was overrun between two
    reads — is REPORTED, not bridged: the gates are reset, since their windows need consecutive sub-blocks, and the summary counts the gaps
    and the sub-blocks lost."""

    def __init__(self, n_streams, block_len=4800):
        self.n_streams, self.block_len = int(n_streams), int(block_len)
        self.gates = [LoudnessGate(block_len) for _ in range(self.n_streams)]
        self.next_block, self.gaps, self.lost, self.reads = 0, 0, 0, 0

    def close(self):
        for g in self.gates:
            g.close()

    def push(self, first_block, energies):
        """returns the sub-blocks lost before this read (0: it follows the last one)"""
        e = np.asarray(energies, dtype=np.float64)
        assert e.ndim == 3 and e.shape[0] == self.n_streams and e.shape[2] == 2, e.shape
        first_block = int(first_block)
        assert first_block >= self.next_block or e.shape[1] == 0, (first_block, self.next_block)
        lost = first_block - self.next_block if e.shape[1] else 0
        if lost:
            self.gaps += 1
            self.lost += lost
            for g in self.gates:
                g.reset()
        for s, g in enumerate(self.gates):
            g.push(e[s])
        if e.shape[1]:
            self.next_block = first_block + e.shape[1]
        self.reads += 1
        return lost

    def summary(self):
        """one dict per stream: stream, reads, gaps, lost and every field of the gate's report"""
        return [dict(stream=s, reads=self.reads, gaps=self.gaps, lost=self.lost, **g.report()) for s, g in enumerate(self.gates)]
