"""A thin driver of sdrfm_ring_* for tests/test_fm_host_paths_gpu.py and tests/test_ring_gpu.py: status codes, one ring per object, collects into a
canaried buffer (what lies behind n_audio must keep its pattern)."""
import ctypes as C

import numpy as np

OK, BUSY, EINVAL, EODD, ECAPACITY = 0, 1, 16, 17, 18
CANARY = np.float32(-77.25)


def ring_create(lib, dm, n_buffers, buffer_bytes):
    """(status, handle): the handle is NULL after a refusal"""
    out = C.c_void_p(0xDEAD)
    st = lib.sdrfm_ring_create(dm._h, n_buffers, buffer_bytes, C.byref(out))
    return st, out


class Ring:
    def __init__(self, lib, dm, n_buffers, buffer_bytes):
        self.lib, self.dm = lib, dm
        st, self.r = ring_create(lib, dm, n_buffers, buffer_bytes)
        assert st == OK and self.r.value, st
        cfg = dm.cfg
        self.cap = buffer_bytes // 2 // cfg.fir_decim // cfg.audio_decim + 2       # what a slot can hold at any phases
        self.buf = np.full(self.cap + 8, CANARY, np.float32)
        self.n = C.c_uint32()

    def submit(self, chunk):
        chunk = np.asarray(chunk, dtype=np.uint8).reshape(-1)
        keep = chunk.copy() if chunk.size else np.zeros(2, np.uint8)
        st = self.lib.sdrfm_ring_submit(self.r, keep.ctypes.data, chunk.size)
        keep[:] = 0xEE                                                            # the slot owns a copy: the caller's buffer is free again
        return st

    def collect(self, wait, cap=None):
        """(status, audio or None); the canaries behind the audio are checked and restored"""
        self.n.value = 0xFFFF
        cap = self.cap if cap is None else cap
        st = self.lib.sdrfm_ring_collect(self.r, self.buf.ctypes.data, cap, C.byref(self.n), wait)
        if st != OK:
            assert self.n.value == 0, (st, self.n.value)
            assert (self.buf == CANARY).all(), "a refused collect wrote to the caller's buffer"
            return st, None
        n = self.n.value
        assert n <= cap and (self.buf[n:] == CANARY).all(), "collect wrote behind n_audio"
        out = self.buf[:n].copy()
        self.buf[:n] = CANARY
        return st, out

    def collect_polled(self, polls=64):
        """a bounded number of non-blocking collects, then the blocking one: (audio, whether a poll took it)"""
        for _ in range(polls):
            st, out = self.collect(0)
            if st == OK:
                return out, True
            assert st == BUSY, st
        st, out = self.collect(1)
        assert st == OK, st
        return out, False

    def drain(self):
        outs = []
        while True:
            st, out = self.collect(1)
            if st == BUSY:
                return outs
            assert st == OK, st
            outs.append(out)

    def destroy(self):
        if self.r is not None:
            self.lib.sdrfm_ring_destroy(self.r)
            self.r = None


def feed(ring, chunks):
    """Every chunk through the ring as fast as it takes them: a submit that finds the ring full is followed by one blocking collect and made again.
    Returns (audio per chunk in order — a 0-byte chunk takes no slot and gives none —, submits answered SDRFM_BUSY, kernel_name after each submit,
    sdrfm_audio_count's answer right before each submit)."""
    outs, busy, names, counts = [], 0, [], []
    for chunk in chunks:
        counts.append(ring.dm.audio_count(len(chunk)))
        st = ring.submit(chunk)
        if st == BUSY:
            busy += 1
            st, out = ring.collect(1)
            assert st == OK, st
            outs.append(out)
            st = ring.submit(chunk)
        assert st == OK, st
        names.append(ring.dm.kernel_name)
    outs = iter(outs + ring.drain())
    per_chunk = [next(outs) if len(chunk) else np.zeros(0, np.float32) for chunk in chunks]
    assert next(outs, None) is None
    return per_chunk, busy, names, counts
