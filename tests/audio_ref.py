"""Reference of the broadcast receiver's audio conditioning (include/sdrfm.h), shared by the CPU and the GPU tests: the
ramp in Python ints, exactly the header's closed form, and the blend formula with every fp32 rounding made on its own.  It knows nothing
of the library: AudioState mirrors what sdrfm_bcast_set_audio, the calls, reset / tune and sdrfm_bcast_get_audio do to the handle's
numbers."""
import numpy as np

ONE = 32768
J_MAX = 65536


def ramp(x0, xt, slew, n):
    """the value after n outputs: k = min(n, cdiv(|xt - x0|, slew)), x0 + sgn(xt - x0) min(k slew, |xt - x0|)"""
    x0, xt, slew, n = int(x0), int(xt), int(slew), int(n)
    assert 0 <= x0 <= ONE and 0 <= xt <= ONE and 1 <= slew <= ONE and n >= 0
    dist = abs(xt - x0)
    k = min(n, -(-dist // slew))
    move = min(k * slew, dist)
    return x0 + move if xt >= x0 else x0 - move


def ramp_outputs(x0, xt, slew, J, count):
    """the values outputs 0 .. count - 1 of a call use that starts J outputs after the set: output j uses n = J + j + 1"""
    x0, xt, slew, J = int(x0), int(xt), int(slew), int(J)
    assert 0 <= x0 <= ONE and 0 <= xt <= ONE and 1 <= slew <= ONE and J >= 0
    n = J + 1 + np.arange(count, dtype=np.int64)                # ramp() on every n at once: the same first form, in int64
    dist = abs(xt - x0)
    move = np.minimum(np.minimum(n, -(-dist // slew)) * slew, dist)
    return x0 + move if xt >= x0 else x0 - move


def blend(am, as_, b, v):
    """L, R (float32) of the sum channel am and the difference channel as_ under blend b and gain v (Q15 ints, arrays or one value):
    beta = b 2^-15, mu = v 2^-15 exact; t = beta as; L = mu (am + t), R = mu (am - t), each operation rounded to fp32 on its own"""
    am, as_ = np.asarray(am, np.float32), np.asarray(as_, np.float32)
    beta = (np.asarray(b, np.float64) / ONE).astype(np.float32)
    mu = (np.asarray(v, np.float64) / ONE).astype(np.float32)
    t = (beta * as_).astype(np.float32)
    return (mu * (am + t).astype(np.float32)).astype(np.float32), (mu * (am - t).astype(np.float32)).astype(np.float32)


class AudioState:
    """the handle's numbers: per stream (b0, bt, v0, vt), the slew and J"""

    def __init__(self, ns):
        self.ns = ns
        self.b0, self.bt, self.v0, self.vt = (np.full(ns, ONE, np.int64) for _ in range(4))
        self.slew, self.J = ONE, J_MAX

    def now(self):
        """(blend, gain) the next output starts from"""
        return (np.array([ramp(self.b0[s], self.bt[s], self.slew, self.J) for s in range(self.ns)]),
                np.array([ramp(self.v0[s], self.vt[s], self.slew, self.J) for s in range(self.ns)]))

    def set(self, blend_q15, gain_q15, slew):
        self.b0, self.v0 = self.now()
        if blend_q15 is not None:
            self.bt = np.array(np.broadcast_to(np.asarray(blend_q15, np.int64), (self.ns,)))
        if gain_q15 is not None:
            self.vt = np.array(np.broadcast_to(np.asarray(gain_q15, np.int64), (self.ns,)))
        self.slew, self.J = int(slew), 0

    def call(self, count):
        """(b [ns, count], v [ns, count]) of a call's outputs; the count moves on"""
        b = np.stack([ramp_outputs(self.b0[s], self.bt[s], self.slew, self.J, count) for s in range(self.ns)]).reshape(self.ns, count)
        v = np.stack([ramp_outputs(self.v0[s], self.vt[s], self.slew, self.J, count) for s in range(self.ns)]).reshape(self.ns, count)
        self.J = min(J_MAX, self.J + count)
        return b, v

    def complete(self):
        """reset and tune: every ramp at its target"""
        self.J = J_MAX

    def check(self, state):
        """BroadcastDemod.audio_state() against these numbers"""
        b, v = self.now()
        assert np.array_equal(state["blend"], b) and np.array_equal(state["gain"], v), (state, b, v)
        assert np.array_equal(state["blend_target"], self.bt) and np.array_equal(state["gain_target"], self.vt), (state, self.bt, self.vt)
