"""Reference of the stereo PCM sink's ramped high-cut (include/sdrfm.h), shared by the CPU and the GPU tests: the definition
restated in numpy fp32, one rounding at a time, with the ramp in Python ints.  It knows nothing of the library: HicutState mirrors what
sdrfm_pcm_stereo_sink_set_hicut, the calls, reset and sdrfm_pcm_stereo_sink_get_hicut do to the sink's numbers.

    h[i]     = h0 moved towards ht by min(min(J + i + 1, 65536) slew, |ht - h0|)
    alpha[i] = alpha * ((float)h[i] * 2^-15)            the inner product exact, the outer one rounded once
    y[i]     = fmaf(alpha[i], x[i] - y[i-1], y[i-1])    one rounded difference, one fused multiply-add (fma32: exact product, exact sum, one rounding)
    pcm[i]   = (int16) rint(clamp(y[i] * gain, -32768, 32767))
"""
import numpy as np

F = np.float32
ONE, HMIN, J_MAX = 32768, 1024, 65536


def ramp(h0, ht, slew, n):
    """the value after n samples (n = 0: h0 itself), in Python ints: "move towards the target by at most slew per sample" in closed form"""
    h0, ht, slew, n = int(h0), int(ht), int(slew), int(n)
    assert HMIN <= h0 <= ONE and HMIN <= ht <= ONE and 1 <= slew <= ONE and n >= 0
    move = min(min(n, J_MAX) * slew, abs(ht - h0))
    return h0 + move if ht >= h0 else h0 - move


def ramp_samples(h0, ht, slew, J, count):
    """the values samples 0 .. count - 1 of a call use that starts J samples after the set: sample i uses n = J + i + 1"""
    return np.array([ramp(h0, ht, slew, min(int(J), J_MAX) + i + 1) for i in range(count)], dtype=np.int64)


def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product of two floats is exact in float64; the sum is taken in float64 with its exact
    residual (two-sum) and rounded to ODD where it is inexact, so that the final rounding to float32 (24 of 53 bits) is the only one"""
    p = np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, F).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F)


def alphas(alpha, h):
    """alpha[i] of the Q15 values h: (float)h * 2^-15 is exact, the product with alpha rounded once"""
    return (F(alpha) * (np.asarray(h, np.int64).astype(F) * F(2.0 ** -15))).astype(F)


def pcm_word(v):
    return np.rint(np.clip(np.asarray(v, F), F(-32768.0), F(32767.0))).astype(np.int16)


def hicut_ref(left, right, alpha, gain, h0, ht, slew, J=0, state=None):
    """left, right float32 [ns, n]; h0, ht one Q15 value or one per stream -> (pcm int16 [ns, 2n] interleaved L, R; state float32 [ns, 2]).
    Vectorised over the streams, one sample at a time."""
    x = np.stack([np.asarray(left, F), np.asarray(right, F)], axis=1)           # [ns, 2, n]
    ns, n = x.shape[0], x.shape[2]
    h0 = np.broadcast_to(np.asarray(h0, np.int64), (ns,))
    ht = np.broadcast_to(np.asarray(ht, np.int64), (ns,))
    h = np.stack([ramp_samples(h0[s], ht[s], slew, J, n) for s in range(ns)]).reshape(ns, n)
    al = alphas(alpha, h)
    y = np.zeros((ns, 2), F) if state is None else np.array(state, F).reshape(ns, 2)
    gain = F(gain)
    pcm = np.zeros((ns, 2 * n), np.int16)
    for i in range(n):
        a = al[:, i, None]
        y = fma32(a, (x[:, :, i] - y).astype(F), y)
        w = pcm_word((y * gain).astype(F))
        pcm[:, 2 * i], pcm[:, 2 * i + 1] = w[:, 0], w[:, 1]
    return pcm, y


class HicutState:
    """the sink's numbers: per stream (h0, ht), the slew and J; conditioned or not"""

    def __init__(self, ns):
        self.ns = ns
        self.h0, self.ht = np.full(ns, ONE, np.int64), np.full(ns, ONE, np.int64)
        self.slew, self.J, self.on = ONE, J_MAX, False

    def now(self):
        return np.array([ramp(self.h0[s], self.ht[s], self.slew, self.J) for s in range(self.ns)], dtype=np.int64)

    def set(self, hicut_q15, slew):
        if not slew:
            self.__init__(self.ns)
            return
        self.h0 = self.now()
        if hicut_q15 is not None:
            self.ht = np.array(np.broadcast_to(np.asarray(hicut_q15, np.int64), (self.ns,)))
        self.slew, self.J, self.on = int(slew), 0, True

    def call(self, count):
        """what a call of count samples is to be referred to: (h0, ht, slew, J) before it; the count moves on"""
        at = (self.h0.copy(), self.ht.copy(), self.slew, self.J)
        self.J = min(J_MAX, self.J + count)
        return at

    def complete(self):
        self.J = J_MAX

    def check(self, got):
        """StereoPcmSink.hicut_state() against these numbers"""
        h, t, slew = got
        assert np.array_equal(h, self.now()) and np.array_equal(t, self.ht) and slew == (self.slew if self.on else 0), (got, self.now(), self.ht, self.slew)
