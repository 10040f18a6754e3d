"""The PCM mix bus's definition (include/sdrfm.h) restated with Python integers: nothing here can wrap or round on its own, and
nothing is shared with csrc/.  `ramp_at` and `rounding` exist for the mutation check alone (tests/test_pcm_mix_cpu.py): the definition is
ramp_at = 1, rounding = 32768."""
import math

import numpy as np

ONE = 32768
J_MAX = 65536
NONE = 0xFFFFFFFF
STEREO, MONO, LEFT, RIGHT, SWAP = range(5)


def ramp(x0, xt, slew, n):
    """towards xt by at most slew per pair, n pairs after the set"""
    move = min(min(n, J_MAX) * slew, abs(xt - x0))
    return x0 + move if xt >= x0 else x0 - move


def ramp_iterated(x0, xt, slew, n):
    """the same one pair at a time: what the closed form stands for"""
    x = x0
    for _ in range(n):
        x = min(x + slew, xt) if xt >= x else max(x - slew, xt)
    return x


def curve_at(t, g):
    if t is None:
        return g
    if g == ONE:
        return int(t[128])
    j, f = g >> 8, g & 255
    return int(t[j]) + (((int(t[j + 1]) - int(t[j])) * f + 128) >> 8)


def contribution(mode, L, R):
    return {STEREO: (2 * L, 2 * R), MONO: (L + R, L + R), LEFT: (2 * L, 2 * L), RIGHT: (2 * R, 2 * R), SWAP: (2 * R, 2 * L)}[mode]


def curve_ok(t):
    t = [int(v) for v in t]
    return len(t) == 129 and t[0] == 0 and t[128] == ONE and all(b >= a for a, b in zip(t, t[1:]))


def slots_ok(slots, n_in):
    return all((s == NONE or 0 <= s < n_in) and 0 <= m <= 4 and 0 <= g0 <= ONE and 0 <= gt <= ONE for s, m, g0, gt in slots)


def mix_bus(rows, slots, slew, J, curve=None, ramp_at=1, rounding=32768):
    """one bus's call: rows int16 [n_in, 2n], slots a list of (src, mode, g0, gt) -> (out int16 [2n], (n, clipped_l, clipped_r, peak))"""
    n = rows.shape[1] // 2
    data = rows.tolist()
    out = np.zeros(2 * n, np.int16)
    clipped, peak = [0, 0], 0
    for i in range(n):
        acc = [0, 0]
        for src, mode, g0, gt in slots:
            if src == NONE:
                continue
            c = curve_at(curve, ramp(g0, gt, slew, J + i + ramp_at))
            lr = contribution(mode, data[src][2 * i], data[src][2 * i + 1])
            acc[0] += c * lr[0]
            acc[1] += c * lr[1]
        for ch in (0, 1):
            v = (acc[ch] + rounding) >> 16
            y = max(-32768, min(32767, v))
            out[2 * i + ch] = y
            clipped[ch] += v != y
            peak = max(peak, abs(v))
    return out, (n, clipped[0], clipped[1], peak)


def mix(rows, slots, slew, J, curve=None, **kw):
    """every bus: slots [n_bus][n_slots] of 4-tuples -> (out int16 [n_bus, 2n], list of record tuples)"""
    got = [mix_bus(rows, [tuple(int(v) for v in s) for s in bus], slew, J, curve, **kw) for bus in slots]
    return np.stack([g[0] for g in got]), [g[1] for g in got]


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], max(a[3], b[3]))


def rec_tuple(r):
    return tuple(int(r[f]) for f in ("n", "clipped_l", "clipped_r", "peak"))


def report(rec):
    n, cl, cr, peak = rec
    if n == 0:
        return dict(peak_dbfs=math.nan, clipped_frac=math.nan)
    return dict(peak_dbfs=20 * math.log10(peak / 32768) if peak else -math.inf, clipped_frac=(cl + cr) / (2 * n))
