"""The inputs the loudness meter's CPU and GPU tests share, and the tolerances the device is held to.

Geometry: L, NT and TILE are read from csrc/sdrfm_loudness.h, so the lengths below follow the kernel's constants.

Tolerance.  Per sub-block and channel |e - e_host| <= RTOL * e_host + ATOL * block_len, in LSB^2.  tests/test_loudness_emulate_cpu.py measures
tools/loudness_emulate.py (the kernel's order of operations in numpy) against the C routine on these inputs, the two terms separately: a
sub-block whose mean square e_host / block_len is at least LOUD = 1e6 LSB^2 counts towards the relative term, |d| / e_host (MEASURED_REL:
3.17e-11, on the high-pass's decay behind DC), any other towards the absolute term, |d| / block_len (MEASURED_ABS: 3.41e-5 LSB^2 per sample,
on the same decay a little later).  LOUD is where the two capped terms are equal, 1e-3 / 1e-9.  RTOL and ATOL are 8 x the recorded figures,
the room for the device's own evaluation order.  The hard conditions RTOL <= 1e-9 and ATOL <= 1e-3 are no measurements: one lost, doubled
or misplaced sample of a full-range row moves a sub-block by 1 / block_len >= 2e-4 of its energy.

Gate.  GATE_I_DIFF and GATE_LRA_DIFF are the largest differences measured between the C gate's 0.1 LU histograms and exact list gating
(tests/loudness_ref.py) over the EBU programmes and a random programme (measured 0.0039 LU and 0.0495 LU, both on the random programme);
tests/test_loudness_cpu.py asserts them with a margin of 2, far inside the 0.1 LU and 1 LU the specifications allow."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "stm32f7-rtlsdr_amd", "csrc", "sdrfm_loudness.h")).read()
L = int(re.search(r"#define SDRFM_LD_L (\d+)u", _H).group(1))
NT = int(re.search(r"#define SDRFM_LD_NT (\d+)u", _H).group(1))
TILE = L * NT

LOUD = 1e6
MEASURED_REL, MEASURED_ABS = 3.3e-11, 3.5e-5
RTOL, ATOL = 8 * MEASURED_REL, 8 * MEASURED_ABS          # 2.64e-10 and 2.8e-4 LSB^2 per sample
GATE_I_DIFF, GATE_LRA_DIFF = 0.004, 0.05

LENGTHS = (1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, 4800, 2 * TILE + 17)
STREAMS = (1, 3, 65)
BLOCK_LENS = (64, 100, 4800)
SEQUENCE = (1, 0, 2, 4799, 257, 64)


def interleave(Li, Ri):
    Li, Ri = np.asarray(Li), np.asarray(Ri)
    out = np.empty(Li.shape[:-1] + (2 * Li.shape[-1],), np.int16)
    out[..., 0::2], out[..., 1::2] = Li, Ri
    return out


def random_rows(n, ns):
    """random rows over the whole int16 range with stretches of zeros, small values and rails mixed in: (L, R) int64 [ns, n]"""
    rng = np.random.default_rng(7000 + 131 * n + ns)
    Li, Ri = rng.integers(-32768, 32768, (ns, n)), rng.integers(-32768, 32768, (ns, n))
    for ch in (Li, Ri):
        for s in range(ns):
            for _ in range(4):
                a, w = int(rng.integers(0, n)), int(rng.integers(1, 200))
                ch[s, a:a + w] = (0, 0, int(rng.integers(-3, 4)), -32768, 32767)[int(rng.integers(0, 5))]
    return Li, Ri


def hard_rows():
    """name -> list of calls, each (L, R) int64 [2, n]: two streams, the second with L and R exchanged"""
    n = 4800
    t = np.arange(n)
    rng = np.random.default_rng(7001)
    tone = np.rint(32.768 * np.sin(2 * np.pi * 1000.0 * t / 48000.0)).astype(np.int64)       # -60 dBFS
    loud = rng.integers(-32768, 32768, n)
    z = np.zeros(n, np.int64)
    one = {"dc_pos": [(np.full(n, 32767), np.full(n, 32767))] * 2, "dc_neg": [(np.full(n, -32768), np.full(n, -32768))] * 2,
           "burst_then_zeros": [(loud, loud[::-1].copy()), (z, z), (z, z), (z, z)], "tone_m60": [(tone, tone)] * 2, "left_only": [(loud, z)] * 2}
    return {k: [(np.stack([a, b]), np.stack([b, a])) for a, b in calls] for k, calls in one.items()}


def random_programme():
    """120 s of noise whose level moves every 0.5 .. 3 s between -60 and -10 dBFS, L and R different"""
    rng = np.random.default_rng(5)
    parts, total = [], 0
    while total < 120 * 48000:
        n, db = int(rng.integers(24000, 144000)), rng.uniform(-60, -10)
        parts.append(np.rint(32768 * 10 ** (db / 20) * rng.standard_normal(n) / 3))
        total += n
    x = np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)
    return interleave(x, x[::-1].copy())


def measure(got, want, block_len):
    """(worst |d| / e_host over the loud sub-blocks, worst |d| / block_len over the others)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d, loud = np.abs(got - want), want >= LOUD * block_len
    return (float((d[loud] / want[loud]).max()) if loud.any() else 0.0, float(d[~loud].max() / block_len) if (~loud).any() else 0.0)


def within(got, want, block_len):
    """the bound, and for a failing assertion the worst excess"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False, ("shape", got.shape, want.shape)
    d = np.abs(got - want)
    bound = RTOL * want + ATOL * block_len
    ok = bool((d <= bound).all())
    k = np.unravel_index(np.argmax(d - bound), d.shape) if d.size else ()
    return ok, (None if ok else (k, float(got[k]), float(want[k]), float(d[k]), float(bound[k])))


# ---- the EBU programmes: a 1 kHz stereo sine, in phase, quantised to int16; segments of (seconds, dBFS peak) -----------------------------------------
def programme(segments, fs=48000):
    parts, at = [], 0
    for seconds, db in segments:
        n = int(round(seconds * fs))
        t = np.arange(at, at + n)
        parts.append(np.rint(32768.0 * 10.0 ** (db / 20.0) * np.sin(2 * np.pi * 1000.0 * t / fs)))
        at += n
    x = np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)
    return interleave(x, x)


TECH_3341 = {1: ([(20, -23)], -23.0), 2: ([(20, -33)], -33.0), 3: ([(10, -36), (60, -23), (10, -36)], -23.0),
             4: ([(10, -72), (10, -36), (60, -23), (10, -36), (10, -72)], -23.0), 5: ([(20, -26), (20.1, -20), (20, -26)], -23.0)}
TECH_3342 = {1: ([(20, -20), (20, -30)], 10.0), 2: ([(20, -20), (20, -15)], 5.0), 3: ([(20, -40), (20, -20)], 20.0),
             4: ([(20, -50), (20, -35), (20, -20), (20, -35), (20, -50)], 15.0)}
# what exact list gating gives on these (tests/loudness_ref.py)
LIST_I = {1: -22.994, 2: -32.991, 3: -23.014, 4: -23.014, 5: -22.979}
LIST_LRA = {1: 10.00, 2: 5.00, 3: 20.00, 4: 15.00}
