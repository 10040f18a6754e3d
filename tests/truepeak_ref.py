"""The true-peak meter's record (include/sdrfm.h) restated in numpy, independent of the library: record() evaluates the
definition on int16 stereo PCM by an int64 convolution (the GPU tests give it the PCM the device returned), join() is the ordered join.  The
table is written out here a second time, from the issue's integers, so that the library's copy is compared with something."""
import numpy as np

from audio_meter_ref import ALPHA, GAIN, interleave, random_full_range, rows_of   # noqa: F401  (the case helpers are the audio meter's)

DTYPE = np.dtype([(n, "<u8") for n in ("n", "peak_l", "peak_r", "at_l", "at_r", "over_l", "over_r", "reserved")])

# ITU-R BS.1770-4 Annex 2 in units of 2^-13: phases 0 and 1; phase 2 is phase 1 reversed, phase 3 phase 0 reversed
PHASE0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
PHASE1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
BS1770_Q13 = np.array([PHASE0, PHASE1, PHASE1[::-1], PHASE0[::-1]], np.int64)
BS1770 = (4 * BS1770_Q13).astype(np.int16)                                       # Q15
ZERO_DBTP = 1 << 30
LIMIT_M1 = int(np.floor(ZERO_DBTP * 10.0 ** (-1.0 / 20.0)))                      # -1 dBTP


def values(x, coef, hist=None):
    """one channel: int samples [n], the NT - 1 before them (zeros when None) -> A [n, P] in int64, A[i][p] = sum_k coef[p][k] x[i - k]"""
    coef = np.asarray(coef, dtype=np.int64)
    P, NT = coef.shape
    x = np.asarray(x, dtype=np.int64)
    lead = np.zeros(NT - 1, np.int64) if hist is None else np.asarray(hist, dtype=np.int64)
    assert lead.shape == (NT - 1,)
    full = np.concatenate([lead, x])
    out = np.empty((x.size, P), np.int64)
    for p in range(P):
        out[:, p] = np.convolve(full, coef[p])[NT - 1:NT - 1 + x.size]            # integer arithmetic: exact
    return out


def _channel(A, limit):
    if A.shape[0] == 0:
        return 0, 0, 0
    M = np.abs(A)
    per_pair = M.max(axis=1)
    peak = int(per_pair.max())
    at = int(np.argmax(per_pair == peak)) if peak else 0                          # the first pair that attains it
    return peak, at, int((M > limit).sum())


def record(pcm, coef=BS1770, limit=LIMIT_M1, hist=None):
    """one row of interleaved int16 PCM -> (a DTYPE scalar array, the history behind it int16 [2 (NT - 1)]); hist likewise, zeros when None"""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and pcm.size % 2 == 0, (pcm.dtype, pcm.shape)
    NT = np.asarray(coef).shape[1]
    h = np.zeros(2 * (NT - 1), np.int16) if hist is None else np.asarray(hist, dtype=np.int16)
    out = np.zeros((), DTYPE)
    out["n"] = pcm.size // 2
    for ch, name in enumerate("lr"):
        out["peak_" + name], out["at_" + name], out["over_" + name] = _channel(values(pcm[ch::2], coef, h[ch::2]), limit)
    return out, np.concatenate([h, pcm])[-2 * (NT - 1):].copy()


def records(pcm_rows, coef=BS1770, limit=LIMIT_M1, hist=None):
    """[streams, 2n] int16 -> (DTYPE [streams], histories [streams, 2 (NT - 1)])"""
    pcm_rows = np.atleast_2d(pcm_rows)
    got = [record(row, coef, limit, None if hist is None else hist[s]) for s, row in enumerate(pcm_rows)]
    return np.array([g[0] for g in got], dtype=DTYPE), np.array([g[1] for g in got], dtype=np.int16)


def join(a, b):
    """a then b, per include/sdrfm.h, on DTYPE scalars in Python integers"""
    out = np.zeros((), DTYPE)
    out["n"] = int(a["n"]) + int(b["n"])
    for c in "lr":
        out["over_" + c] = int(a["over_" + c]) + int(b["over_" + c])
        if int(b["peak_" + c]) > int(a["peak_" + c]):
            out["peak_" + c], out["at_" + c] = int(b["peak_" + c]), int(a["n"]) + int(b["at_" + c])
        else:
            out["peak_" + c], out["at_" + c] = int(a["peak_" + c]), int(a["at_" + c])
    return out


def same(a, b):
    """integer equality of every field"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 64 and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff(a, b):
    """the fields that differ, for a failing assertion's message"""
    a, b = np.atleast_1d(np.asarray(a)).view(DTYPE), np.atleast_1d(np.asarray(b)).view(DTYPE)
    out = []
    for s in range(min(a.size, b.size)):
        for f in DTYPE.names:
            if int(a[s][f]) != int(b[s][f]):
                out.append((s, f, int(a[s][f]), int(b[s][f])))
    return out[:8]


def trap_row(n=64, coef=BS1770, phase=1):
    """the 32-bit trap: L[i] = 32767 where coef[phase][NT - 1 - i] >= 0, else -32768, for NT pairs, then zeros; R = 0.  At pair NT - 1 the
    phase's whole row lines up with matching signs."""
    c = np.asarray(coef, dtype=np.int64)[phase]
    L = np.zeros(n, np.int64)
    L[:c.size] = np.where(c[::-1] >= 0, 32767, -32768)
    return L, np.zeros(n, np.int64)


def bound_table(P, NT):
    """a table at the half-row bound: in every row either half holds one tap of -32768 and one of -32767 (sum of |coef| = 65535), at places
    that move with the row.  Against a constant -32768 every product is positive: A = 2 * 65535 * 32768 = 4 294 901 760, the top of the key."""
    c = np.zeros((P, NT), np.int16)
    half = NT // 2
    for p in range(P):
        for h in range(2):
            c[p, h * half + p % half] = -32768
            c[p, h * half + (p + 1) % half] = -32767
    return c


BOUND_PEAK = 2 * 65535 * 32768
