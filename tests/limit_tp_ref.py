"""The look-ahead PCM limiter's true-peak form (include/sdrfm.h) restated in int64 numpy: what tests/test_limit_tp_cpu.py holds the
C routine to.  The interpolator is a direct convolution over the state's delay line and the call's pairs, the release is iterated one pair at a
time and the windows are taken naively.  It shares nothing with the C routine but the definition; from limit_ref it takes what is common to both
forms (the ramp, the record join, the corners, the cuts and the full-range rows)."""
import numpy as np

from limit_ref import CORNERS, CUTS, DEFAULT, ONE, R_ONE, join, ramp, random_full_range, rec_tuple  # noqa: F401  (re-exported for the tests)

# BS.1770-4 Annex 2 in Q15, typed in from the Recommendation: phases 0 and 1 in units of 2^-13, phases 2 and 3 their reversals
_P0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
_P1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
BS1770 = 4 * np.array([_P0, _P1, _P1[::-1], _P0[::-1]], dtype=np.int64)


def state_init(lw, nt):
    D = (1 << lw) - 1
    return np.concatenate([np.zeros(2 * D + nt, np.int64), np.full(D, ONE, np.int64), np.full(D, R_ONE, np.int64)]).astype(np.int32)


def peaks(xfull, coef, first, n):
    """T for the n pairs that start at entry `first` of xfull int64 [m, 2]: max over channel and phase of |sum_k coef[p][k] x[e - k]|"""
    coef = np.asarray(coef, dtype=np.int64)
    P, NT = coef.shape
    T = np.zeros(n, np.int64)
    for c in range(2):
        for p in range(P):
            full = np.convolve(xfull[:, c], coef[p])                       # full[e] = sum_k coef[p][k] x[e - k], zero outside
            T = np.maximum(T, np.abs(full[first:first + n]))
    return T


def process(x, lw, slew=1, J=0, params=DEFAULT, state=None, coef=BS1770):
    """one stream's call: x int16 [2n] -> (y int16 [2n], state int32 [4 D + NT], (n, limited, min_gain, at), s int64 [n], T int64 [n])"""
    C, delta, g0, gt = (int(v) for v in params)
    coef = np.asarray(coef, dtype=np.int64)
    NT = coef.shape[1]
    D, H = (1 << lw) - 1, NT // 2
    LX = D + H
    assert (1 << lw) >= H and LX >= NT - 1
    st = (state_init(lw, NT) if state is None else np.asarray(state)).astype(np.int64)
    assert st.shape == (4 * D + NT,)
    xin = np.asarray(x, dtype=np.int16).astype(np.int64).reshape(-1, 2)
    n = xin.shape[0]
    G = ramp(g0, gt, slew, J + np.arange(n, dtype=np.int64) + 1)
    xp = (xin * np.reshape(G, (-1, 1)) + 2048) >> 12                     # arithmetic shift
    xfull = np.concatenate([st[:2 * LX].reshape(LX, 2), xp])             # pair i of the call is entry LX + i, its detector pair entry D + i
    T = peaks(xfull, coef, LX, n)
    assert n == 0 or T.max() < 1 << 36
    a = np.maximum(np.abs(xfull[D:D + n]).max(axis=1), (T + 32767) >> 15) if n else np.zeros(0, np.int64)
    g = np.where(a <= C, ONE, (C * ONE) // np.maximum(a, 1))
    gfull = np.concatenate([st[2 * LX:2 * LX + D], g])
    rfull = np.concatenate([st[2 * LX + D:], np.zeros(n, np.int64)])
    y = np.zeros((n, 2), np.int64)
    s_all = np.zeros(n, np.int64)
    for i in range(n):                                                  # detector pair i is entry D + i of g and r
        m = int(gfull[i:i + D + 1].min())
        rfull[D + i] = min(256 * m, int(rfull[D + i - 1]) + delta)
        S = int(rfull[i:i + D + 1].sum())
        assert S <= 1 << 31
        s = S >> (lw + 8)
        s_all[i] = s
        y[i] = (xfull[i] * s + (1 << 14)) >> 15
    assert n == 0 or (-32768 <= y.min() and y.max() <= 32767), "the output left int16: the ceiling does not hold"
    new = np.concatenate([xfull[n:].reshape(-1), gfull[n:], rfull[n:]]).astype(np.int32)
    limited = int((s_all < ONE).sum())
    mg = int(s_all.min()) if n else ONE
    at = int(np.argmax(s_all == mg)) if limited else 0
    return y.astype(np.int16).reshape(-1), new, (n, limited, mg, at), s_all, T


def true_peak(y, coef=BS1770):
    """the true-peak meter's reading of one row int16 [2n] from a zero history, in its units (0 dBTP = 2^30)"""
    v = np.asarray(y, dtype=np.int16).astype(np.int64).reshape(-1, 2)
    return int(peaks(v, coef, 0, v.shape[0]).max()) if v.shape[0] else 0


def fixtures(n=6000, seed=61):
    """the seeded programme fixtures of DESIGN.md §4.25, name -> int16 [2n]: levels that a make-up gain of x 4 carries well over a ceiling of -2 dBFS"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    white = 4000.0 * rng.standard_normal((n, 2))
    low = np.stack([np.convolve(rng.standard_normal(n + 8), np.hanning(9), mode="valid") for _ in range(2)], axis=1)
    low *= 14000.0 / np.abs(low).max()
    tone = 7800.0 * np.sin(np.pi * t / 2 + np.pi / 4)                      # a quarter-rate tone at 45 degrees: its samples are 0.707 of its peak
    am = 10000.0 * (0.6 + 0.4 * np.sin(2 * np.pi * t / 500.0)) * np.sin(2 * np.pi * 0.2503 * t + 0.3)
    square = 9000.0 * np.where((np.arange(n) // 12) % 2, -1.0, 1.0)
    out = {"white": white, "lowpassed": low, "tone45": np.stack([tone, -0.8 * tone], axis=1), "am_hf": np.stack([am, np.roll(am, 3)], axis=1),
           "square": np.stack([square, 0.5 * square], axis=1)}
    return {k: np.clip(np.rint(v), -32768, 32767).astype(np.int16).reshape(-1) for k, v in out.items()}
