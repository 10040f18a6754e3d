"""The look-ahead PCM limiter's definition (include/sdrfm.h) restated in int64 numpy: what tests/test_limit_cpu.py holds the C
routine to.  The release is iterated one pair at a time; the windows are taken naively over the state's lead-in and the call's pairs."""
import numpy as np

ONE, R_ONE = 32768, 1 << 23
DEFAULT = (29204, 874, 4096, 4096)                 # ceiling, release, gain0, gain_t after create
# (ceiling, gain, release): the corners the tests sweep; "any" is taken as the defaults
CORNERS = [(29204, 4096, 874), (1, 65536, 1), (32767, 65536, 1 << 23), (12000, 20000, 5000), (29204, 0, 874)]
CUTS = [1, 0, 2, 30, 31, 32, 1, 1, 1, 257, 64, 0, 3, 700, 5, 1872]
assert sum(CUTS) == 3000


def random_full_range(rng, size):
    """int16 over the whole range, -32768 and 32767 planted"""
    x = rng.integers(-32768, 32768, size=size, dtype=np.int64).astype(np.int16)
    if x.shape[-1] >= 8:
        x[..., [1, 4]] = -32768
        x[..., [2, 7]] = 32767
    return x


def state_init(lw):
    D = (1 << lw) - 1
    return np.concatenate([np.zeros(2 * D, np.int64), np.full(D, ONE, np.int64), np.full(D, R_ONE, np.int64)]).astype(np.int32)


def ramp(x0, xt, slew, n):
    """the gain after n pairs, one step at a time"""
    n = np.minimum(np.asarray(n, dtype=np.int64), 65536)
    dist = abs(int(xt) - int(x0))
    move = np.minimum(n * int(slew), dist)
    return int(x0) + (move if xt >= x0 else -move)


def process(x, lw, slew=1, J=0, params=DEFAULT, state=None):
    """one stream's call: x int16 [2n] -> (y int16 [2n], state int32 [4 D], (n, limited, min_gain, at), s int64 [n])"""
    C, delta, g0, gt = (int(v) for v in params)
    D = (1 << lw) - 1
    st = (state_init(lw) if state is None else np.asarray(state)).astype(np.int64)
    assert st.shape == (4 * D,)
    xin = np.asarray(x, dtype=np.int16).astype(np.int64).reshape(-1, 2)
    n = xin.shape[0]
    G = ramp(g0, gt, slew, J + np.arange(n, dtype=np.int64) + 1)
    xp = (xin * np.reshape(G, (-1, 1)) + 2048) >> 12                     # arithmetic shift
    a = np.abs(xp).max(axis=1) if n else np.zeros(0, np.int64)
    g = np.where(a <= C, ONE, (C * ONE) // np.maximum(a, 1))
    xfull = np.concatenate([st[:2 * D].reshape(D, 2), xp])
    gfull = np.concatenate([st[2 * D:3 * D], g])
    rfull = np.concatenate([st[3 * D:], np.zeros(n, np.int64)])
    y = np.zeros((n, 2), np.int64)
    s_all = np.zeros(n, np.int64)
    for i in range(n):                                                  # pair i is entry D + i
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
    return y.astype(np.int16).reshape(-1), new, (n, limited, mg, at), s_all


def join(a, b):
    """record a then record b"""
    n, lim, mg, at = a
    if b[2] < mg:
        mg, at = b[2], n + b[3]
    return (n + b[0], lim + b[1], mg, at)


def rec_tuple(rec):
    """a LIMIT_DTYPE record as the tuple process returns"""
    return tuple(int(rec[k]) for k in ("n", "limited", "min_gain", "at"))
