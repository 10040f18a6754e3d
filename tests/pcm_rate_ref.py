"""An independent restatement of the PCM rate matcher's definition (include/sdrfm.h) in int64 numpy and Python integers: the
reference of tests/test_pcm_rate_cpu.py (for the C routine) and tests/test_pcm_rate_gpu.py (for the device).  It shares no code with the
library: the counts are Python big-integer arithmetic, the sums one gather and one int64 matrix product per call."""
import numpy as np

ONE = 1 << 32
STEPS = (1 << 30, 1 << 32, ONE + 429497, ONE - 429497, round(48 / 44.1 * ONE), (1 << 34) - 1, 1 << 34)   # 429497 = round(1e-4 2^32)


def shape_of(coef):
    nt = coef.shape[1]
    logph = (coef.shape[0] - 1).bit_length() - 1
    assert coef.shape[0] == (1 << logph) + 1
    return nt, logph


def count(pos, step, n):
    return 0 if pos >= n * ONE else -((pos - n * ONE) // step)          # ceil((n 2^32 - pos) / step)


def process(x, coef, step, pos=0, hist=None):
    """one call: x int16 [2n] interleaved -> (out int16 [2 cnt], pos, hist int16 [2 (NT - 1)])"""
    nt, logph = shape_of(coef)
    x = np.asarray(x, np.int16).reshape(-1, 2)
    n = x.shape[0]
    hist = np.zeros((nt - 1, 2), np.int16) if hist is None else np.asarray(hist, np.int16).reshape(nt - 1, 2)
    ext = np.concatenate([hist, x]).astype(np.int64)                     # ext[i + nt - 1] = x[i]
    cnt = count(pos, step, n)
    P = [pos + j * step for j in range(cnt)]
    i = np.array([v >> 32 for v in P], np.int64)
    f = np.array([v & 0xFFFFFFFF for v in P], np.int64)
    p, mu = f >> (32 - logph), (f >> (24 - logph)) & 255
    out = np.zeros((cnt, 2), np.int16)
    if cnt:
        taps = ext[i[:, None] + np.arange(nt)[None, :]]                  # [cnt, nt, 2]: x[i - nt + 1 + k]
        c = coef.astype(np.int64)
        a0 = np.einsum("jk,jkc->jc", c[p], taps)
        a1 = np.einsum("jk,jkc->jc", c[p + 1], taps)
        acc = a0 * (256 - mu)[:, None] + a1 * mu[:, None]
        out = np.clip((acc + (1 << 22)) >> 23, -32768, 32767).astype(np.int16)
    return out.reshape(-1), pos + cnt * step - n * ONE, ext[ext.shape[0] - (nt - 1):].astype(np.int16).reshape(-1)


def process_fast(x, coef, step, pos=0, hist=None, chunk=1 << 16):
    """process() for calls of up to 2^20 pairs: the phases as one uint64 numpy progression (pos + cnt step < 2^32 (n + 4) <= 2^53, no wrap) and the
    sums `chunk` outputs at a time.  tests/test_pcm_rate_cpu.py holds it to process()"""
    nt, logph = shape_of(coef)
    x = np.asarray(x, np.int16).reshape(-1, 2)
    n = x.shape[0]
    hist = np.zeros((nt - 1, 2), np.int16) if hist is None else np.asarray(hist, np.int16).reshape(nt - 1, 2)
    ext = np.concatenate([hist, x]).astype(np.int64)
    cnt = count(pos, step, n)
    assert 0 <= pos < 1 << 53 and pos + cnt * step < 1 << 53
    c = coef.astype(np.int64)
    out = np.zeros((cnt, 2), np.int16)
    for a in range(0, cnt, chunk):
        P = np.uint64(pos) + np.arange(a, min(a + chunk, cnt), dtype=np.uint64) * np.uint64(step)
        i, f = (P >> np.uint64(32)).astype(np.int64), (P & np.uint64(0xFFFFFFFF)).astype(np.int64)
        p, mu = f >> (32 - logph), (f >> (24 - logph)) & 255
        taps = ext[i[:, None] + np.arange(nt)[None, :]]
        acc = np.einsum("jk,jkc->jc", c[p], taps) * (256 - mu)[:, None] + np.einsum("jk,jkc->jc", c[p + 1], taps) * mu[:, None]
        out[a:a + P.size] = np.clip((acc + (1 << 22)) >> 23, -32768, 32767)
    return out.reshape(-1), pos + cnt * step - n * ONE, ext[ext.shape[0] - (nt - 1):].astype(np.int16).reshape(-1)


def run(x, coef, step, cuts, pos=0, hist=None):
    """the row cut into calls of the given lengths (pairs): (the outputs of every call, pos after every call, final hist)"""
    outs, poss, at = [], [], 0
    for c in cuts:
        o, pos, hist = process(x[2 * at:2 * (at + c)], coef, step, pos, hist)
        outs.append(o)
        poss.append(pos)
        at += c
    return outs, poss, hist


def random_full_range(rng, shape):
    """int16 over the whole range, with both rails present"""
    x = rng.integers(-32768, 32768, shape).astype(np.int16)
    flat = x.reshape(-1)
    if flat.size >= 4:
        flat[:2], flat[-2:] = -32768, 32767
    return x


def bound_table(nt, logph, rng=None):
    """a legal table with the sum of |coef| EXACTLY 65535 in both halves of every row, at any tap count (small_table's clip to int16 can leave a
    half row of two or four taps short of it): random magnitudes of at most 32767 with random signs; a half row of two taps is -32768 beside
    +-32767, the only way two int16 reach 65535"""
    rng = np.random.default_rng(nt * 32 + logph) if rng is None else rng
    rows, half = (1 << logph) + 1, nt // 2
    c = np.zeros((rows, nt), np.int64)
    for p in range(rows):
        for h in range(2):
            if half == 2:
                seg = np.array([-32768, 32767 * int(rng.choice((-1, 1)))])[:: int(rng.choice((-1, 1)))]
            else:
                w = rng.random(half) + 0.05
                mag = np.minimum(np.floor(w * (65535 / w.sum())).astype(np.int64), 32767)
                while mag.sum() < 65535:                                   # hand the remainder to the taps that have room, largest first
                    k = int(np.argmax(np.where(mag < 32767, mag, -1)))
                    mag[k] += min(65535 - int(mag.sum()), 32767 - int(mag[k]))
                seg = mag * rng.choice((-1, 1), half)
            c[p, h * half:(h + 1) * half] = seg
    assert (np.abs(c[:, :half]).sum(axis=1) == 65535).all() and (np.abs(c[:, half:]).sum(axis=1) == 65535).all()
    return c.astype(np.int16)


def small_table(nt, logph, rng=None, overshoot=False):
    """a legal table that is no window design: random taps scaled so that every half row's sum of |coef| is at most 65535 — with overshoot exactly
    65535 in both halves of every row, which full-range input drives into both rails"""
    rng = np.random.default_rng(nt * 16 + logph) if rng is None else rng
    rows, half = (1 << logph) + 1, nt // 2
    c = rng.integers(-20000, 20001, (rows, nt)).astype(np.int64)
    for p in range(rows):
        for h in range(2):
            seg = c[p, h * half:(h + 1) * half]
            s = int(np.abs(seg).sum())
            limit = 65535 if overshoot else 30000
            if s == 0:
                seg[0] = 1
                s = 1
            seg[:] = np.trunc(seg * (limit / s))
            if overshoot:                                                  # top up the largest tap to the bound exactly
                k = int(np.argmax(np.abs(seg)))
                seg[k] += (limit - int(np.abs(seg).sum())) * (1 if seg[k] >= 0 else -1)
            c[p, h * half:(h + 1) * half] = np.clip(seg, -32768, 32767)
    return c.astype(np.int16)
