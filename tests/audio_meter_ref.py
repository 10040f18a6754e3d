"""The audio meter's record (include/sdrfm.h) restated in numpy, independent of the library: record() evaluates the definition
on int16 stereo PCM (the GPU tests give it the PCM the device returned), join() is the ordered join, and the case helpers build the float rows
that put a chosen int16 pattern into a sink's PCM — with alpha = 1 and gain = 1 the sink's chain gives pcm = rint(x)."""
import numpy as np

RUNS = np.dtype([("count", "<u8"), ("lead", "<u8"), ("trail", "<u8"), ("longest", "<u8")])
DTYPE = np.dtype([("n", "<u8"), ("sum_l", "<i8"), ("sum_r", "<i8"), ("sq_l", "<u8"), ("sq_r", "<u8"), ("cross", "<i8"), ("peak_l", "<u4"),
                  ("peak_r", "<u4"), ("clip_l", "<u8"), ("clip_r", "<u8"), ("quiet_l", RUNS), ("quiet_r", RUNS), ("quiet_both", RUNS),
                  ("reserved", "<u8", (3,))])
PREDICATES = ("quiet_l", "quiet_r", "quiet_both")


def runs(q):
    """(count, lead, trail, longest) of a boolean sequence, from run boundaries"""
    q = np.asarray(q, dtype=bool)
    if q.size == 0:
        return 0, 0, 0, 0
    edge = np.diff(np.concatenate([[0], q.astype(np.int8), [0]]))
    start, stop = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)       # run k spans start[k] .. stop[k] - 1
    if start.size == 0:
        return 0, 0, 0, 0
    length = stop - start
    return int(q.sum()), int(length[0]) if start[0] == 0 else 0, int(length[-1]) if stop[-1] == q.size else 0, int(length.max())


def record(pcm, quiet_lsb):
    """one row of interleaved int16 PCM -> a DTYPE scalar array (shape ())"""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and pcm.size % 2 == 0, (pcm.dtype, pcm.shape)
    L, R = pcm[0::2].astype(np.int64), pcm[1::2].astype(np.int64)
    out = np.zeros((), DTYPE)
    out["n"] = L.size
    out["sum_l"], out["sum_r"] = L.sum(), R.sum()
    out["sq_l"], out["sq_r"], out["cross"] = (L * L).sum(), (R * R).sum(), (L * R).sum()
    out["peak_l"], out["peak_r"] = (np.abs(L).max(), np.abs(R).max()) if L.size else (0, 0)
    out["clip_l"], out["clip_r"] = ((L == -32768) | (L == 32767)).sum(), ((R == -32768) | (R == 32767)).sum()
    ql, qr = np.abs(L) <= quiet_lsb, np.abs(R) <= quiet_lsb
    for name, q in zip(PREDICATES, (ql, qr, ql & qr)):
        out[name] = runs(q)
    return out


def records(pcm_rows, quiet_lsb):
    """[streams, 2n] int16 -> DTYPE [streams]"""
    pcm_rows = np.atleast_2d(pcm_rows)
    return np.array([record(row, quiet_lsb) for row in pcm_rows], dtype=DTYPE)


def join(a, b):
    """a then b, per include/sdrfm.h, on DTYPE scalars in Python integers"""
    out = np.zeros((), DTYPE)
    an, bn = int(a["n"]), int(b["n"])
    out["n"] = an + bn
    for f in ("sum_l", "sum_r", "sq_l", "sq_r", "cross", "clip_l", "clip_r"):
        out[f] = int(a[f]) + int(b[f])
    for f in ("peak_l", "peak_r"):
        out[f] = max(int(a[f]), int(b[f]))
    for p in PREDICATES:
        x, y = a[p], b[p]
        lead = int(x["lead"]) + (int(y["lead"]) if int(x["lead"]) == an else 0)
        trail = int(y["trail"]) + (int(x["trail"]) if int(y["trail"]) == bn else 0)
        out[p] = (int(x["count"]) + int(y["count"]), lead, trail, max(int(x["longest"]), int(y["longest"]), int(x["trail"]) + int(y["lead"])))
    return out


def same(a, b):
    """integer equality of every field"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 192 and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff(a, b):
    """the fields that differ, for a failing assertion's message"""
    a, b = np.atleast_1d(np.asarray(a)).view(DTYPE), np.atleast_1d(np.asarray(b)).view(DTYPE)
    out = []
    for s in range(min(a.size, b.size)):
        for f in DTYPE.names:
            if a[s][f].tobytes() != b[s][f].tobytes():
                out.append((s, f, a[s][f].tolist(), b[s][f].tolist()))
    return out[:8]


# ---- the case generator: int16 patterns as float rows ---------------------------------------------------------------------------------------------------
ALPHA, GAIN = 1.0, 1.0      # the sink's chain is then y = x, pcm = rint(x): integer-valued rows come out as themselves


def rows_of(L, R):
    """integer arrays (any shape, values in -32768 .. 32767) -> the float32 L and R rows that carry them"""
    L, R = np.asarray(L), np.asarray(R)
    assert L.shape == R.shape and L.min() >= -32768 and L.max() <= 32767 and R.min() >= -32768 and R.max() <= 32767
    return np.ascontiguousarray(L, dtype=np.float32), np.ascontiguousarray(R, dtype=np.float32)


def interleave(L, R):
    """the int16 PCM the rows of rows_of(L, R) are meant to give: [..., 2n]"""
    L, R = np.asarray(L), np.asarray(R)
    out = np.empty(L.shape[:-1] + (2 * L.shape[-1],), np.int16)
    out[..., 0::2], out[..., 1::2] = L, R
    return out


def random_full_range(rng, streams, n):
    """random rows over the whole int16 range with stretches of zeros, of small values and of rails mixed in"""
    L, R = rng.integers(-32768, 32768, (streams, n)), rng.integers(-32768, 32768, (streams, n))
    for ch in (L, R):
        for s in range(streams):
            for _ in range(4):
                a, w = int(rng.integers(0, n)), int(rng.integers(1, 200))
                ch[s, a:a + w] = (0, 0, int(rng.integers(-3, 4)), -32768, 32767)[int(rng.integers(0, 5))]
    return L, R


def one_loud_pair(streams, n, loud=1000):
    """stream p is zero except one loud pair at p % n"""
    L = np.zeros((streams, n), np.int64)
    L[np.arange(streams), np.arange(streams) % n] = loud
    return L, -L


def one_quiet_pair(streams, n, loud=1000):
    """the complement: loud except one zero pair at p % n"""
    L = np.full((streams, n), loud, np.int64)
    L[np.arange(streams), np.arange(streams) % n] = 0
    return L, -L
