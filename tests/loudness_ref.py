"""The loudness meter's definitions (include/sdrfm.h) restated independently of the library: energies() K-weights int16 stereo PCM
with scipy.signal.lfilter and sums y^2 per sub-block; gate_list() is BS.1770-4 / EBU Tech 3342 gating on plain lists — exact gates and exact
percentiles, no histogram — which the C gate's histogram is measured against."""
import numpy as np

# BS.1770-4, 48 kHz: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
K48 = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])


def kweight(x, coef=K48):
    from scipy.signal import lfilter
    y = lfilter(coef[0:3], np.concatenate([[1.0], coef[3:5]]), np.asarray(x, np.float64))
    return lfilter(coef[5:8], np.concatenate([[1.0], coef[8:10]]), y)


def energies(pcm_row, block_len, coef=K48):
    """int16 [2n] from zero state -> float64 [n // block_len, 2]"""
    pcm_row = np.asarray(pcm_row)
    assert pcm_row.dtype == np.int16 and pcm_row.ndim == 1 and pcm_row.size % 2 == 0
    nb = pcm_row.size // 2 // block_len
    out = np.zeros((nb, 2))
    for ch in range(2):
        y = kweight(pcm_row[ch::2], coef)[:nb * block_len]
        out[:, ch] = (y * y).reshape(nb, block_len).sum(axis=1)
    return out


def lufs(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def gate_list(e, block_len):
    """energies [n, 2] of consecutive sub-blocks -> dict(m, s, i, lra, n_gating, n_abs, n_rel) by the text of the recommendations"""
    z = np.asarray(e, np.float64).sum(axis=1) / (block_len * 32768.0 ** 2)
    out = dict(m=np.nan, s=np.nan, i=np.nan, lra=np.nan, n_gating=0, n_abs=0, n_rel=0)
    if z.size >= 4:
        g = np.array([z[k - 3:k + 1].mean() for k in range(3, z.size)])
        out["m"], out["n_gating"] = float(lufs(g[-1])), g.size
        a = g[lufs(g) > -70.0]
        out["n_abs"] = a.size
        out["i"] = -np.inf
        if a.size:
            r = a[lufs(a) > lufs(a.mean()) - 10.0]
            out["n_rel"] = r.size
            if r.size:
                out["i"] = float(lufs(r.mean()))
    if z.size >= 30:
        st = np.array([z[k - 29:k + 1].mean() for k in range(29, z.size)])
        out["s"] = float(lufs(st[-1]))
        a = st[lufs(st) > -70.0]
        if a.size:
            r = np.sort(lufs(a[lufs(a) > lufs(a.mean()) - 20.0]))
            if r.size:
                out["lra"] = float(r[int(np.floor((r.size - 1) * 0.95 + 0.5))] - r[int(np.floor((r.size - 1) * 0.10 + 0.5))])
    return out
