"""Reference of the stereo stages (include/sdrfm.h), evaluated on the oracle's discriminator output.

d comes from the scalar-C oracle with a one-tap unit audio filter at Da = 1 (its audio is then d exactly).  The stages behind it are
fp32-faithful: an fmaf is a float64 product (exact for two float32) plus the accumulator, rounded once to float32; products and
quotients are rounded to float32 like the device's.  Every FIR is vectorised over m with a loop over k, oldest sample first.
"""
import numpy as np

f32 = np.float32


def _fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def oracle_d(oracle_mod, h, iq, D=10):
    """the definition's d[0 .. M) of one stream (all of iq in one call)"""
    return oracle_mod.Oracle(h, np.ones(1, f32), D, 1).process(iq).astype(f32)


def _split(b):
    b = np.asarray(b)
    if np.iscomplexobj(b):
        return b.real.astype(f32), b.imag.astype(f32)
    b = np.asarray(b, f32).reshape(-1)
    return b[0::2].copy(), b[1::2].copy()


def stereo_ref(d, b, g, pilot_min, diff_gain, Da=5, exact64=False):
    """d[0 .. M) from the start of a stream -> dict(L, R, am, as_, pw, on, pmin2, count); L, R hold the A = M // Da outputs.
    exact64: the same stages in float64 without any rounding (the restatement the fp32-faithful form is checked against)."""
    br, bi = _split(b)
    g = np.asarray(g, f32)
    P, Ta = br.size, g.size
    dl = (P - 1) // 2
    d = np.asarray(d, f32)
    M = d.size
    A = M // Da
    if exact64:
        fma = lambda a, x, c: np.asarray(a, np.float64) * x + c
        rnd = lambda v: np.asarray(v, np.float64)
        d = d.astype(np.float64)
    else:
        fma = _fmaf
        rnd = lambda v: np.asarray(v, f32)
    dp = np.concatenate([np.zeros(P - 1 + Ta, d.dtype), d])        # d[m < 0] = 0
    off = P - 1 + Ta
    m = np.arange(M)
    qr = rnd(np.zeros(M))
    qi = rnd(np.zeros(M))
    for k in range(P - 1, -1, -1):                                  # oldest first
        x = dp[off + m - k]
        qr = fma(br[k], x, qr)
        qi = fma(bi[k], x, qi)
    pmin2 = f32(pilot_min) * f32(pilot_min)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pw = fma(qr, qr, rnd(qi * qi))
        on = pw >= pmin2
        c = np.where(on, rnd(rnd(-2.0 * rnd(qr * qi)) / pw), 0.0)
        c = rnd(c)
    s = rnd(rnd(c * (np.float64(diff_gain) if exact64 else f32(diff_gain))) * dp[off + m - dl])
    sp = np.concatenate([np.zeros(Ta, s.dtype), s])
    j = np.arange(A)
    nj = (j + 1) * Da - 1
    am = rnd(np.zeros(A))
    as_ = rnd(np.zeros(A))
    for k in range(Ta - 1, -1, -1):
        am = fma(g[k], dp[off + nj - k - dl], am)
        as_ = fma(g[k], sp[Ta + nj - k], as_)
    return dict(L=rnd(am + as_), R=rnd(am - as_), am=am, as_=as_, pw=pw, on=on, pmin2=pmin2, count=int(on.sum()))


def tone_amplitudes(x, freqs, fs=48e3, skip=600):
    """least-squares amplitudes of the given tones (plus a DC term) in x[skip:]"""
    x = np.asarray(x, np.float64)[skip:]
    t = np.arange(x.size) / fs
    cols = [np.ones_like(t)]
    for f in freqs:
        cols += [np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)]
    coef, *_ = np.linalg.lstsq(np.stack(cols, 1), x, rcond=None)
    return [float(np.hypot(coef[1 + 2 * i], coef[2 + 2 * i])) for i in range(len(freqs))]


def separation_db(L, R, fl=1e3, fr=3.1e3, fs=48e3):
    """(separation in L, separation in R) in dB for an L-only tone at fl and an R-only tone at fr, and the four amplitudes"""
    l_l, l_r = tone_amplitudes(L, (fl, fr), fs)
    r_l, r_r = tone_amplitudes(R, (fl, fr), fs)
    return 20 * np.log10(l_l / l_r), 20 * np.log10(r_r / r_l), (l_l, l_r, r_l, r_r)
