"""Reference of the RDS baseband stages (include/sdrfm.h), evaluated on a discriminator output d (the oracle's, or the
device's own): fp32-faithful — an fmaf is a float64 product (exact for two float32) plus the accumulator, rounded once to float32;
products and quotients are rounded to float32 like the device's — with an exact64 restatement (the same stages in float64, no
rounding).  Every FIR is vectorised over m with a loop over k, oldest sample first."""
import numpy as np

from stereo_ref import _fmaf, _split, oracle_d  # noqa: F401  (oracle_d is re-exported for the tests)

f32 = np.float32


def rds_ref(d, b, g, pilot_min, rds_gain, Dr=25, exact64=False):
    """d[0 .. M) from the start of a stream -> dict(w complex [M // Dr], wr, wi, pw, on, pmin2, count)"""
    br, bi = _split(b)
    g = np.asarray(g, f32)
    P, Tr = br.size, g.size
    dl = (P - 1) // 2
    d = np.asarray(d, f32)
    M = d.size
    A = M // Dr
    if exact64:
        fma = lambda a, x, c: np.asarray(a, np.float64) * x + c
        rnd = lambda v: np.asarray(v, np.float64)
        d = d.astype(np.float64)
        gain = np.float64(f32(rds_gain))
    else:
        fma = _fmaf
        rnd = lambda v: np.asarray(v, f32)
        gain = f32(rds_gain)
    off = P - 1 + Tr
    dp = np.concatenate([np.zeros(off, d.dtype), d])               # d[m < 0] = 0
    m = np.arange(M)
    qr = rnd(np.zeros(M))
    qi = rnd(np.zeros(M))
    for k in range(P - 1, -1, -1):                                  # oldest first
        x = dp[off + m - k]
        qr = fma(br[k], x, qr)
        qi = fma(bi[k], x, qi)
    pmin2 = f32(pilot_min) * f32(pilot_min)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        qq = rnd(qi * qi)
        pw = fma(qr, qr, qq)
        on = pw >= pmin2
        u2r = rnd(fma(qr, qr, -qq) / pw)
        u2i = rnd(rnd(2.0 * rnd(qr * qi)) / pw)
        kr = fma(u2r, qr, -rnd(u2i * qi))
        ki = fma(u2r, qi, rnd(u2i * qr))
        kr = rnd(np.where(on, kr, 0.0))
        ki = rnd(np.where(on, ki, 0.0))
        dd = dp[off + m - dl]
        zr = rnd(rnd(kr * gain) * dd)
        zi = rnd(rnd(ki * gain) * dd)
    zrp = np.concatenate([np.zeros(Tr, zr.dtype), zr])
    zip_ = np.concatenate([np.zeros(Tr, zi.dtype), zi])
    nj = (np.arange(A) + 1) * Dr - 1
    wr = rnd(np.zeros(A))
    wi = rnd(np.zeros(A))
    for k in range(Tr - 1, -1, -1):
        wr = fma(g[k], zrp[Tr + nj - k], wr)
        wi = fma(g[k], zip_[Tr + nj - k], wi)
    w = (wr.astype(np.float64) + 1j * wi.astype(np.float64))
    return dict(w=w if exact64 else w.astype(np.complex64), wr=wr, wi=wi, pw=pw, on=on, pmin2=pmin2, count=int(on.sum()))


def station_samples(n_groups, fs=2.4e6):
    """samples that carry n_groups whole groups through every filter's delay (12 bits of margin: the delays come to 3 bits, 100 ppm of
    40 groups to half a bit)"""
    return int(np.ceil((104 * n_groups + 12) / 1187.5 * fs))


def check_blocks(groups_sent, got, n_groups, where=""):
    """The block criterion: the station sent groups_sent cyclically from t = 0, n_groups of them completely; `got` is what the decoder
    reported.  Two groups may be lost to the pilot filter's ramp-up and to acquisition, nothing else: the first reported group is the
    transmitted group 0, 1 or 2; from it on there is a report for every transmitted group, in order; every block of every transmitted
    group from the third on is reported ok with the right 16 bits; and no block anywhere is reported ok with wrong bits.
    Returns (index of the first reported group, blocks reported ok)."""
    cyc = len(groups_sent)
    fits = []
    for first in range(3):
        wrong = [(first + i, k) for i, g in enumerate(got) for k in range(4)
                 if g.ok_mask >> k & 1 and g.blocks[k] != groups_sent[(first + i) % cyc][k]]
        fits.append((len(wrong), first, wrong))
    n_wrong, first, wrong = min(fits)
    assert n_wrong == 0, (where, "blocks reported ok with wrong bits (group, block):", wrong[:8], [f[0] for f in fits])
    assert len(got) >= n_groups - first, (where, "groups reported", len(got), "first", first, "wanted", n_groups - first)
    bad = [(i, got[i - first].ok_mask) for i in range(2, n_groups) if got[i - first].ok_mask != 0xF]
    assert not bad, (where, "transmitted groups from the third on with a block not ok (group, ok_mask):", bad[:8])
    return first, sum(bin(g.ok_mask).count("1") for g in got)
