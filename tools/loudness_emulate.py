#!/usr/bin/env python3
"""tools/loudness_emulate.py — (CPU) the arithmetic of the stereo PCM sink's loudness kernel (csrc/sdrfm_loudness.h) restated in
numpy with the kernel's order of operations: the same chunk length L = 19, the same tile of 256 x 19 pairs, the same matrix powers A^(L 2^i)
built the same way (in long double: the transition taken into the scan's balanced coordinates (z0, z1, z2, kappa (z2 + z3)), its L-th
power by L - 1 products from the left, then repeated squaring, rounded to double), pass 1 from zero state (lane 0 from the carried state), the
Hillis-Steele scan over lanes in those coordinates whose combine adds a row's four products left to right and then the row onto the lane's state, pass 2 from the
state the lane before leaves with two partial sums split at the sub-block boundary, and every sub-block summed from the carried energy and
then its lanes' pieces in lane order.  float64 throughout and no fused multiply-add, as the library is built (-ffp-contract=off).

The index arithmetic is restated too (chunk, split, block span, piece, ring slot); tests/native/loudness_check.cpp holds the header's own
functions to naive loops.  tests/test_loudness_emulate_cpu.py compares emulate() with the C routine sdrfm_pcm_loudness_s16 and so measures
the tolerance the device is held to.  Run as a script: prints that comparison for a random full-range row and a DC row.
Test infrastructure: nothing here is on a product path."""
import numpy as np

L, NT, STEPS = 19, 256, 8
TILE = L * NT
TABLE_DTYPE = np.longdouble          # the precision the table is built in (ld_matrix_powers: long double); a test sets float64 to show what that costs


def transition(c):
    """ld_transition: the zero-input step of both biquads in transposed direct form II, z = (shelf s1, shelf s2, high-pass s1, high-pass s2)"""
    A = np.zeros((4, 4))
    A[0, 0], A[0, 1] = -c[3], 1.0
    A[1, 0] = -c[4]
    A[2, 0], A[2, 2], A[2, 3] = c[6] - c[8] * c[5], -c[8], 1.0
    A[3, 0], A[3, 2] = c[7] - c[9] * c[5], -c[9]
    return A


def matmul(X, Y):
    """ld_matmul: a row's products added left to right"""
    out = np.zeros((4, 4), X.dtype)
    for r in range(4):
        for q in range(4):
            t = X[r, 0] * Y[0, q]
            for k in range(1, 4):
                t = t + X[r, k] * Y[k, q]
            out[r, q] = t
    return out


def balance(c):
    """ld_balance: kappa, the power of two nearest 1 / sqrt(1 + a1 + a2) of the high-pass, within 1 .. 2^20"""
    t, kappa = 1.0 + c[8] + c[9], 1.0
    for _ in range(20):
        if not 2.0 * kappa * kappa * t < 1.0:
            break
        kappa *= 2.0
    return kappa


def matrix_powers(c):
    """ld_matrix_powers: [STEPS, 4, 4], pw[i] = (T A T^-1)^(L 2^i) in long double, rounded to double at the end; T maps z to the scan's
    coordinates (z0, z1, z2, kappa (z2 + z3))"""
    kap = TABLE_DTYPE(balance(c))
    T = np.eye(4, dtype=TABLE_DTYPE)
    T[3, 2] = T[3, 3] = kap
    Ti = np.eye(4, dtype=TABLE_DTYPE)
    Ti[3, 2], Ti[3, 3] = -1.0, 1.0 / kap
    A = matmul(matmul(T, transition(c).astype(TABLE_DTYPE)), Ti)
    P = A.copy()
    for _ in range(1, L):
        P = matmul(A, P)
    pw = []
    for _ in range(STEPS):
        pw.append(P)
        P = matmul(P, P)
    return np.array(pw).astype(np.float64)


def kw_step(c, z, x):
    """ld_kw_step on arrays: z [..., 4] is updated in place, x [...] -> y2 [...]"""
    y1 = c[0] * x + z[..., 0]
    z[..., 0] = (c[1] * x - c[3] * y1) + z[..., 1]
    z[..., 1] = c[2] * x - c[4] * y1
    y2 = c[5] * y1 + z[..., 2]
    z[..., 2] = (c[6] * y1 - c[8] * y2) + z[..., 3]
    z[..., 3] = c[7] * y1 - c[9] * y2
    return y2


def matvec_add(M, q, p):
    """ld_matvec_add on arrays [..., 4]: p + M q"""
    out = np.empty_like(p)
    for r in range(4):
        t = M[r, 0] * q[..., 0]
        t = t + M[r, 1] * q[..., 1]
        t = t + M[r, 2] * q[..., 2]
        t = t + M[r, 3] * q[..., 3]
        out[..., r] = p[..., r] + t
    return out


def emulate(pcm, block_len, coef, pos=0, z=None, e=None, cap_blocks=None):
    """One call of the kernel on one stream: pcm int16 [2n] -> (blocks [(index, e_l, e_r)] of the sub-blocks the call completes AND stores,
    pos, z [2, 4], e [2]) from the state (pos, z, e).  cap_blocks: only the newest cap_blocks of all completed sub-blocks are stored."""
    c = np.asarray(coef, np.float64)
    pw = matrix_powers(c)
    kap = balance(c)
    x = np.stack([np.asarray(pcm[0::2], np.float64), np.asarray(pcm[1::2], np.float64)])       # [2, n]
    n = x.shape[1]
    cz = np.zeros((2, 4)) if z is None else np.array(z, np.float64)
    ce = np.zeros(2) if e is None else np.array(e, np.float64)
    off, blk = pos % block_len, pos // block_len
    total = (pos + n) // block_len
    keep_from = total - cap_blocks if cap_blocks is not None and total > cap_blocks else 0
    blocks = []
    lane = np.arange(NT)
    for t in range((n + TILE - 1) // TILE):
        m = min(TILE, n - t * TILE)
        nact = (m + L - 1) // L
        xt = np.zeros((2, TILE))
        xt[:, :m] = x[:, t * TILE:t * TILE + m]
        xt = xt.reshape(2, NT, L)
        ln = np.clip(m - lane * L, 0, L)                                                     # ld_chunk
        # pass 1: from zero state; lane 0 from the carried state
        zz = np.zeros((2, NT, 4))
        zz[:, 0] = cz
        for i in range(L):
            act = i < ln
            new = zz.copy()
            kw_step(c, new, xt[:, :, i])
            zz[:, act] = new[:, act]
        zz[..., 3] = kap * (zz[..., 2] + zz[..., 3])                                        # into the scan's coordinates
        # the scan
        s = 0
        while (1 << s) < nact:
            d = 1 << s
            upd = (lane >= d) & (lane < nact)
            q = np.roll(zz, d, axis=1)
            new = matvec_add(pw[s], q, zz)
            zz = np.where(upd[None, :, None], new, zz)
            s += 1
        # pass 2
        zz[..., 3] = zz[..., 3] / kap - zz[..., 2]                                          # and back
        st = np.roll(zz, 1, axis=1)
        st[:, 0] = cz
        split = np.minimum(ln, block_len - (off + lane * L) % block_len)                     # ld_split (inactive lanes: ln = 0)
        piece = np.zeros((2, 2, NT))                                                         # [part, channel, lane]
        for i in range(L):
            act = i < ln
            new = st.copy()
            y = kw_step(c, new, xt[:, :, i])
            st[:, act] = new[:, act]
            sq = y * y
            first = act & (i < split)
            second = act & ~(i < split)
            piece[0] = np.where(first[None, :], piece[0] + sq, piece[0])
            piece[1] = np.where(second[None, :], piece[1] + sq, piece[1])
        cz = st[:, nact - 1].copy()
        # one lane per sub-block and channel
        nb = (off + m) // block_len
        ce_next = None
        for k in range(nb + 1):
            bs = k * block_len - off                                                         # ld_block_span
            lo, hi = min(max(bs, 0), m), min(bs + block_len, m)
            acc = ce.copy() if k == 0 else np.zeros(2)
            if hi > lo:
                for j in range(lo // L, (hi - 1) // L + 1):
                    acc = acc + piece[0 if j * L >= bs else 1, :, j]                         # ld_piece
            if k < nb:
                if blk + k >= keep_from:
                    blocks.append((blk + k, acc[0], acc[1]))
            else:
                ce_next = acc
        ce = ce_next
        blk += nb
        off = (off + m) % block_len
    return blocks, pos + n, cz, ce


def emulate_rows(pcm_rows, block_len, coef):
    """[streams, 2n] int16 from zero state -> energies [streams, n_blocks, 2]"""
    out = []
    for row in np.atleast_2d(pcm_rows):
        b = emulate(row, block_len, coef)[0]
        out.append(np.array([[el, er] for _, el, er in b], np.float64).reshape(-1, 2))
    return np.stack(out)


def compare(got, want, block_len):
    """(worst |d| / want over sub-blocks with want > 0, worst |d| / block_len) of two energy arrays"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    rel = float((d[want > 0] / want[want > 0]).max()) if (want > 0).any() else 0.0
    return rel, float(d.max() / block_len) if d.size else 0.0


if __name__ == "__main__":
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    coef = pkg.loudness_default_coef()
    rng = np.random.default_rng(1)
    n = 2 * TILE + 17
    rows = {"random full range": rng.integers(-32768, 32768, 2 * n).astype(np.int16), "DC +32767": np.full(2 * n, 32767, np.int16)}
    for name, row in rows.items():
        for bl in (64, 4800):
            want, _ = pkg.pcm_loudness_host(row, bl, coef)
            rel, ab = compare(emulate_rows(row, bl, coef), want, bl)
            print("%-18s block_len %4d: worst relative %.3g, worst absolute %.3g LSB^2 per sample" % (name, bl, rel, ab))
