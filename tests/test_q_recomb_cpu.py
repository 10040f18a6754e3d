"""CPU tests of design Q's scale-free recombination (csrc/sdrfm_q.hip SDRFM_Q_SCALEFREE, csrc/qtaps.c sdrfm_q_seed), through the instruction model
of tests/test_q_tables.py: per block the window XOR 0x80 as i8, the sparse K-chunks against the three digit tables, exact i32 sums — then, in place
of y = fma(f32(S0 + 256 S1), q, fma(f32(S2), 65536 q, cst)), the S0 accumulator STARTED at the seed and

    Y = fma(f32(S2), 65536, f32(S0 + (S1 << 8)))          (= y / q: K3 takes the angle, which a positive common factor leaves alone)

at every T = 1 .. 64 of the three rates sdrfm_create offers design Q.  Held here:
  * q Y within 2e-4 of the oracle's y per component — the bound tests/test_q_tables.py holds the scaled form to — and the ANGLE of Y (Y itself, unscaled)
    within asin(|dy| / |y|), |dy| = sqrt(2) 2e-4, of the angle of the oracle's y: what that bound allows an angle, nothing wider;
  * the seed is sum(H) / 2 for an even tap sum and one of its two integer neighbours for an odd one (both parities occur in the sweep);
  * seed + S0 + (S1 << 8) stays inside i32 at full-scale bytes — all 0, all 255, 0 / 255 alternating per sample and per component — and so does every value
    the S0 accumulator passes through (|seed| + 128 sum|digit 0|).
"""
import ctypes as C

import numpy as np
import pytest

import q_tap_sets as qt
import test_q_tables as tq

SWEEP_BLOCKS = 40                                                          # blocks of 8 outputs per row: 320 outputs, the first 16 left out
Y_TOL = 2e-4                                                               # tests/test_q_tables.py's bound on |y - oracle's y| per component


def _seed(pkg, h, D):
    lib = pkg.load_library()
    h = np.ascontiguousarray(h, dtype=np.float32)
    s = C.c_int32()
    rc = lib.sdrfm_q_seed(h.ctypes.data, h.size, D, C.byref(s))
    return rc, int(s.value)


def _taps_from_tables(A, T, D):
    """H[k] read back from row 0 (I of output 0) of the dense tables: window sample w meets tap k = 9 D - 1 - w at window byte 2 w"""
    dense = tq._dense(A)
    H = np.zeros(T, dtype=np.int64)
    d01 = np.zeros((2, T), dtype=np.int64)
    for k in range(T):
        c, kb = divmod(2 * (9 * D - 1 - k), 128)
        digs = [int(dense[c, t, 0, kb]) for t in range(3)]
        H[k] = digs[0] + 256 * digs[1] + 65536 * digs[2]
        d01[:, k] = digs[:2]
    return H, d01


def _digit_sums(A, iq, D):
    """S[t][block][row 16] exact, for every block whose window lies inside the row (block 0: zeros)"""
    blkb = 16 * D
    nblk = iq.size // blkb
    x = (iq.astype(np.int16) - 128).astype(np.int64)
    dense = tq._dense(A)
    nsc = dense.shape[0]
    S = np.zeros((3, nblk, 16), dtype=np.int64)
    for j in range(1, nblk):
        win = np.zeros(128 * nsc, dtype=np.int64)
        win[:2 * blkb] = x[(j - 1) * blkb:(j + 1) * blkb]
        win[2 * blkb:] = -99                                               # (beyond the window: the kernel feeds whatever its registers hold — no tap there)
        for c in range(nsc):
            S[:, j] += dense[c] @ win[128 * c:128 * c + 128]
    return S


def _scale_free(S, seed):
    """Y per (block, row) as the kernel forms it, and the i32 values it passes through"""
    s01 = S[0] + seed + 256 * S[1]                                         # the S0 accumulator started at the seed; v_lshl_add_u32
    assert np.abs(s01).max() < 2 ** 31 and np.abs(S[0] + seed).max() < 2 ** 31
    f = s01.astype(np.float32)                                             # v_cvt_f32_i32
    return (S[2].astype(np.float32).astype(np.float64) * 65536.0 + f.astype(np.float64)).astype(np.float32)   # one fused multiply-add


@pytest.mark.parametrize("D", [10, 8, 16])
def test_scale_free_recombination_at_every_tap_count(pkg, oracle_mod, D):
    Da, fs = qt.RATES[D]
    rows = {"fm": pkg.make_iq(1, 8 * D * SWEEP_BLOCKS, mode="fm", fs=fs, first_id=5)[0],
            "random": pkg.make_iq(1, 8 * D * SWEEP_BLOCKS, mode="random", first_id=6)[0]}
    n2 = 16 * D * 4
    full = {"all 0": np.zeros(n2, np.uint8), "all 255": np.full(n2, 255, np.uint8),
            "0 / 255 per sample": np.tile(np.repeat(np.array([0, 255], np.uint8), 2), n2 // 4),
            "0 / 255 per component": np.tile(np.array([0, 255], np.uint8), n2 // 2)}
    parities, fails = set(), {}
    worst_y, worst_ang, worst_reach = 0.0, 0.0, 0
    for T in range(1, 65):
        h, g = qt.plain_taps(pkg, T, D)
        rc, A, q, cst, c0 = qt.q_build(pkg, h, D)
        rs, seed = _seed(pkg, h, D)
        assert rc == 0 and rs == 0, (T, rc, rs)
        H, d01 = _taps_from_tables(A, T, D)
        sumH = int(H.sum())
        parities.add(sumH & 1)
        bad = []
        if sumH % 2 == 0:
            if seed != sumH // 2:
                bad.append("even tap sum %d: seed %d" % (sumH, seed))
        else:
            if seed not in ((sumH - 1) // 2, (sumH + 1) // 2):
                bad.append("odd tap sum %d: seed %d" % (sumH, seed))
            # ... the one nearer to the scaled form's constant 0.5 sum(h) / q in tap units
            w = 0.5 * float(h.astype(np.float64).sum()) / float(q)
            if abs(seed - w) > abs((sumH - seed) - w) + 1e-6:
                bad.append("odd tap sum: seed %d is not the neighbour nearer to 0.5 sum(h) / q = %.3f" % (seed, w))
        # ---- the i32 bound, by the digits (every byte at |byte - 128| = 128) and at the full-scale rows
        reach0 = abs(seed) + 128 * int(np.abs(d01[0]).sum())
        reach = abs(seed) + 128 * int((np.abs(d01[0]) + 256 * np.abs(d01[1])).sum())
        worst_reach = max(worst_reach, reach)
        if not (reach0 < 2 ** 31 and reach < 2 ** 31):
            bad.append("seed + the largest S0 + (S1 << 8) = %d leaves i32" % reach)
        for name, iq in full.items():
            S = _digit_sums(A, iq, D)[:, 1:]
            v = S[0] + seed + 256 * S[1]
            if not (np.abs(v).max() < 2 ** 31 and np.abs(S[0] + seed).max() < 2 ** 31 and np.abs(v).max() <= reach):
                bad.append("%s: %d" % (name, int(np.abs(v).max())))
        # ---- q Y against the oracle's y, and the angle of Y against the angle of the oracle's y
        for mode, iq in rows.items():
            o = oracle_mod.Oracle(h, g, D, Da)
            o.process(iq)
            yo, _ = o.last_stage()
            Y = _scale_free(_digit_sums(A, iq, D), seed).reshape(-1, 2)[16:yo.shape[0]].astype(np.float64)
            yo = yo[16:].astype(np.float64)
            err = float(np.abs(Y * float(q) - yo).max())
            worst_y = max(worst_y, err)
            if not err <= Y_TOL:
                bad.append("%s: q Y %.3g off the oracle's y" % (mode, err))
            r = np.hypot(yo[:, 0], yo[:, 1])
            ok = r > 4.0 * np.sqrt(2.0) * Y_TOL                            # (an angle means something: every output of the carrier, nearly every one of the noise)
            assert ok.sum() >= 0.9 * ok.size, (T, mode, int(ok.sum()))
            da = np.angle(np.exp(1j * (np.arctan2(Y[:, 1], Y[:, 0]) - np.arctan2(yo[:, 1], yo[:, 0]))))
            lim = np.arcsin(np.sqrt(2.0) * Y_TOL / r[ok])
            worst_ang = max(worst_ang, float(np.max(np.abs(da[ok]) / lim)))
            if not np.all(np.abs(da[ok]) <= lim):
                bad.append("%s: the angle of Y is %.3g x its bound off the angle of the oracle's y" % (mode, float(np.max(np.abs(da[ok]) / lim))))
        if bad:
            fails[T] = bad
    print("D = %d: T = 1 .. 64: worst |q Y - oracle's y| %.3g; worst angle error %.3g of asin(sqrt(2) 2e-4 / |y|); largest |seed| + reach 2^%.2f; tap-sum parities met %s" % (
        D, worst_y, worst_ang, np.log2(max(worst_reach, 1)), sorted(parities)))
    assert not fails, fails
    assert parities == {0, 1}, parities                                     # odd and even tap sums both occur


def test_seed_refuses_what_the_tables_refuse(pkg):
    h, _ = pkg.default_config(64)
    assert _seed(pkg, h, 9)[0] != 0                                         # odd decimation
    assert _seed(pkg, np.zeros(8, np.float32), 10)[0] != 0                  # all-zero taps
    assert _seed(pkg, np.ones(91, np.float32), 10)[0] != 0                  # T > 9 D
    bad = h.copy(); bad[3] = np.inf
    assert _seed(pkg, bad, 10)[0] != 0
    # the largest table the builder serves (144 taps of one sign at D = 16: every H = SDRFM_Q_HMAX) stays inside i32
    rc, seed = _seed(pkg, np.ones(144, np.float32), 16)
    assert rc == 0 and abs(seed - 144 * qt.Q_HMAX // 2) <= 72           # (H = SDRFM_Q_HMAX or one below: q is rounded to fp32)
