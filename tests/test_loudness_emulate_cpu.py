"""The tolerance the loudness kernel is held to, measured without a GPU: tools/loudness_emulate.py — the kernel's order of
operations in numpy: same L, same tile, same matrix powers — against the C routine sdrfm_pcm_loudness_s16 on the GPU tests' own inputs
(tests/loudness_cases.py).  The two terms of |e - e_host| <= RTOL e_host + ATOL block_len are measured separately and printed; RTOL and ATOL
are 8 x the recorded figures, and the hard conditions RTOL <= 1e-9 and ATOL <= 1e-3 LSB^2 per sample are asserted as such."""
import os
import sys

import numpy as np

import loudness_cases as lc

sys.path.insert(0, os.path.join(lc.ROOT, "tools"))
import loudness_emulate as em  # noqa: E402


def test_geometry_is_the_headers():
    assert (em.L, em.NT, em.TILE) == (lc.L, lc.NT, lc.TILE) and lc.L <= 64 and lc.TILE == lc.L * lc.NT


def _hard(pkg, coef, name, bl, s):
    """the calls of one hard row through both, call by call: the energies of all calls, and the two end states"""
    st, pos, z, e, got, want = None, 0, None, None, [], []
    for Li, Ri in lc.hard_rows()[name]:
        pcm = lc.interleave(Li, Ri)[s]
        w, st = pkg.pcm_loudness_host(pcm, bl, coef, state=st)
        b, pos, z, e = em.emulate(pcm, bl, coef, pos, z, e)
        assert [k for k, _, _ in b] == list(range(len(got), len(got) + w.shape[1]))          # block indices are exact
        got += [[el, er] for _, el, er in b]
        want += w[0].tolist()
    assert pos == int(st["pos"][0])
    return np.array(got).reshape(-1, 2), np.array(want).reshape(-1, 2)


def test_measured_tolerance_and_the_hard_caps(pkg):
    coef = pkg.loudness_default_coef()
    rel = ab = 0.0
    for n in lc.LENGTHS:
        pcm = lc.interleave(*lc.random_rows(n, 3))
        for bl in lc.BLOCK_LENS:
            want, st = pkg.pcm_loudness_host(pcm, bl, coef)
            got = em.emulate_rows(pcm, bl, coef)
            assert want.shape == (3, n // bl, 2) and (st["pos"] == n).all()
            ok, why = lc.within(got, want, bl)
            assert ok, (n, bl, why)
            r, a = lc.measure(got, want, bl)
            rel, ab = max(rel, r), max(ab, a)
    print("random rows: worst relative %.3g, worst absolute %.3g LSB^2 per sample" % (rel, ab))
    for name in lc.hard_rows():
        for bl in (64, 4800):
            for s in range(2):
                got, want = _hard(pkg, coef, name, bl, s)
                ok, why = lc.within(got, want, bl)
                assert ok, (name, bl, s, why)
                r, a = lc.measure(got, want, bl)
                rel, ab = max(rel, r), max(ab, a)
        print("%s: worst relative so far %.3g, worst absolute %.3g LSB^2 per sample" % (name, rel, ab))
    assert rel <= lc.MEASURED_REL and ab <= lc.MEASURED_ABS, (rel, ab)                       # the recorded figures stand
    assert rel >= lc.MEASURED_REL / 2 and ab >= lc.MEASURED_ABS / 2, (rel, ab)               # and are measurements, not guesses
    assert lc.RTOL == 8 * lc.MEASURED_REL and lc.ATOL == 8 * lc.MEASURED_ABS
    assert lc.RTOL <= 1e-9 and lc.ATOL <= 1e-3                                               # the hard conditions


def test_a_displaced_sample_is_far_outside_the_bound(pkg):
    """what the bound must not hide: one pair of a full-range row lost, doubled or moved to its neighbour"""
    coef = pkg.loudness_default_coef()
    rng = np.random.default_rng(9)
    Li, Ri = rng.integers(-32768, 32768, (1, 640)), rng.integers(-32768, 32768, (1, 640))
    assert Li[0, 300] != Li[0, 301] and Ri[0, 300] != Ri[0, 301]
    good = lc.interleave(Li, Ri)
    want, _ = pkg.pcm_loudness_host(good, 64, coef)
    for what in ("lost", "doubled", "swapped"):
        a, b = Li[0].copy(), Ri[0].copy()
        if what == "lost":
            a[300:-1], b[300:-1] = Li[0, 301:], Ri[0, 301:]
        elif what == "doubled":
            a[301:], b[301:] = Li[0, 300:-1], Ri[0, 300:-1]
        else:
            a[[300, 301]], b[[300, 301]] = a[[301, 300]], b[[301, 300]]
        got, _ = pkg.pcm_loudness_host(lc.interleave(a[None], b[None]), 64, coef)
        assert not lc.within(got, want, 64)[0], what


def test_carried_state_and_ring_rule(pkg):
    """the ragged sequence through the emulation with the state carried: the C routine call by call and on the concatenation; with
    cap_blocks = 4 a call that completes 75 sub-blocks stores exactly 71 .. 74"""
    coef = pkg.loudness_default_coef()
    total = sum(lc.SEQUENCE)
    pcm = lc.interleave(*lc.random_rows(total, 1))[0]
    whole, _ = pkg.pcm_loudness_host(pcm, 100, coef)
    st, pos, z, e, got, at = None, 0, None, None, [], 0
    for k in lc.SEQUENCE:
        piece = pcm[2 * at:2 * (at + k)]
        w, st = pkg.pcm_loudness_host(piece, 100, coef, state=st)
        b, pos, z, e = em.emulate(piece, 100, coef, pos, z, e)
        assert len(b) == w.shape[1] and pos == int(st["pos"][0])
        got += [[el, er] for _, el, er in b]
        at += k
    assert len(got) == total // 100
    ok, why = lc.within(np.array(got)[None], whole, 100)
    assert ok, why
    b = em.emulate(pcm[:9600], 64, coef, cap_blocks=4)[0]
    assert [k for k, _, _ in b] == [71, 72, 73, 74]
