#!/usr/bin/env python3
"""tools/pcm_hicut_scan_emulate.py — (CPU) the arithmetic of the stereo PCM sink's CONDITIONED default form (k_pcm_stereo_sink_hicut_scan,
csrc/sdrfm_sink_stereo.hip; the scan itself: hicut_scan_segments, csrc/sdrfm_sink_hicut.h) restated in numpy with the kernel's operation
order: segments of 256 chunks of 19 samples; per chunk its own contribution from state 0 (lane 0: from the carried state) and, beside it,
its own decay a = fma(alpha[q], -a, a) from 1; six doubling steps within each wave of 64 lanes on the pairs, s = fma(A, s_o, s) and then
A = A A_o; the four waves' totals combined in order, cw = fma(A_w, cw, s_w); every chunk re-walked from its true carry-in
fma(A_prev, cw, s_prev) with the exact chain's operations.  alpha[q] = alpha * (h 2^-15) with h the ramp of csrc/sdrfm_audio_ctl.h in
integers.  fp32 throughout (fused multiply-adds as in tools/pcm_chain_emulate.py).  tests/test_pcm_hicut_scan_cpu.py holds it to the host
routine sdrfm_pcm_deemph_stereo_hicut_s16 on the inputs, shapes, alphas and ramps of tests/test_pcm_hicut_gpu.py, which hicut_ramps() and
RAMPS below make for both.  Test infrastructure: nothing here is on a product path."""
import numpy as np

from pcm_chain_emulate import F, fma, pcm_word
from pcm_stereo_scan_emulate import C, NT, SEG, _shift_up, sink_inputs

ONE, J_MAX = 32768, 65536
# the ramps of the default form's tests: (the low end, the slew) — between 1024 or 2048 and 32768, slow, faster, ended inside a call, a jump
RAMPS = [(lo, slew) for lo in (1024, 2048) for slew in (1, 7, 40, 32768)]


def hicut_ramps(ns, lo):
    """(h0, ht) int64 [ns]: even streams run from lo up to 32768, odd streams the opposite way"""
    odd = np.arange(ns) % 2 == 1
    return np.where(odd, ONE, lo).astype(np.int64), np.where(odd, lo, ONE).astype(np.int64)


def ramp_values(h0, ht, slew, J, n):
    """int64 [ns, n]: audio_ctl_ramp(h0, ht, slew, audio_ctl_advance(J, i + 1)) for i < n, per stream"""
    h0, ht = np.asarray(h0, np.int64)[:, None], np.asarray(ht, np.int64)[:, None]
    run = np.minimum(min(int(J), J_MAX) + np.arange(1, n + 1, dtype=np.int64), J_MAX)[None, :] * int(slew)
    move = np.minimum(run, np.abs(ht - h0))
    return np.where(ht >= h0, h0 + move, h0 - move)


def coefficients(alpha, h):
    return (F(alpha) * (h.astype(F) * F(2.0 ** -15))).astype(F)


def scan_segment(x, al, y0, gain):
    """One segment: x [ns, 2, m] (m <= SEG), al [ns, m] the samples' coefficients, y0 [ns, 2] -> (PCM values int32 [ns, 2, m], the states
    behind the last sample [ns, 2])."""
    ns, m = x.shape[0], x.shape[-1]
    assert 0 < m <= SEG
    xp = np.zeros((ns, 2, SEG), F)
    xp[..., :m] = x
    xr = xp.reshape(ns, 2, NT, C)
    ap = np.zeros((ns, SEG), F)
    ap[:, :m] = al
    ar = ap.reshape(ns, 1, NT, C)                                  # shared by both channels
    t = np.arange(NT)
    i0 = np.minimum(t * C, m)
    cnt = np.minimum(m - i0, C)
    wl, wv = t & 63, t >> 6
    y0 = np.asarray(y0, F)
    # 1. the chunk's own contribution and its decay
    y = np.zeros((ns, 2, NT), F)
    y[..., 0] = y0
    A = np.ones((ns, 1, NT), F)
    for q in range(C):
        yn = fma(ar[..., q], (xr[..., q] - y).astype(F), y)
        An = fma(ar[..., q], -A, A)
        y = np.where(q < cnt, yn, y).astype(F)
        A = np.where(q < cnt, An, A).astype(F)
    # 2. the prefix over the pairs
    sv = y
    d = 1
    while d < 64:
        Ao = _shift_up(A, d)
        sn = fma(A, _shift_up(sv, d), sv)
        sv = np.where(wl >= d, sn, sv).astype(F)
        A = np.where(wl >= d, (A * Ao).astype(F), A).astype(F)
        d <<= 1
    sc = sv.reshape(ns, 2, 4, 64)[..., 63]                         # the waves' totals [ns, 2, 4]
    Aw = A.reshape(ns, 1, 4, 64)[..., 63]                          # [ns, 1, 4]
    prev, Aprev = _shift_up(sv, 1), _shift_up(A, 1)
    cw1 = sc[..., 0]
    cw2 = fma(Aw[..., 1], cw1, sc[..., 1])
    cw3 = fma(Aw[..., 2], cw2, sc[..., 2])
    cw = np.stack([np.zeros_like(cw1), cw1, cw2, cw3], axis=-1)[..., wv]
    # 3. the exact chain from the true carry-in
    first = np.where(wv == 0, y0[..., None], cw)
    y = np.where(wl == 0, first, fma(Aprev, cw, prev)).astype(F)
    out = np.zeros((ns, 2, NT, C), np.int32)
    for q in range(C):
        yn = fma(ar[..., q], (xr[..., q] - y).astype(F), y)
        out[..., q] = pcm_word((yn * gain).astype(F))
        y = np.where(q < cnt, yn, y).astype(F)
    return out.reshape(ns, 2, SEG)[..., :m], y[..., (m - 1) // C]


def hicut_scan_emulate(left, right, alpha, gain, h0, ht, slew, J=0, state=None):
    """left, right [ns, n]; h0, ht [ns] -> (pcm int16 [ns, 2n] interleaved L, R; state float32 [ns, 2]) by the blocked scan over affine maps,
    from state [ns, 2] (None: zeros), the ramps J samples old."""
    gain = F(gain)
    x = np.stack([np.asarray(left, F), np.asarray(right, F)], axis=1)          # [ns, 2, n]
    ns, n = x.shape[0], x.shape[2]
    al = coefficients(alpha, ramp_values(h0, ht, slew, J, n))
    y = np.zeros((ns, 2), F) if state is None else np.array(state, F).reshape(ns, 2)
    vals = np.zeros((ns, 2, n), np.int32)
    for base in range(0, n, SEG):
        vals[..., base:base + SEG], y = scan_segment(x[..., base:base + SEG], al[:, base:base + SEG], y, gain)
    pcm = np.zeros((ns, 2 * n), np.int16)
    pcm[:, 0::2], pcm[:, 1::2] = vals[:, 0], vals[:, 1]
    return pcm, y


def host_reference(pkg, left, right, alpha, gain, h0, ht, slew, J=0, state=None):
    """sdrfm_pcm_deemph_stereo_hicut_s16 per stream over the whole rows: (pcm int16 [ns, 2n], state float32 [ns, 2])"""
    ns = left.shape[0]
    pcm = np.zeros((ns, 2 * left.shape[1]), np.int16)
    st = np.zeros((ns, 2), np.float32)
    for s in range(ns):
        pcm[s], st[s] = pkg.pcm_deemph_stereo_hicut_s16_host(left[s], right[s], alpha, gain, int(h0[s]), int(ht[s]), slew, J,
                                                             (0.0, 0.0) if state is None else (float(state[s][0]), float(state[s][1])))
    return pcm, st


def main():
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    gain = F(32767.0 / (2 * np.pi * 75e3 / 240e3))
    for tau in (50e-6, 75e-6):
        alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, tau))
        for ns, n in ((3, 20), (65, 4865), (2, 9729)):
            left, right = sink_inputs(ns, n)
            for lo, slew in RAMPS:
                h0, ht = hicut_ramps(ns, lo)
                a, sa = hicut_scan_emulate(left[:, :n], right[:, :n], alpha, gain, h0, ht, slew, 0)
                b, sb = hicut_scan_emulate(left[:, n:], right[:, n:], alpha, gain, h0, ht, slew, min(n, J_MAX), sa)
                want, st = host_reference(pkg, left, right, alpha, gain, h0, ht, slew, 0)
                dd = np.abs(np.concatenate([a, b], axis=1).astype(np.int32) - want.astype(np.int32))
                print("%g us, %d x 2 x %d, %d <-> 32768 at slew %d: max |PCM difference| %d LSB, share %.3g, state %.3e relative"
                      % (tau * 1e6, ns, n, lo, slew, dd.max(), float((dd > 0).mean()), float(np.max(np.abs(sb - st) / np.maximum(np.abs(st), 0.25)))))


if __name__ == "__main__":
    main()
