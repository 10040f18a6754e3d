#!/usr/bin/env python3
"""tools/pcm_stereo_scan_emulate.py — (CPU) the arithmetic of the stereo PCM sink's default form (k_pcm_stereo_sink_scan, csrc/sdrfm_sink_stereo.hip; the scan itself: sink_scan_segments, csrc/sdrfm_sink_kernels.h)
restated in numpy with the kernel's operation order, for both channels side by side: segments of 256 chunks of 19 samples, the chunk's own contribution
from state 0 (lane 0: from the carried state), six doubling steps within each wave of 64 lanes with the powers squared on the way, the four waves' totals
combined, every chunk re-walked from its true carry-in with the exact chain's operations.  fp32 throughout (fused multiply-adds as in
tools/pcm_chain_emulate.py: through float64, exact products, one rounding that differs from a true fma's in ~1e-9 of the cases).
tests/test_pcm_stereo_scan_cpu.py holds it to the host routine sdrfm_pcm_deemph_stereo_s16 on the inputs of tests/test_pcm_stereo_sink_gpu.py, which
sink_inputs() below makes for both.  mono_scan_emulate() is the mono sink's default form (k_pcm_sink_scan, csrc/sdrfm_sink.hip): the same scan over one
chain, as in the kernels, which instantiate one body for one channel and for two, held to sdrfm_pcm_deemph_s16 by tests/test_pcm_mono_scan_cpu.py.  Test infrastructure: nothing here is on a product path."""
import numpy as np

from pcm_chain_emulate import F, fma, pcm_word

NT, C = 256, 19
SEG = NT * C


def sink_inputs(ns, n):
    """(L, R) float32 [ns, 2n]: two calls of n samples per stream; independent draws, row 0 starting with values that saturate both channels."""
    rng = np.random.default_rng(ns * 77 + n)
    left = (rng.standard_normal((ns, 2 * n)) * 1.5).astype(F)
    right = (rng.standard_normal((ns, 2 * n)) * 1.5).astype(F)
    head = np.array([9.0, -9.0, 0.0, 1e-30, 0.5, -0.5], F)[: min(6, 2 * n)]
    left[0, : head.size] = head
    right[0, : head.size] = -head
    return left, right


def _shift_up(v, d):
    """__shfl_up by d within waves of 64 lanes (last axis: 256 lanes); lanes below d keep their own value"""
    w = v.reshape(v.shape[:-1] + (4, 64))
    o = w.copy()
    o[..., d:] = w[..., :-d]
    return o.reshape(v.shape)


def scan_segment(x, y0, alpha, gain, pc):
    """One segment: x [..., m] (m <= SEG), y0 [...] -> (PCM values int32 [..., m], the states behind the last sample [...]).  The leading axes are
    independent chains (streams, channels): the kernel walks a stream's two in one lane."""
    lead, m = x.shape[:-1], x.shape[-1]
    assert 0 < m <= SEG
    xp = np.zeros(lead + (SEG,), F)
    xp[..., :m] = x
    xr = xp.reshape(lead + (NT, C))
    t = np.arange(NT)
    i0 = np.minimum(t * C, m)
    cnt = np.minimum(m - i0, C)
    wl, wv = t & 63, t >> 6
    y0 = np.asarray(y0, F)
    # 1. the chunk's own contribution
    y = np.zeros(lead + (NT,), F)
    y[..., 0] = y0
    for q in range(C):
        yn = fma(alpha, (xr[..., q] - y).astype(F), y)
        y = np.where(q < cnt, yn, y).astype(F)
    # 2. the carries
    sv, pw = y, F(pc)
    d = 1
    while d < 64:
        sn = fma(pw, _shift_up(sv, d), sv)
        sv = np.where(wl >= d, sn, sv).astype(F)
        pw = F(pw * pw)
        d <<= 1
    sc = sv.reshape(lead + (4, 64))[..., 63]                       # the waves' totals
    pl, pb = np.ones(NT, F), F(pc)
    for bit in range(6):
        pl = np.where((wl >> bit) & 1, (pl * pb).astype(F), pl).astype(F)
        pb = F(pb * pb)
    prev = _shift_up(sv, 1)
    cw1 = sc[..., 0]
    cw2 = fma(pw, cw1, sc[..., 1])
    cw3 = fma(pw, cw2, sc[..., 2])
    cw = np.stack([np.zeros_like(cw1), cw1, cw2, cw3], axis=-1)[..., wv]
    # 3. the exact chain from the true carry-in
    first = np.where(wv == 0, y0[..., None], cw)
    y = np.where(wl == 0, first, fma(pl, cw, prev)).astype(F)
    out = np.zeros(lead + (NT, C), np.int32)
    for q in range(C):
        yn = fma(alpha, (xr[..., q] - y).astype(F), y)
        out[..., q] = pcm_word((yn * gain).astype(F))
        y = np.where(q < cnt, yn, y).astype(F)
    return out.reshape(lead + (SEG,))[..., :m], y[..., (m - 1) // C]


def stereo_scan_emulate(left, right, alpha, gain, state=None):
    """left, right [ns, n] -> (pcm int16 [ns, 2n] interleaved L, R; state float32 [ns, 2]) by the blocked scan, from state [ns, 2] (None: zeros)."""
    alpha, gain = F(alpha), F(gain)
    pc = F((1.0 - float(alpha)) ** C)
    x = np.stack([np.asarray(left, F), np.asarray(right, F)], axis=1)          # [ns, 2, n]
    ns, n = x.shape[0], x.shape[2]
    y = np.zeros((ns, 2), F) if state is None else np.array(state, F).reshape(ns, 2)
    vals = np.zeros((ns, 2, n), np.int32)
    for base in range(0, n, SEG):
        vals[..., base:base + SEG], y = scan_segment(x[..., base:base + SEG], y, alpha, gain, pc)
    pcm = np.zeros((ns, 2 * n), np.int16)
    pcm[:, 0::2], pcm[:, 1::2] = vals[:, 0], vals[:, 1]
    return pcm, y


def mono_inputs(ns, n):
    """x float32 [ns, 2n]: the mono sink's analogue of sink_inputs (two calls of n samples per stream, row 0 starting with values that saturate)"""
    rng = np.random.default_rng(ns * 79 + n)
    x = (rng.standard_normal((ns, 2 * n)) * 1.5).astype(F)
    head = np.array([9.0, -9.0, 0.0, 1e-30, 0.5, -0.5], F)[: min(6, 2 * n)]
    x[0, : head.size] = head
    return x


def mono_scan_emulate(x, alpha, gain, state=None):
    """x [ns, n] -> (pcm int16 [ns, 2n], L = R; state float32 [ns]) by the mono sink's default form (k_pcm_sink_scan, csrc/sdrfm_sink.hip): the same segments,
    chunks and operations as one channel of the stereo scan, from state [ns] (None: zeros)."""
    alpha, gain = F(alpha), F(gain)
    pc = F((1.0 - float(alpha)) ** C)
    x = np.asarray(x, F)
    ns, n = x.shape
    y = np.zeros(ns, F) if state is None else np.array(state, F).reshape(ns)
    vals = np.zeros((ns, n), np.int32)
    for base in range(0, n, SEG):
        vals[:, base:base + SEG], y = scan_segment(x[:, base:base + SEG], y, alpha, gain, pc)
    return np.repeat(vals.astype(np.int16), 2, axis=1), y


def mono_host_reference(pkg, x, alpha, gain):
    """sdrfm_pcm_deemph_s16 per stream over the whole rows: (pcm int16 [ns, 2n], state float32 [ns])"""
    pcm = np.zeros((x.shape[0], 2 * x.shape[1]), np.int16)
    st = np.zeros(x.shape[0], np.float32)
    for s in range(x.shape[0]):
        pcm[s], st[s] = pkg.pcm_deemph_s16_host(x[s], alpha, gain)
    return pcm, st


def host_reference(pkg, left, right, alpha, gain):
    """sdrfm_pcm_deemph_stereo_s16 per stream over the whole rows: (pcm int16 [ns, 2n], state float32 [ns, 2])"""
    ns = left.shape[0]
    pcm = np.zeros((ns, 2 * left.shape[1]), np.int16)
    st = np.zeros((ns, 2), np.float32)
    for s in range(ns):
        pcm[s], st[s] = pkg.pcm_deemph_stereo_s16_host(left[s], right[s], alpha, gain)
    return pcm, st


def main():
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    gain = F(32767.0 / (2 * np.pi * 75e3 / 240e3))
    for ns, n in ((5, 255), (65, 1300), (2, 30000)):
        left, right = sink_inputs(ns, n)
        a, sa = stereo_scan_emulate(left[:, :n], right[:, :n], alpha, gain)
        b, sb = stereo_scan_emulate(left[:, n:], right[:, n:], alpha, gain, sa)
        want, st = host_reference(pkg, left, right, alpha, gain)
        dd = np.abs(np.concatenate([a, b], axis=1).astype(np.int32) - want.astype(np.int32))
        print("%d x 2 x %d: max |PCM difference| %d LSB, %.4f %% of the outputs differ, state %.3e relative"
              % (ns, n, dd.max(), 100.0 * (dd > 0).mean(), float(np.max(np.abs(sb - st) / np.maximum(np.abs(st), 0.25)))))


if __name__ == "__main__":
    main()
