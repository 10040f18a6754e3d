"""CPU: the arithmetic of the stereo PCM sink's conditioned default form (k_pcm_stereo_sink_hicut_scan: hicut_scan_segments of
csrc/sdrfm_sink_hicut.h) restated in numpy (tools/pcm_hicut_scan_emulate.py), held to the host routine sdrfm_pcm_deemph_stereo_hicut_s16
(csrc/pcm_sink.c) on exactly the inputs, shapes, alphas and ramps tests/test_pcm_hicut_gpu.py gives the kernel: the sink's three existing caps
(tests/test_pcm_sink_gpu.py: at most 1 LSB; a share of differing outputs <= 1e-3 + 2 / size; states within 1e-6 max(|st|, 0.25)) hold by the
arithmetic alone, at the two broadcast alphas — the only ones at which the header claims them."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_hicut_scan_emulate")

SHAPES = [(1, 19), (3, 20), (63, 4864), (65, 4865), (2, 9729)]     # tests/test_pcm_sink_params_gpu.py's
GAIN = np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))


def _alpha(pkg, aname):
    return float(pkg.load_library().sdrfm_pcm_alpha(48000.0, float(aname[:-2]) * 1e-6))


def _figures(pkg, ns, n, alpha, lo, slew):
    """two calls of n samples, the states and the count carried, against the host routine over the whole rows: (worst LSB, share, cap of the
    share, worst relative state difference)"""
    left, right = emu.sink_inputs(ns, n)
    h0, ht = emu.hicut_ramps(ns, lo)
    a, sa = emu.hicut_scan_emulate(left[:, :n], right[:, :n], alpha, GAIN, h0, ht, slew, 0)
    b, sb = emu.hicut_scan_emulate(left[:, n:], right[:, n:], alpha, GAIN, h0, ht, slew, min(n, emu.J_MAX), sa)
    want, st = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, slew, 0)
    d = np.abs(np.concatenate([a, b], axis=1).astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d != 0).mean()), 1e-3 + 2.0 / d.size, float(np.max(np.abs(sb - st) / np.maximum(np.abs(st), 0.25)))


@pytest.mark.parametrize("lo,slew", emu.RAMPS, ids=["%d-slew%d" % r for r in emu.RAMPS])
@pytest.mark.parametrize("aname", ["50us", "75us"])
def test_scan_over_affine_maps_stays_inside_the_three_caps(pkg, aname, lo, slew):
    alpha = _alpha(pkg, aname)
    worst, fails = [0, 0.0, 0.0], []
    for ns, n in SHAPES:
        lsb, share, cap, rel = _figures(pkg, ns, n, alpha, lo, slew)
        print("%s, %d <-> 32768 at slew %d, %d x %d: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" % (aname, lo, slew, ns, n, lsb, share, cap, rel))
        worst = [max(worst[0], lsb), max(worst[1], share), max(worst[2], rel)]
        if not (lsb <= 1 and share <= cap and rel <= 1e-6):
            fails.append((ns, n, lsb, share, rel))
    print("%s, %d <-> 32768 at slew %d: worst PCM %d LSB, share %.3g, state %.3g relative" % (aname, lo, slew, worst[0], worst[1], worst[2]))
    assert not fails, fails


def test_a_flat_32768_is_the_plain_scan_within_the_caps_and_the_plain_host_routine(pkg):
    """h = 32768 throughout: alpha[q] == alpha, the decay walked per chunk in place of the plain scan's precomputed power"""
    alpha = _alpha(pkg, "75us")
    for ns, n in [(3, 20), (65, 4865)]:
        left, right = emu.sink_inputs(ns, n)
        one = np.full(ns, 32768)
        got, st = emu.hicut_scan_emulate(left, right, alpha, GAIN, one, one, 1, 0)
        want = np.zeros_like(got)
        want_st = np.zeros((ns, 2), np.float32)
        for s in range(ns):
            want[s], want_st[s] = pkg.pcm_deemph_stereo_s16_host(left[s], right[s], alpha, float(GAIN))
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1 and (d != 0).mean() <= 1e-3 + 2.0 / d.size
        assert np.all(np.abs(st - want_st) <= 1e-6 * np.maximum(np.abs(want_st), 0.25))


def test_the_emulators_ramp_is_the_references(pkg):
    import hicut_ref as hr
    for (h0, ht), slew, J in [((1024, 32768), 7, 0), ((32768, 2048), 40, 4865), ((8192, 8192), 1, 3), ((32768, 1024), 1, 65530), ((1024, 32768), 32768, 0)]:
        got = emu.ramp_values([h0], [ht], slew, J, 900)[0]
        assert np.array_equal(got, hr.ramp_samples(h0, ht, slew, J, 900)), (h0, ht, slew, J)
    assert np.array_equal(emu.coefficients(0.25, np.array([[1024, 32768]])).view(np.uint32), hr.alphas(0.25, np.array([[1024, 32768]])).view(np.uint32))


def test_the_channels_share_the_coefficient_and_nothing_else(pkg):
    alpha = _alpha(pkg, "50us")
    left, right = emu.sink_inputs(3, 700)
    h0, ht = emu.hicut_ramps(3, 2048)
    a, sa = emu.hicut_scan_emulate(left, right, alpha, GAIN, h0, ht, 7, 0)
    b, sb = emu.hicut_scan_emulate(right, left, alpha, GAIN, h0, ht, 7, 0)
    assert np.array_equal(a[:, 0::2], b[:, 1::2]) and np.array_equal(a[:, 1::2], b[:, 0::2]) and np.array_equal(sa, sb[:, ::-1])
    c, _ = emu.hicut_scan_emulate(left, right, alpha, GAIN, h0, ht, 7, 1)                      # one sample later in the ramp: other bits
    assert not np.array_equal(a, c)
