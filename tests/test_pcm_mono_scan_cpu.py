"""CPU: the arithmetic of the mono PCM sink's default form (k_pcm_sink_scan, csrc/sdrfm_sink.hip: sink_scan_segments<1> of csrc/sdrfm_sink_kernels.h; its LIST instance serves routed streams behind a mixed launch with
the same arithmetic) restated in numpy (mono_scan_emulate, tools/pcm_stereo_scan_emulate.py: one chain of the stereo scan), held to the host routine
sdrfm_pcm_deemph_s16 (csrc/pcm_sink.c) at the three caps of tests/test_pcm_sink_gpu.py: at the edges of a chunk and of a segment, at every alpha of
tests/pcm_params.py and at its gains, two calls with the state carried."""
import importlib
import os
import sys

import numpy as np
import pytest

import pcm_params as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_stereo_scan_emulate")

EDGE_SHAPES = [(2, 18), (1, 19), (3, 20), (5, 4863), (63, 4864), (65, 4865), (2, 9729)]


def _hold(pkg, ns, n, alpha, gain):
    x = emu.mono_inputs(ns, n)
    a, sa = emu.mono_scan_emulate(x[:, :n], alpha, gain)                                # two calls: the state is carried
    b, sb = emu.mono_scan_emulate(x[:, n:], alpha, gain, sa)
    got = np.concatenate([a, b], axis=1)
    want, st = emu.mono_host_reference(pkg, x, alpha, gain)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (int(d.max()), np.argwhere(d > 1)[:4])
    assert (d != 0).mean() <= 1e-3 + 2.0 / d.size, float((d != 0).mean())
    assert np.all(np.abs(sb - st) <= 1e-6 * np.maximum(np.abs(st), 0.25)), (sb, st)


def _alpha75(pkg):
    return pp.alpha_of(pkg.load_library(), "75us")


@pytest.mark.parametrize("ns,n", EDGE_SHAPES)
def test_mono_blocked_scan_at_the_edges_of_a_chunk_and_of_a_segment(pkg, ns, n):
    _hold(pkg, ns, n, _alpha75(pkg), np.float32(pp.DEFAULT_GAIN))


@pytest.mark.parametrize("ns,n", [(65, 4865), (2, 9729)])
@pytest.mark.parametrize("name", pp.ALPHAS)
def test_mono_blocked_scan_at_every_alpha(pkg, name, ns, n):
    _hold(pkg, ns, n, pp.alpha_of(pkg.load_library(), name), np.float32(pp.DEFAULT_GAIN))


@pytest.mark.parametrize("gain", pp.GAINS[1:], ids=pp.gain_id)
def test_mono_blocked_scan_at_a_mirrored_a_zero_and_a_saturating_gain(pkg, gain):
    _hold(pkg, 65, 4865, _alpha75(pkg), np.float32(gain))


def test_mono_scan_is_one_channel_of_the_stereo_scan(pkg):
    x = emu.mono_inputs(3, 700)
    a, sa = emu.mono_scan_emulate(x, _alpha75(pkg), pp.DEFAULT_GAIN)
    b, sb = emu.stereo_scan_emulate(x, x[:, ::-1].copy(), _alpha75(pkg), pp.DEFAULT_GAIN)
    assert np.array_equal(a[:, 0::2], b[:, 0::2]) and np.array_equal(sa, sb[:, 0]) and np.array_equal(a[:, 0::2], a[:, 1::2])
