"""CPU: the arithmetic of the stereo PCM sink's default form (k_pcm_stereo_sink_scan, csrc/sdrfm_sink_stereo.hip: sink_scan_segments<2> of
csrc/sdrfm_sink_kernels.h) restated in numpy
(tools/pcm_stereo_scan_emulate.py), held to the host routine sdrfm_pcm_deemph_stereo_s16 (csrc/pcm_sink.c) on the very inputs
tests/test_pcm_stereo_sink_gpu.py gives the kernel: the three bounds of that test (the mono sink's, tests/test_pcm_sink_gpu.py) hold by the
arithmetic alone, without a GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

import pcm_params as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_stereo_scan_emulate")

SCAN_SHAPES = [(1, 4800), (3, 1), (5, 255), (64, 257), (65, 1300), (2, 30000), (256, 4800)]
# one chunk of 19 samples - 1, whole, + 1; one segment of 256 chunks - 1, whole, + 1; two segments + 1 (tests/test_pcm_sink_params_gpu.py's shapes among them)
EDGE_SHAPES = [(2, 18), (1, 19), (3, 20), (5, 4863), (63, 4864), (65, 4865), (2, 9729)]


def _params(pkg):
    return pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))


@pytest.mark.parametrize("ns,n", SCAN_SHAPES)
def test_blocked_scan_of_two_channels_stays_inside_the_gpu_tests_bounds(pkg, ns, n):
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(ns, n)
    a, sa = emu.stereo_scan_emulate(left[:, :n], right[:, :n], alpha, gain)             # two calls: the states are carried
    b, sb = emu.stereo_scan_emulate(left[:, n:], right[:, n:], alpha, gain, sa)
    got = np.concatenate([a, b], axis=1)
    want, st = emu.host_reference(pkg, left, right, alpha, gain)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (int(d.max()), np.argwhere(d > 1)[:4])
    assert (d != 0).mean() <= 1e-3 + 2.0 / d.size, float((d != 0).mean())
    assert np.all(np.abs(sb - st) <= 1e-6 * np.maximum(np.abs(st), 0.25)), (sb, st)


def _hold(pkg, ns, n, alpha, gain):
    left, right = emu.sink_inputs(ns, n)
    a, sa = emu.stereo_scan_emulate(left[:, :n], right[:, :n], alpha, gain)             # two calls: the states are carried
    b, sb = emu.stereo_scan_emulate(left[:, n:], right[:, n:], alpha, gain, sa)
    got = np.concatenate([a, b], axis=1)
    want, st = emu.host_reference(pkg, left, right, alpha, gain)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, (int(d.max()), np.argwhere(d > 1)[:4])
    assert (d != 0).mean() <= 1e-3 + 2.0 / d.size, float((d != 0).mean())
    assert np.all(np.abs(sb - st) <= 1e-6 * np.maximum(np.abs(st), 0.25)), (sb, st)


@pytest.mark.parametrize("ns,n", EDGE_SHAPES)
def test_blocked_scan_at_the_edges_of_a_chunk_and_of_a_segment(pkg, ns, n):
    alpha, gain = _params(pkg)
    _hold(pkg, ns, n, alpha, gain)


@pytest.mark.parametrize("ns,n", [(65, 4865), (2, 9729)])
@pytest.mark.parametrize("name", pp.ALPHAS)
def test_blocked_scan_at_every_alpha(pkg, name, ns, n):
    """(1 - alpha)^19 squared six times: 0 by the fifth squaring at 75 us, by the first at alpha = 1, never at 0.001 (where a chunk's carry-in does not decay inside
    the chunk) — the three caps hold at each."""
    _hold(pkg, ns, n, pp.alpha_of(pkg.load_library(), name), _params(pkg)[1])


@pytest.mark.parametrize("gain", pp.GAINS[1:], ids=pp.gain_id)
def test_blocked_scan_at_a_mirrored_a_zero_and_a_saturating_gain(pkg, gain):
    _hold(pkg, 65, 4865, _params(pkg)[0], np.float32(gain))


def test_the_inputs_saturate_both_channels_and_the_channels_differ(pkg):
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(5, 255)
    want, _ = emu.host_reference(pkg, left, right, alpha, gain)
    assert want[0, 0::2].max() == 32767 and want[0, 1::2].min() == -32768               # row 0: L clips high where R clips low
    assert not np.array_equal(want[:, 0::2], want[:, 1::2])
    got, _ = emu.stereo_scan_emulate(left, right, alpha, gain)
    assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1


def test_a_channel_of_the_emulator_does_not_depend_on_the_other(pkg):
    """Two chains in one lane share nothing but the powers of (1 - alpha): swapping the channels swaps the PCM slots and the states."""
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(3, 700)
    a, sa = emu.stereo_scan_emulate(left, right, alpha, gain)
    b, sb = emu.stereo_scan_emulate(right, left, alpha, gain)
    assert np.array_equal(a[:, 0::2], b[:, 1::2]) and np.array_equal(a[:, 1::2], b[:, 0::2])
    assert np.array_equal(sa, sb[:, ::-1])
