"""CPU checks of the high-cut's C-ABI (include/sdrfm.h): the three symbols exported and declared, what set and get refuse
without a device, the Python argument handling and the slew of a ramp time.  (The refusals that need a sink are tests/test_pcm_hicut_gpu.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrfm_pcm_deemph_stereo_hicut_s16", "sdrfm_pcm_stereo_sink_set_hicut", "sdrfm_pcm_stereo_sink_get_hicut"]


def test_symbols_are_exported_and_declared(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "sdrfm.h")) as fh:
        header = fh.read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
        assert re.search(r"^int\s+%s\(" % n, header, re.M), n
    assert len(set(pkg.ABI_SYMBOLS)) == len(pkg.ABI_SYMBOLS)
    assert re.search(r"^#define SDRFM_HICUT_MIN 1024u$", header, re.M) and pkg.sink.HICUT_MIN == 1024
    assert re.search(r"^#define SDRFM_ABI_VERSION\s+1u?\b", header, re.M) and lib.sdrfm_abi_version() == 1
    for m in ("set_hicut", "clear_hicut", "hicut_state", "condition"):
        assert callable(getattr(pkg.StereoPcmSink, m)), m
    for f in ("pcm_deemph_stereo_hicut_s16_host", "hicut_slew", "hicut_corner_hz", "hicut_policy"):
        assert callable(getattr(pkg, f)) and f in pkg.__all__, f
    # the header says where the default form's caps are claimed
    assert "CLAIMED AND TESTED AT THE TWO BROADCAST ALPHAS ONLY" in header


def test_set_and_get_refuse_a_null_sink_without_a_device(pkg):
    lib = pkg.load_library()
    E = pkg.lib.EINVAL
    h = np.full(4, 32768, np.uint16)
    slew = C.c_uint32(77)
    assert lib.sdrfm_pcm_stereo_sink_set_hicut(None, h.ctypes.data, 40) == E
    assert lib.sdrfm_pcm_stereo_sink_set_hicut(None, None, 0) == E
    assert lib.sdrfm_pcm_stereo_sink_set_hicut(None, None, 40000) == E
    assert lib.sdrfm_pcm_stereo_sink_get_hicut(None, h.ctypes.data, h.ctypes.data, C.byref(slew)) == E
    assert lib.sdrfm_pcm_stereo_sink_get_hicut(None, None, None, None) == E
    assert slew.value == 77 and (h == 32768).all()


def test_slew_of_a_ramp_time(pkg):
    """as BroadcastDemod.set_audio computes its own: max(1, ceil(32768 / samples)), a jump below one sample"""
    assert pkg.hicut_slew(50.0) == 14 and pkg.hicut_slew(50.0, 48000.0) == -(-32768 // 2400)
    assert pkg.hicut_slew(0) == 32768 and pkg.hicut_slew(1.0 / 48.0) == 32768 and pkg.hicut_slew(2.0 / 48.0) == 16384
    assert pkg.hicut_slew(1000.0) == 1 and pkg.hicut_slew(1e9) == 1
    assert pkg.hicut_slew(50.0, 32000.0) == -(-32768 // 1600)
    for bad in (-1.0, float("nan")):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.hicut_slew(bad)
        assert e.value.status == pkg.lib.EINVAL


def test_python_argument_handling(pkg):
    """_hq15 on an object that has only a stream count: floats scale by 32768 and round, ints pass, one value broadcasts; what a uint16 cannot
    hold is refused with the C call's status"""
    sink = pkg.StereoPcmSink.__new__(pkg.StereoPcmSink)
    sink.n_streams = 3
    assert np.array_equal(sink._hq15(0.25), [8192] * 3) and sink._hq15(0.25).dtype == np.uint16
    assert np.array_equal(sink._hq15([1.0, 0.5, 1 / 32]), [32768, 16384, 1024])
    assert np.array_equal(sink._hq15([32768, 1024, 5000]), [32768, 1024, 5000])
    assert np.array_equal(sink._hq15(np.array([1023, 32769, 0])), [1023, 32769, 0])          # (in a uint16: the C call's to refuse)
    for bad in (-0.5, 3.0, float("nan"), 70000, -1):
        with pytest.raises(pkg.SdrfmError) as e:
            sink._hq15(bad)
        assert e.value.status == pkg.lib.EINVAL
    with pytest.raises(ValueError):
        sink._hq15([1.0, 0.5])


def test_corner_of_a_settled_stream(pkg):
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    assert abs(float(pkg.hicut_corner_hz(alpha, 32768, 48000.0)) - 2122.0) < 1.0           # 1 / (2 pi 75 us)
    assert abs(float(pkg.hicut_corner_hz(alpha, 8192, 48000.0)) - 480.0) < 5.0
    c = pkg.hicut_corner_hz(alpha, np.array([1024, 4096, 8192, 32768]), 48000.0)
    assert np.all(np.diff(c) > 0)
    assert np.isinf(pkg.hicut_corner_hz(1.0, 32768, 48000.0))
