"""CPU checks of the sdrfm_pcm_stereo_sink_* C-ABI and the two one-call forms that use it: exported, every invalid create argument refused
before a device is looked for, NULL handles harmless."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["sdrfm_pcm_stereo_sink_create", "sdrfm_pcm_stereo_sink_destroy", "sdrfm_pcm_stereo_sink_reset", "sdrfm_pcm_stereo_sink_process_batch",
         "sdrfm_pcm_stereo_sink_set_stream", "sdrfm_pcm_stereo_sink_synchronize", "sdrfm_pcm_stereo_sink_get_state",
         "sdrfm_stereo_process_batch_pcm", "sdrfm_bcast_process_batch_pcm"]


def test_stereo_sink_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
        assert "_host_" not in n and "_dev_" not in n and "debug" not in n
    assert len(set(pkg.ABI_SYMBOLS)) == len(pkg.ABI_SYMBOLS)
    assert hasattr(pkg, "StereoPcmSink") and "StereoPcmSink" in pkg.__all__
    for cls, meths in ((pkg.StereoPcmSink, ("process_batch", "process_batch_device", "state", "reset", "set_stream", "synchronize")),
                       (pkg.StereoDemod, ("process_batch_pcm", "process_batch_pcm_device")),
                       (pkg.BroadcastDemod, ("process_batch_pcm", "process_batch_pcm_device"))):
        for m in meths:
            assert callable(getattr(cls, m)), (cls, m)


BAD = {
    "streams_zero": (0, 0.24, 1.0), "alpha_zero": (4, 0.0, 1.0), "alpha_negative": (4, -0.1, 1.0), "alpha_above_one": (4, 1.0001, 1.0),
    "alpha_nan": (4, float("nan"), 1.0), "alpha_inf": (4, float("inf"), 1.0), "gain_nan": (4, 0.24, float("nan")),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_create_arguments_are_refused_without_a_device(pkg, case):
    lib = pkg.load_library()
    ns, alpha, gain = BAD[case]
    out = C.c_void_p(1)
    assert lib.sdrfm_pcm_stereo_sink_create(ns, alpha, gain, 0, C.byref(out)) == pkg.lib.EINVAL
    assert not out.value


def test_create_without_an_out_pointer(pkg):
    assert pkg.load_library().sdrfm_pcm_stereo_sink_create(4, 0.24, 1.0, 0, None) == pkg.lib.EINVAL


@pytest.mark.parametrize("args", [(4, 0.24, 16000.0), (1, 1.0, 0.0), (256, 1e-6, float("inf"))], ids=["usual", "alpha_one_gain_zero", "gain_inf"])
def test_valid_create_looks_for_the_device(pkg, args):
    lib = pkg.load_library()
    out = C.c_void_p()
    rc = lib.sdrfm_pcm_stereo_sink_create(*args, 0, C.byref(out))
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    assert rc == (pkg.lib.OK if has_gpu else pkg.lib.NO_DEVICE)
    if rc == pkg.lib.OK:
        lib.sdrfm_pcm_stereo_sink_destroy(out)
    else:
        assert not out.value


def test_null_handles_are_harmless(pkg):
    lib = pkg.load_library()
    E = pkg.lib.EINVAL
    x = np.zeros(8, np.float32)
    pcm = np.zeros(16, np.int16)
    st = (C.c_float * 2)()
    n, m = C.c_uint32(), C.c_uint32()
    assert lib.sdrfm_pcm_stereo_sink_reset(None) == E
    assert lib.sdrfm_pcm_stereo_sink_process_batch(None, x.ctypes.data, x.ctypes.data, 8, 8, pcm.ctypes.data, 16, 0) == E
    assert lib.sdrfm_pcm_stereo_sink_process_batch(None, None, None, 0, 0, None, 0, 0) == E
    assert lib.sdrfm_pcm_stereo_sink_set_stream(None, None) == E
    assert lib.sdrfm_pcm_stereo_sink_synchronize(None) == E
    assert lib.sdrfm_pcm_stereo_sink_get_state(None, st) == E
    assert lib.sdrfm_stereo_process_batch_pcm(None, None, None, 0, 0, None, None, 0, None, 0, None, C.byref(n), 0) == E
    assert lib.sdrfm_bcast_process_batch_pcm(None, None, None, 0, 0, None, None, 0, None, 0, None, 0, None, C.byref(n), C.byref(m), 0) == E
    lib.sdrfm_pcm_stereo_sink_destroy(None)


def test_python_mirror_raises_the_status(pkg):
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.StereoPcmSink(4, 0.0, 1.0)
    assert e.value.status == pkg.lib.EINVAL
