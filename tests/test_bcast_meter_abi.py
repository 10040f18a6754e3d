"""CPU checks of sdrfm_bcast_process_batch_metered: exported, declared, listed; the refusals that need no device; the
Python mirror's methods and the status they raise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAME = "sdrfm_bcast_process_batch_metered"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrfm.h")


def test_symbol_is_exported_declared_and_listed(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, NAME) and NAME in pkg.ABI_SYMBOLS
    assert lib.sdrfm_abi_version() == 1
    text = open(HEADER).read()
    decl = re.search(r"^int\s+%s\(([^;]*)\);" % NAME, text, re.M)
    assert decl, "not declared in include/sdrfm.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")]
    assert len(args) == len(getattr(lib, NAME).argtypes) == 17, args
    assert args[1].startswith("sdrfm_pcm_stereo_sink_t*") and args[13] == "sdrfm_scan_meter* meters" and args[16] == "uint32_t flags", args
    assert "stream_status" in pkg.__all__ and callable(pkg.stream_status)


def _call(lib, h, meters, na, nr, pcm=None, flags=0):
    return lib.sdrfm_bcast_process_batch_metered(h, None, None, 0, 100, None, None, 0, pcm, 0, None, 0, None, meters, na, nr, flags)


def test_null_arguments_are_refused_without_a_device(pkg):
    """a NULL handle whatever else is given; NULL meters, NULL counts and pcm without a sink are refused before the handle is looked at —
    the stand-in here is a block of zeroed memory, which no call may read further than its refusal"""
    lib = pkg.load_library()
    na, nr = C.c_uint32(7), C.c_uint32(7)
    meters = np.full(4, 5, pkg.METER_DTYPE)
    m = C.c_void_p(meters.ctypes.data)
    assert _call(lib, None, m, C.byref(na), C.byref(nr)) == pkg.lib.EINVAL
    assert _call(lib, None, None, None, None) == pkg.lib.EINVAL
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    assert _call(lib, h, None, C.byref(na), C.byref(nr)) == pkg.lib.EINVAL
    assert _call(lib, h, m, None, C.byref(nr)) == pkg.lib.EINVAL
    assert _call(lib, h, m, C.byref(na), None) == pkg.lib.EINVAL
    pcm = np.zeros(8, np.int16)
    assert _call(lib, h, m, C.byref(na), C.byref(nr), pcm=C.c_void_p(pcm.ctypes.data)) == pkg.lib.EINVAL
    assert _call(lib, h, C.c_void_p(meters.ctypes.data + 4), C.byref(na), C.byref(nr)) == pkg.lib.EINVAL      # records not 8-byte aligned
    assert (na.value, nr.value) == (7, 7) and (meters["n"] == 5).all() and (meters["reserved"] == 5).all()   # a refusal writes nothing
    assert block.raw == bytes(1 << 16)


def test_python_mirror_has_the_methods_and_raises_the_status(pkg):
    for n in ("process_batch_metered", "process_batch_metered_device"):
        assert callable(getattr(pkg.BroadcastDemod, n)), n
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    cfg = pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=pkg.lowpass_taps(32, 15e3 / 240e3), rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                              pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3))
    bc = pkg.BroadcastDemod.__new__(pkg.BroadcastDemod)             # a closed handle: every call on it is refused with SDRFM_EINVAL
    bc._lib, bc.cfg, bc._shared_input, bc._h = pkg.load_library(), cfg, False, None
    with pytest.raises(pkg.SdrfmError) as e:
        bc.process_batch_metered(np.zeros((1, 100), np.uint8))
    assert e.value.status == pkg.lib.EINVAL
    # the call itself, past counts(): the status it returns is the one raised
    with pytest.raises(pkg.SdrfmError) as e:
        bc._ck(_call(bc._lib, None, None, None, None), NAME)
    assert e.value.status == pkg.lib.EINVAL and NAME in str(e.value)
