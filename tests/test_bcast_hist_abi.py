"""CPU checks of sdrfm_bcast_process_batch_metered_hist: exported, declared, listed; its own refusals on a stand-in handle
before the handle is read, then the metered call's in their order, with nothing written; the Python mirror's methods and the status they
raise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAME, NAME_FN = "sdrfm_bcast_process_batch_metered_hist", "sdrfm_bcast_hist_kernel_name"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrfm.h")
BINS = 512


def test_symbols_are_exported_declared_and_listed(pkg):
    lib = pkg.load_library()
    for n in (NAME, NAME_FN):
        assert hasattr(lib, n) and n in pkg.ABI_SYMBOLS, n
    assert lib.sdrfm_abi_version() == 1
    text = open(HEADER).read()
    decl = re.search(r"^int\s+%s\(([^;]*)\);" % NAME, text, re.M)
    assert decl, "not declared in include/sdrfm.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")]
    metered = re.search(r"^int\s+sdrfm_bcast_process_batch_metered\(([^;]*)\);", text, re.M)
    margs = [a.strip() for a in re.sub(r"/\*.*?\*/", "", metered.group(1)).split(",")]
    # the metered call's arguments with hist and hist_stride behind meters
    assert args == margs[:14] + ["uint32_t* hist", "size_t hist_stride"] + margs[14:], (args, margs)
    assert len(args) == len(getattr(lib, NAME).argtypes) == 19
    assert re.search(r"^const char\*\s+%s\(const sdrfm_bcast_t\* h\);" % NAME_FN, text, re.M)
    assert lib.sdrfm_bcast_hist_kernel_name(None) == b""
    assert "#define SDRFM_SCAN_HIST_BINS 512u" in text


def _call(lib, h, meters, hist, stride, na, nr, pcm=None, flags=0, nbytes=100):
    return lib.sdrfm_bcast_process_batch_metered_hist(h, None, None, 0, nbytes, None, None, 0, pcm, 0, None, 0, None, meters, hist, stride, na, nr, flags)


def test_refusals_that_need_no_device(pkg):
    """a NULL handle whatever else is given; on a stand-in handle of zeroed memory NULL meters, NULL hist and hist_stride 511 and 0 are
    refused before the handle is read — with arguments that every later check would refuse as well, so only the order is free —, then the
    metered call's own: NULL counts, pcm without a sink, records off 8 bytes, rows off 4, and the tap sums (a zeroed handle has meter_ok
    clear).  Nothing is written"""
    lib, EINVAL = pkg.load_library(), pkg.lib.EINVAL
    na, nr = C.c_uint32(7), C.c_uint32(7)
    meters = np.full(4, 5, pkg.METER_DTYPE)
    hist = np.full((4, BINS + 1), 9, np.uint32)
    m, hp = C.c_void_p(meters.ctypes.data), C.c_void_p(hist.ctypes.data)
    A, R = C.byref(na), C.byref(nr)
    assert _call(lib, None, m, hp, BINS, A, R) == EINVAL
    assert _call(lib, None, None, None, 0, None, None) == EINVAL
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    assert _call(lib, h, None, hp, BINS, A, R) == EINVAL
    assert _call(lib, h, m, None, BINS, A, R) == EINVAL
    assert _call(lib, h, m, hp, BINS - 1, A, R) == EINVAL
    assert _call(lib, h, m, hp, 0, A, R) == EINVAL
    assert _call(lib, h, m, hp, BINS - 1, A, R, nbytes=101, flags=pkg.lib.F_OVERLAP) == EINVAL   # before the flags' and the odd count's
    # the metered call's own, in its order
    assert _call(lib, h, m, hp, BINS, None, R) == EINVAL
    assert _call(lib, h, m, hp, BINS, A, None) == EINVAL
    pcm = np.zeros(8, np.int16)
    assert _call(lib, h, m, hp, BINS, A, R, pcm=C.c_void_p(pcm.ctypes.data)) == EINVAL
    assert _call(lib, h, C.c_void_p(meters.ctypes.data + 4), hp, BINS, A, R) == EINVAL
    assert _call(lib, h, m, C.c_void_p(hist.ctypes.data + 2), BINS, A, R) == EINVAL
    assert _call(lib, h, m, hp, BINS, A, R) == EINVAL                     # the tap sums: before the odd count's SDRFM_EODD ...
    assert _call(lib, h, m, hp, BINS, A, R, nbytes=101) == EINVAL         # ... as in the metered call
    assert (na.value, nr.value) == (7, 7) and (meters["n"] == 5).all() and (meters["reserved"] == 5).all() and (hist == 9).all()
    assert block.raw == bytes(1 << 16)


def test_python_mirror_has_the_methods_and_raises_the_status(pkg):
    for n in ("process_batch_metered_hist", "process_batch_metered_hist_device", "hist_kernel_name"):
        assert callable(getattr(pkg.BroadcastDemod, n)), n
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    cfg = pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=pkg.lowpass_taps(32, 15e3 / 240e3), rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                              pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3))
    bc = pkg.BroadcastDemod.__new__(pkg.BroadcastDemod)             # a closed handle: every call on it is refused with SDRFM_EINVAL
    bc._lib, bc.cfg, bc._shared_input, bc._h = pkg.load_library(), cfg, False, None
    with pytest.raises(pkg.SdrfmError) as e:
        bc.process_batch_metered_hist(np.zeros((1, 100), np.uint8))
    assert e.value.status == pkg.lib.EINVAL
    assert bc.hist_kernel_name() == ""
    with pytest.raises(pkg.SdrfmError) as e:
        bc._ck(_call(bc._lib, None, None, None, 0, None, None), NAME)
    assert e.value.status == pkg.lib.EINVAL and NAME in str(e.value)
    # the readers of the scan handle's rows take these as they are
    for n in ("hist_add", "hist_report", "deviation_quantile", "ModulationMonitor"):
        assert n in pkg.__all__, n
