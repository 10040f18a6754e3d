"""CPU checks of sdrfm_bcast_retune: exported, declared, listed; the refusals that need no device; the Python mirror's
methods and the status they raise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAME = "sdrfm_bcast_retune"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrfm.h")


def test_symbol_is_exported_declared_and_listed(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, NAME) and NAME in pkg.ABI_SYMBOLS
    assert lib.sdrfm_abi_version() == 1                            # additive: the version stays
    text = open(HEADER).read()
    decl = re.search(r"^int\s+%s\(([^;]*)\);" % NAME, text, re.M)
    assert decl, "not declared in include/sdrfm.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert len(args) == len(getattr(lib, NAME).argtypes) == 6, args
    assert args == ["sdrfm_bcast_t* h", "const float* ctaps", "const float* rot", "const float* carry", "const uint8_t* restart", "uint32_t flags"], args
    for n in ("retune_carry", "follow_selection"):
        assert n in pkg.__all__ and callable(getattr(pkg, n)), n


def test_null_arguments_and_unknown_flags_are_refused_without_a_device(pkg):
    """a NULL handle whatever else is given; NULL ctaps, NULL rot and unknown flags are refused before the handle is looked at — the
    stand-in here is a block of zeroed memory, which no call may read further than its refusal"""
    lib = pkg.load_library()
    t, r = np.zeros(2 * 64, np.float32), np.zeros(1, np.float32)
    tp, rp = C.c_void_p(t.ctypes.data), C.c_void_p(r.ctypes.data)
    assert lib.sdrfm_bcast_retune(None, tp, rp, None, None, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_retune(None, None, None, None, None, 0) == pkg.lib.EINVAL
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    assert lib.sdrfm_bcast_retune(h, None, rp, None, None, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_retune(h, tp, None, None, None, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_retune(h, None, None, None, None, pkg.lib.TUNE_SHARED_INPUT) == pkg.lib.EINVAL   # un-tuning stays sdrfm_bcast_tune's job
    for flags in (2, 4, pkg.lib.TUNE_SHARED_INPUT | 0x80000000):
        assert lib.sdrfm_bcast_retune(h, tp, rp, None, None, flags) == pkg.lib.EINVAL, flags
    assert block.raw == bytes(1 << 16)
    assert not t.any() and not r.any()


def test_python_mirror_has_the_methods_and_raises_the_status(pkg):
    for n in ("retune", "follow"):
        assert callable(getattr(pkg.BroadcastDemod, n)), n
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    cfg = pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=pkg.lowpass_taps(32, 15e3 / 240e3), rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                              pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), n_streams=2)
    bc = pkg.BroadcastDemod.__new__(pkg.BroadcastDemod)             # a closed handle: every call on it is refused with SDRFM_EINVAL
    bc._lib, bc.cfg, bc._shared_input, bc._h, bc._hc = pkg.load_library(), cfg, False, None, h
    bc._untuned()
    assert list(bc._offsets_hz) == [0.0, 0.0]                        # an untuned handle remembers 0
    with pytest.raises(pkg.SdrfmError) as e:
        bc.retune(offsets_hz=[100e3, -200e3])
    assert e.value.status == pkg.lib.EINVAL and NAME in str(e.value)
    assert list(bc._offsets_hz) == [0.0, 0.0]                        # a refused call is not remembered
    with pytest.raises(pkg.SdrfmError) as e:
        bc.retune()                                                  # neither offsets nor taps: the C call's own refusal
    assert e.value.status == pkg.lib.EINVAL
    status = [dict(present=True, stereo=True, offset_hz=7e3, level_dbfs=-10.0, stream=0),
              dict(present=False, stereo=False, offset_hz=0.0, level_dbfs=-60.0, stream=1)]
    with pytest.raises(pkg.SdrfmError) as e:
        bc.follow(status)
    assert e.value.status == pkg.lib.EINVAL
    quiet = [dict(s, offset_hz=0.0) for s in status]
    assert bc.follow(quiet) == []                                    # nothing to move: no call at all
