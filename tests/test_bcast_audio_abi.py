"""CPU checks of sdrfm_bcast_set_audio and sdrfm_bcast_get_audio: exported, declared, listed; the refusals, none of which
needs a device; the Python mirror's methods and the status they raise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NAMES = ("sdrfm_bcast_set_audio", "sdrfm_bcast_get_audio")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrfm.h")
ARGS = {
    "sdrfm_bcast_set_audio": ["sdrfm_bcast_t* h", "const uint16_t* blend_q15", "const uint16_t* gain_q15", "uint32_t slew_q15"],
    "sdrfm_bcast_get_audio": ["const sdrfm_bcast_t* h", "uint16_t* blend_q15", "uint16_t* gain_q15", "uint16_t* blend_target_q15",
                              "uint16_t* gain_target_q15"],
}


def test_symbols_are_exported_declared_and_listed(pkg):
    lib = pkg.load_library()
    assert lib.sdrfm_abi_version() == 1                            # additive: the version stays
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
        decl = re.search(r"^int\s+%s\(([^;]*)\);" % name, text, re.M)
        assert decl, "%s is not declared in include/sdrfm.h" % name
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
        assert len(args) == len(getattr(lib, name).argtypes), (name, args)
        assert [" ".join(a.split()) for a in args] == ARGS[name], (name, args)
    for n in ("pilot_snr_db", "audio_policy"):
        assert n in pkg.__all__ and callable(getattr(pkg, n)), n


def test_every_refusal_without_a_device(pkg):
    """a NULL handle whatever else is given.  The other three are decided from the arguments and the handle's stream count alone, before the
    device is touched: the stand-in here is a block of zeroed memory whose public head — the handle keeps its sdrfm_bcast_config first, and
    that struct's second word is n_streams — says 3 streams; no refused call may read it further or write to it"""
    lib = pkg.load_library()
    E = pkg.lib.EINVAL
    ok = np.array([0, 16384, 32768], np.uint16)
    over = np.array([0, 32769, 5], np.uint16)
    last = np.array([0, 5, 65535], np.uint16)
    p = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    for b, g, slew in ((ok, ok, 5), (None, None, 0), (None, None, 40), (over, None, 0)):
        assert lib.sdrfm_bcast_set_audio(None, p(b), p(g), slew) == E
    assert lib.sdrfm_bcast_get_audio(None, None, None, None, None) == E
    assert lib.sdrfm_bcast_get_audio(None, p(ok.copy()), None, None, None) == E
    block = C.create_string_buffer(1 << 16)
    C.cast(block, C.POINTER(C.c_uint32))[1] = 3                     # sdrfm_bcast_config.n_streams
    image = block.raw
    h = C.cast(block, C.c_void_p)
    refusals = [(over, ok, 5), (ok, over, 5), (last, None, 1), (None, last, 32768), (over, None, 32768),       # a value above 32768
                (ok, ok, 0), (ok, None, 0), (None, ok, 0),                                                    # a slew of 0 with an array
                (ok, ok, 32769), (None, None, 32769), (ok, ok, 0xFFFFFFFF), (over, over, 65536)]              # a slew above 32768
    for k, (b, g, slew) in enumerate(refusals):
        assert lib.sdrfm_bcast_set_audio(h, p(b), p(g), slew) == E, k
    assert block.raw == image
    assert list(ok) == [0, 16384, 32768] and list(over) == [0, 32769, 5] and list(last) == [0, 5, 65535]


def test_python_mirror_has_the_methods_and_raises_the_status(pkg):
    for n in ("set_audio", "clear_audio", "audio_state", "condition"):
        assert callable(getattr(pkg.BroadcastDemod, n)), n
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    cfg = pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=pkg.lowpass_taps(32, 15e3 / 240e3), rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                              pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), n_streams=2)
    bc = pkg.BroadcastDemod.__new__(pkg.BroadcastDemod)             # a closed handle: every call on it is refused with SDRFM_EINVAL
    bc._lib, bc.cfg, bc._shared_input, bc._h, bc._hc = pkg.load_library(), cfg, False, None, h
    bc._untuned()
    for call, name in ((lambda: bc.set_audio(0.5, 1.0), NAMES[0]), (lambda: bc.set_audio(blend=[0, 32768], ramp_ms=0), NAMES[0]),
                       (lambda: bc.set_audio(gain=[1.0, 0.0]), NAMES[0]), (bc.clear_audio, NAMES[0]), (bc.audio_state, NAMES[1])):
        with pytest.raises(pkg.SdrfmError) as e:
            call()
        assert e.value.status == pkg.lib.EINVAL and name in str(e.value), str(e.value)
    # what a uint16 cannot hold is refused with the same status before the C call
    for kw in (dict(blend=-0.1), dict(gain=[0, 70000]), dict(blend=float("nan")), dict(gain=2.5), dict(ramp_ms=-1.0), dict(ramp_ms=float("nan"))):
        with pytest.raises(pkg.SdrfmError) as e:
            bc.set_audio(**kw)
        assert e.value.status == pkg.lib.EINVAL, kw
    status = [dict(present=True, stereo=True, offset_hz=0.0, level_dbfs=-10.0, stream=0),
              dict(present=False, stereo=False, offset_hz=0.0, level_dbfs=-60.0, stream=1)]
    report = dict(pilot_steadiness=np.array([1.001, 1.9]))
    with pytest.raises(pkg.SdrfmError) as e:
        bc.condition(report, status)
    assert e.value.status == pkg.lib.EINVAL and NAMES[0] in str(e.value)


def test_the_slew_of_a_ramp_time(pkg):
    """slew = max(1, ceil(32768 / (ramp_ms x audio rate / 1000))) at 48 kHz, a jump for ramp_ms = 0: read back from a stand-in library"""
    seen = []

    class Lib:
        def sdrfm_bcast_set_audio(self, h, b, g, slew):
            seen.append(slew)
            return 0
    cfg = pkg.BroadcastConfig(fir_coeffs=np.ones(4, np.float32), audio_coeffs=np.ones(4, np.float32), rds_coeffs=np.ones(4, np.float32),
                              pilot_coeffs=np.ones(3, np.complex64), n_streams=2)
    bc = pkg.BroadcastDemod.__new__(pkg.BroadcastDemod)
    bc._lib, bc.cfg, bc._h = Lib(), cfg, None
    bc._untuned()
    for ms, want in ((50.0, 14), (0.0, 32768), (1000.0, 1), (1e6, 1), (1.0, 683), (0.01, 32768), (10.0, 69)):
        assert bc.set_audio(ramp_ms=ms) == want and seen[-1] == want, (ms, seen[-1], want)
