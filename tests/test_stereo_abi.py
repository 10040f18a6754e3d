"""CPU checks of the sdrfm_stereo_* C-ABI: exported, every invalid configuration refused before a device is looked for, NULL handles
refused, and the stereo PCM helper equal to the mono routine per channel."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["sdrfm_stereo_create", "sdrfm_stereo_destroy", "sdrfm_stereo_reset", "sdrfm_stereo_audio_count", "sdrfm_stereo_process_batch",
         "sdrfm_stereo_set_stream", "sdrfm_stereo_synchronize", "sdrfm_stereo_kernel_name", "sdrfm_pcm_deemph_stereo_s16"]


def test_stereo_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n


def _cfg(pkg, keep, **kw):
    lib = pkg.lib
    h, g = pkg.default_config()
    b = np.zeros(2 * 101, np.float32)
    b[0::2] = pkg.stereo_pilot_taps(101, 240e3).real
    vals = dict(n_streams=4, fir_taps=64, fir_decim=10, h=h, pilot_taps=101, b=b, pilot_min=0.05, diff_gain=2.0, audio_taps=32,
                audio_decim=5, g=g, max_bytes_per_call=0, device=0, flags=0, struct_size=C.sizeof(lib.StereoConfig))
    vals.update(kw)
    fp = C.POINTER(C.c_float)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    hh, bb, gg = arr(vals["h"]), arr(vals["b"]), arr(vals["g"])
    keep += [hh, bb, gg]
    c = lib.StereoConfig()
    c.struct_size, c.n_streams = vals["struct_size"], vals["n_streams"]
    c.fir_taps, c.fir_decim = vals["fir_taps"], vals["fir_decim"]
    c.fir_coeffs = hh.ctypes.data_as(fp) if hh is not None else None
    c.pilot_taps = vals["pilot_taps"]
    c.pilot_coeffs = bb.ctypes.data_as(fp) if bb is not None else None
    c.pilot_min, c.diff_gain = vals["pilot_min"], vals["diff_gain"]
    c.audio_taps, c.audio_decim = vals["audio_taps"], vals["audio_decim"]
    c.audio_coeffs = gg.ctypes.data_as(fp) if gg is not None else None
    c.max_bytes_per_call, c.device, c.flags = vals["max_bytes_per_call"], vals["device"], vals["flags"]
    return c


def _create(pkg, **kw):
    lib = pkg.load_library()
    keep = []
    c = _cfg(pkg, keep, **kw)
    hnd = C.c_void_p()
    rc = lib.sdrfm_stereo_create(C.byref(c), C.byref(hnd))
    if rc == pkg.lib.OK:
        lib.sdrfm_stereo_destroy(hnd)
    return rc


BAD = {
    "P_even": dict(pilot_taps=100), "P_zero": dict(pilot_taps=0), "P_over_255": dict(pilot_taps=257, b=np.zeros(2 * 257, np.float32)),
    "pilot_min_zero": dict(pilot_min=0.0), "pilot_min_negative": dict(pilot_min=-0.05), "pilot_min_nan": dict(pilot_min=float("nan")),
    "pilot_min_inf": dict(pilot_min=float("inf")), "pilot_min_square_underflows": dict(pilot_min=2e-23),
    "pilot_min_smallest_denormal": dict(pilot_min=float(np.nextafter(np.float32(0), np.float32(1)))),"diff_gain_nan": dict(diff_gain=float("nan")), "diff_gain_inf": dict(diff_gain=float("inf")),
    "T_zero": dict(fir_taps=0), "T_over": dict(fir_taps=257, h=np.zeros(257, np.float32)), "D_zero": dict(fir_decim=0), "D_over": dict(fir_decim=65),
    "Ta_zero": dict(audio_taps=0), "Ta_over": dict(audio_taps=257, g=np.zeros(257, np.float32)), "Da_zero": dict(audio_decim=0),
    "Da_over": dict(audio_decim=65), "null_h": dict(h=None), "null_g": dict(g=None), "null_b": dict(b=None), "streams_zero": dict(n_streams=0),
    "struct_size": dict(struct_size=8), "flags": dict(flags=2), "nan_pilot_tap": dict(b=np.full(202, np.nan, np.float32)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_configs_are_refused_without_a_device(pkg, case):
    assert _create(pkg, **BAD[case]) == pkg.lib.EINVAL


def test_valid_config_looks_for_the_device(pkg):
    rc = _create(pkg)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if has_gpu:
        assert rc == pkg.lib.OK
    else:
        assert rc == pkg.lib.NO_DEVICE


def test_null_handles_are_refused(pkg):
    lib = pkg.load_library()
    n = C.c_uint32()
    assert lib.sdrfm_stereo_create(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_reset(None) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_audio_count(None, 100, C.byref(n)) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_process_batch(None, None, 0, 100, None, None, 0, None, C.byref(n), 0) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_synchronize(None) == pkg.lib.EINVAL
    assert lib.sdrfm_stereo_kernel_name(None) == b""
    lib.sdrfm_stereo_destroy(None)


def test_stereo_pcm_with_equal_channels_is_the_mono_routine(pkg):
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(5000) * 0.4).astype(np.float32)
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    pcm_s, st_s = pkg.pcm_deemph_stereo_s16_host(a, a, alpha, gain, (0.25, 0.25))
    pcm_m, st_m = pkg.pcm_deemph_s16_host(a, alpha, gain, 0.25)
    assert np.array_equal(pcm_s, pcm_m)
    assert np.float32(st_s[0]) == np.float32(st_m) and np.float32(st_s[1]) == np.float32(st_m)


def test_stereo_pcm_channels_are_independent_and_carry_state(pkg):
    rng = np.random.default_rng(2)
    L = (rng.standard_normal(3000) * 0.5).astype(np.float32)
    R = (rng.standard_normal(3000) * 2.0).astype(np.float32)   # (saturates in places)
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 50e-6), 9000.0
    st, stl, str_ = (0.0, 0.0), 0.0, 0.0
    for lo, hi in ((0, 1000), (1000, 1001), (1001, 3000)):
        pcm, st = pkg.pcm_deemph_stereo_s16_host(L[lo:hi], R[lo:hi], alpha, gain, st)
        wl, stl = pkg.pcm_deemph_s16_host(L[lo:hi], alpha, gain, stl)
        wr, str_ = pkg.pcm_deemph_s16_host(R[lo:hi], alpha, gain, str_)
        assert np.array_equal(pcm[0::2], wl[0::2]) and np.array_equal(pcm[1::2], wr[0::2])
        assert np.float32(st[0]) == np.float32(stl) and np.float32(st[1]) == np.float32(str_)


def test_stereo_pcm_argument_checks(pkg):
    lib = pkg.load_library()
    st = (C.c_float * 2)()
    x = np.zeros(4, np.float32)
    out = np.zeros(8, np.int16)
    assert lib.sdrfm_pcm_deemph_stereo_s16(x.ctypes.data, None, 4, 0.5, 1.0, st, out.ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_deemph_stereo_s16(x.ctypes.data, x.ctypes.data, 4, 0.0, 1.0, st, out.ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_deemph_stereo_s16(x.ctypes.data, x.ctypes.data, 4, 0.5, 1.0, None, out.ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_deemph_stereo_s16(None, None, 0, 0.5, 1.0, st, None) == pkg.lib.OK
