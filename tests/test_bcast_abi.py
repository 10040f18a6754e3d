"""CPU checks of the sdrfm_bcast_* C-ABI: exported, every invalid configuration refused before a device is looked for, NULL handles
harmless."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["sdrfm_bcast_create", "sdrfm_bcast_destroy", "sdrfm_bcast_reset", "sdrfm_bcast_counts", "sdrfm_bcast_process_batch",
         "sdrfm_bcast_set_stream", "sdrfm_bcast_synchronize", "sdrfm_bcast_kernel_name"]


def test_bcast_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
        assert "_host_" not in n and "_dev_" not in n and "debug" not in n
    assert lib.sdrfm_abi_version() == 1
    for n in ("BroadcastDemod", "BroadcastConfig"):
        assert hasattr(pkg, n) and n in pkg.__all__, n


def _cfg(pkg, keep, **kw):
    lib = pkg.lib
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    ga = pkg.lowpass_taps(32, 15e3 / 240e3)
    gr = pkg.rds_lowpass_taps(255, 240e3)
    b = np.zeros(2 * 101, np.float32)
    b[0::2] = pkg.stereo_pilot_taps(101, 240e3).real
    vals = dict(n_streams=4, fir_taps=64, fir_decim=10, h=h, pilot_taps=101, b=b, pilot_min=0.05, diff_gain=2.1, audio_taps=32, audio_decim=5,
                ga=ga, rds_gain=2.2, rds_taps=255, rds_decim=25, gr=gr, max_bytes_per_call=0, device=0, flags=0,
                struct_size=C.sizeof(lib.BcastConfig))
    vals.update(kw)
    fp = C.POINTER(C.c_float)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    hh, bb, gga, ggr = arr(vals["h"]), arr(vals["b"]), arr(vals["ga"]), arr(vals["gr"])
    keep += [hh, bb, gga, ggr]
    ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
    c = lib.BcastConfig()
    c.struct_size, c.n_streams = vals["struct_size"], vals["n_streams"]
    c.fir_taps, c.fir_decim, c.fir_coeffs = vals["fir_taps"], vals["fir_decim"], ptr(hh)
    c.pilot_taps, c.pilot_coeffs = vals["pilot_taps"], ptr(bb)
    c.pilot_min, c.diff_gain, c.rds_gain = vals["pilot_min"], vals["diff_gain"], vals["rds_gain"]
    c.audio_taps, c.audio_decim, c.audio_coeffs = vals["audio_taps"], vals["audio_decim"], ptr(gga)
    c.rds_taps, c.rds_decim, c.rds_coeffs = vals["rds_taps"], vals["rds_decim"], ptr(ggr)
    c.max_bytes_per_call, c.device, c.flags = vals["max_bytes_per_call"], vals["device"], vals["flags"]
    return c


def _create(pkg, **kw):
    lib = pkg.load_library()
    keep = []
    c = _cfg(pkg, keep, **kw)
    hnd = C.c_void_p()
    rc = lib.sdrfm_bcast_create(C.byref(c), C.byref(hnd))
    if rc == pkg.lib.OK:
        lib.sdrfm_bcast_destroy(hnd)
    else:
        assert not hnd.value
    return rc


def _with(n, idx, v):
    a = np.full(n, 0.01, np.float32)
    a[idx] = v
    return a


BAD = {
    "struct_size": dict(struct_size=8), "struct_size_plus": dict(struct_size=200), "streams_zero": dict(n_streams=0),
    "P_even": dict(pilot_taps=100), "P_zero": dict(pilot_taps=0), "P_over_255": dict(pilot_taps=257, b=np.zeros(2 * 257, np.float32)),
    "Ta_zero": dict(audio_taps=0), "Ta_over": dict(audio_taps=257, ga=np.zeros(257, np.float32)),
    "Da_zero": dict(audio_decim=0), "Da_over": dict(audio_decim=65),
    "Tr_zero": dict(rds_taps=0), "Tr_over": dict(rds_taps=257, gr=np.zeros(257, np.float32)),
    "Dr_zero": dict(rds_decim=0), "Dr_over": dict(rds_decim=65),
    "T_zero": dict(fir_taps=0), "T_over": dict(fir_taps=257, h=np.zeros(257, np.float32)), "D_zero": dict(fir_decim=0), "D_over": dict(fir_decim=65),
    "null_h": dict(h=None), "null_ga": dict(ga=None), "null_gr": dict(gr=None), "null_b": dict(b=None),
    "nan_fir_tap": dict(h=_with(64, 63, np.nan)), "inf_fir_tap": dict(h=_with(64, 0, np.inf)),
    "nan_audio_tap": dict(ga=_with(32, 31, np.nan)), "inf_audio_tap": dict(ga=_with(32, 0, -np.inf)),
    "nan_rds_tap": dict(gr=_with(255, 0, np.nan)), "inf_rds_tap": dict(gr=_with(255, 254, np.inf)),
    "nan_pilot_tap": dict(b=_with(202, 201, np.nan)), "inf_pilot_tap": dict(b=_with(202, 0, np.inf)),
    "diff_gain_nan": dict(diff_gain=float("nan")), "diff_gain_inf": dict(diff_gain=float("inf")),
    "rds_gain_nan": dict(rds_gain=float("nan")), "rds_gain_inf": dict(rds_gain=float("-inf")),
    "pilot_min_zero": dict(pilot_min=0.0), "pilot_min_negative": dict(pilot_min=-0.05), "pilot_min_nan": dict(pilot_min=float("nan")),
    "pilot_min_inf": dict(pilot_min=float("inf")), "pilot_min_square_underflows": dict(pilot_min=2e-23),
    "pilot_min_smallest_denormal": dict(pilot_min=float(np.nextafter(np.float32(0), np.float32(1)))),
    "flags_unknown": dict(flags=2), "flags_high": dict(flags=0x80000001),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_configs_are_refused_without_a_device(pkg, case):
    assert _create(pkg, **BAD[case]) == pkg.lib.EINVAL


def test_the_stereo_and_rds_structs_sizes_are_refused(pkg):
    lib = pkg.lib
    sizes = {C.sizeof(lib.StereoConfig), C.sizeof(lib.RdsConfig)}
    assert C.sizeof(lib.BcastConfig) not in sizes
    for sz in sizes:
        assert _create(pkg, struct_size=sz) == lib.EINVAL


@pytest.mark.parametrize("kw", [dict(), dict(flags=1), dict(rds_taps=1, rds_decim=1, gr=np.ones(1, np.float32)),
                                dict(audio_taps=1, audio_decim=1, ga=np.ones(1, np.float32)), dict(rds_gain=0.0, diff_gain=0.0),
                                dict(pilot_min=1e20)],
                         ids=["default", "force_generic", "Tr1_Dr1", "Ta1_Da1", "gains_zero", "pmin2_inf"])
def test_valid_config_looks_for_the_device(pkg, kw):
    rc = _create(pkg, **kw)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    assert rc == (pkg.lib.OK if has_gpu else pkg.lib.NO_DEVICE)


def test_null_handles_are_harmless(pkg):
    lib = pkg.load_library()
    na, nr = C.c_uint32(), C.c_uint32()
    keep = []
    c = _cfg(pkg, keep)
    assert lib.sdrfm_bcast_create(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_create(C.byref(c), None) == pkg.lib.EINVAL
    h = C.c_void_p(1)
    assert lib.sdrfm_bcast_create(None, C.byref(h)) == pkg.lib.EINVAL and not h.value
    assert lib.sdrfm_bcast_reset(None) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_counts(None, 100, C.byref(na), C.byref(nr)) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_process_batch(None, None, 0, 100, None, None, 0, None, 0, None, C.byref(na), C.byref(nr), 0) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_synchronize(None) == pkg.lib.EINVAL
    assert lib.sdrfm_bcast_kernel_name(None) == b""
    lib.sdrfm_bcast_destroy(None)


def test_python_mirror_raises_the_status(pkg):
    h = pkg.lowpass_taps(64, 120e3 / 2.4e6)
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=pkg.lowpass_taps(32, 15e3 / 240e3),
                                               rds_coeffs=pkg.rds_lowpass_taps(255, 240e3), pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3)[:100]))
    assert e.value.status == pkg.lib.EINVAL
