"""The look-ahead PCM limiter's C-ABI (include/sdrfm.h) without a device: the symbols, the structs' layouts in the header, in
ctypes and in numpy, the ABI version, the tile constant the GPU tests place their shapes around, every refusal that is made before a device is
looked for, and the Python policies on hand-computed values."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_pcm_limit_create", "sdrfm_pcm_limit_destroy", "sdrfm_pcm_limit_reset", "sdrfm_pcm_limit_set_params", "sdrfm_pcm_limit_set_gain",
           "sdrfm_pcm_limit_get_params", "sdrfm_pcm_limit_process_batch", "sdrfm_pcm_limit_read", "sdrfm_pcm_limit_get_state",
           "sdrfm_pcm_limit_set_stream", "sdrfm_pcm_limit_synchronize", "sdrfm_pcm_limit_kernel_name", "sdrfm_pcm_limit_s16",
           "sdrfm_pcm_limit_state_words", "sdrfm_pcm_limit_state_init", "sdrfm_pcm_limit_check_params", "sdrfm_pcm_limit_add",
           "sdrfm_pcm_limit_report", "sdrfm_pcm_limit_ceiling"]


def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    text = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdrfm_pcm_limit_[a-z0-9_]+)\s*\(", src))
    assert declared == set(SYMBOLS)
    dyn = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and (" T " + sym) in dyn and getattr(lib, sym).argtypes is not None, sym
    assert lib.sdrfm_abi_version() == 1
    assert re.search(r"^#define\s+SDRFM_ABI_VERSION\s+1u?\s*$", text, flags=re.M)
    tile = re.search(r"^#define\s+SDRFM_PCM_LIMIT_TILE\s+(\d+)u?\b", text, flags=re.M)
    assert tile and int(tile.group(1)) == pkg.limit.TILE
    for name in ("PcmLimiter", "LIMIT_DTYPE", "pcm_limit_host", "limit_add", "limit_report", "limit_ceiling", "limit_release", "normalise_gain_q12"):
        assert name in pkg.__all__ and hasattr(pkg, name), name


def test_struct_layouts_in_ctypes_and_numpy(pkg):
    cfg, par, rec, rep = pkg.lib.PcmLimitConfig, pkg.lib.PcmLimitParams, pkg.lib.PcmLimitRec, pkg.lib.PcmLimitReport
    lay = lambda s: [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]
    assert lay(cfg) == [("n_streams", 0, 4), ("log2_window", 4, 4), ("gain_slew", 8, 4), ("flags", 12, 4), ("device", 16, 4)] and C.sizeof(cfg) == 20
    assert lay(par) == [("ceiling", 0, 4), ("release", 4, 4), ("gain0", 8, 4), ("gain_t", 12, 4)] and C.sizeof(par) == 16
    assert lay(rec) == [("n", 0, 8), ("limited", 8, 8), ("min_gain", 16, 8), ("at", 24, 8)] and C.sizeof(rec) == 32
    assert lay(rep) == [("reduction_db", 0, 8), ("limited_frac", 8, 8), ("at_seconds", 16, 8)] and C.sizeof(rep) == 24
    d = pkg.LIMIT_DTYPE
    assert d.itemsize == 32 and [(n, d.fields[n][1], d.fields[n][0].str) for n in d.names] == [("n", 0, "<u8"), ("limited", 8, "<u8"), ("min_gain", 16, "<u8"), ("at", 24, "<u8")]
    p = pkg.limit.LIMIT_PARAMS_DTYPE
    assert p.itemsize == 16 and [(n, p.fields[n][1]) for n in p.names] == [("ceiling", 0), ("release", 4), ("gain0", 8), ("gain_t", 12)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_in_the_header(tmp_path):
    """the same offsets from the header itself, compiled as C99"""
    fields = [("sdrfm_pcm_limit_config", ("n_streams", "log2_window", "gain_slew", "flags", "device")),
              ("sdrfm_pcm_limit_params", ("ceiling", "release", "gain0", "gain_t")),
              ("sdrfm_pcm_limit_rec", ("n", "limited", "min_gain", "at")),
              ("sdrfm_pcm_limit_report_t", ("reduction_db", "limited_frac", "at_seconds"))]
    args = ", ".join(["offsetof(%s, %s)" % (s, f) for s, fs in fields for f in fs] + ["sizeof(%s)" % s for s, _ in fields])
    count = sum(len(fs) for _, fs in fields) + len(fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdrfm.h"\nint main(void) { printf("%s%%u %%u\\n", %s, (unsigned)SDRFM_ABI_VERSION, '
                   "(unsigned)SDRFM_PCM_LIMIT_TILE); return 0; }\n" % ("%zu " * count, args))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True,
                   capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [0, 4, 8, 12, 16, 0, 4, 8, 12, 0, 8, 16, 24, 0, 8, 16, 20, 16, 32, 24, 1, 5120]


def test_create_refuses_before_any_device_is_looked_for(pkg):
    """a bad config: SDRFM_EINVAL with or without a device — on a box without one a legal config answers SDRFM_NO_DEVICE, which shows the order"""
    import torch
    lib = pkg.load_library()
    out = C.c_void_p(1)
    assert lib.sdrfm_pcm_limit_create(None, C.byref(out)) == pkg.lib.EINVAL and not out.value
    good = dict(n_streams=1, log2_window=6, gain_slew=1, flags=0, device=0)
    cfg = pkg.lib.PcmLimitConfig(**good)
    assert lib.sdrfm_pcm_limit_create(C.byref(cfg), None) == pkg.lib.EINVAL
    for kw in (dict(n_streams=0), dict(flags=1), dict(log2_window=1), dict(log2_window=9), dict(log2_window=0), dict(gain_slew=0), dict(gain_slew=32769)):
        cfg = pkg.lib.PcmLimitConfig(**dict(good, **kw))
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_limit_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL and not out.value, kw
    for args in ((1, 9, 1), (1, 6, 0), (0, 6, 1), (1, -1, 1)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.PcmLimiter(*args)
        assert e.value.status == pkg.lib.EINVAL
    if not torch.cuda.is_available():
        cfg = pkg.lib.PcmLimitConfig(**good)
        assert lib.sdrfm_pcm_limit_create(C.byref(cfg), C.byref(out)) == pkg.lib.NO_DEVICE and not out.value


def test_null_handles(pkg):
    lib = pkg.load_library()
    one = np.ones(1, np.uint32)
    rec = np.zeros(1, pkg.LIMIT_DTYPE)
    assert lib.sdrfm_pcm_limit_reset(None) == lib.sdrfm_pcm_limit_synchronize(None) == lib.sdrfm_pcm_limit_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_limit_set_params(None, one.ctypes.data, one.ctypes.data) == lib.sdrfm_pcm_limit_set_gain(None, one.ctypes.data, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_limit_get_params(None, None, None) == lib.sdrfm_pcm_limit_get_state(None, rec.ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_limit_read(None, rec.ctypes.data, 0) == pkg.lib.EINVAL and not rec.tobytes().strip(b"\0")
    assert lib.sdrfm_pcm_limit_process_batch(None, None, 0, 0, None, 0, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_limit_kernel_name(None) is None
    lib.sdrfm_pcm_limit_destroy(None)


def test_host_routine_refusals_leave_their_arguments_untouched(pkg):
    lib = pkg.load_library()
    x = np.arange(16, dtype=np.int16)
    good = (29204, 874, 4096, 4096)
    for kw in (dict(log2_window=1), dict(log2_window=9), dict(gain_slew=0), dict(gain_slew=32769), dict(J=65537), dict(params=(0, 874, 4096, 4096)),
               dict(params=(32768, 874, 4096, 4096)), dict(params=(29204, 0, 4096, 4096)), dict(params=(29204, (1 << 23) + 1, 4096, 4096)),
               dict(params=(29204, 874, 65537, 4096)), dict(params=(29204, 874, 4096, 65537)), dict(params=(29204, 874, 4096, 1 << 32))):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.pcm_limit_host(x, **dict(dict(log2_window=2, params=good), **kw))
        assert e.value.status == pkg.lib.EINVAL, kw
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_limit_host(np.zeros(2 * ((1 << 20) + 1), np.int16), 2)
    assert e.value.status == pkg.lib.EINVAL
    # straight through ctypes: the output row, the state and the record stay as they were
    par = np.array([good], pkg.limit.LIMIT_PARAMS_DTYPE)
    bad = np.array([(29204, 874, 4096, 65537)], pkg.limit.LIMIT_PARAMS_DTYPE)
    st, y, rec = pkg.limit.limit_state_init(2), np.full(16, 77, np.int16), np.array([(5, 1, 30000, 2)], pkg.LIMIT_DTYPE)
    st0, rec0 = st.copy(), rec.copy()
    for args in ((None, 8, 2, 1, 0, par.ctypes.data, st.ctypes.data, y.ctypes.data, rec.ctypes.data),
                 (x.ctypes.data, 8, 2, 1, 0, par.ctypes.data, st.ctypes.data, None, rec.ctypes.data),
                 (x.ctypes.data, 8, 2, 1, 0, None, st.ctypes.data, y.ctypes.data, rec.ctypes.data),
                 (x.ctypes.data, 8, 2, 1, 0, par.ctypes.data, None, y.ctypes.data, rec.ctypes.data),
                 (x.ctypes.data, 8, 2, 1, 0, par.ctypes.data, st.ctypes.data, y.ctypes.data, None),
                 (x.ctypes.data, 8, 2, 1, 0, bad.ctypes.data, st.ctypes.data, y.ctypes.data, rec.ctypes.data),
                 (x.ctypes.data, (1 << 20) + 1, 2, 1, 0, par.ctypes.data, st.ctypes.data, y.ctypes.data, rec.ctypes.data)):
        assert lib.sdrfm_pcm_limit_s16(*args) == pkg.lib.EINVAL
        assert np.array_equal(st, st0) and (y == 77).all() and rec.tobytes() == rec0.tobytes()
    assert lib.sdrfm_pcm_limit_add(None, rec.ctypes.data) == lib.sdrfm_pcm_limit_add(rec.ctypes.data, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_limit_check_params(None, 6, 1) == pkg.lib.EINVAL and lib.sdrfm_pcm_limit_check_params(par.ctypes.data, 6, 1) == 0
    assert lib.sdrfm_pcm_limit_state_words(1) == lib.sdrfm_pcm_limit_state_words(9) == 0
    assert [lib.sdrfm_pcm_limit_state_words(lw) for lw in range(2, 9)] == [4 * ((1 << lw) - 1) for lw in range(2, 9)]


def test_join_and_report(pkg):
    a = np.array([(100, 10, 30000, 40)], pkg.LIMIT_DTYPE)
    for b, want in (((50, 5, 30000, 7), (150, 15, 30000, 40)),          # a tie: the earlier place stays
                    ((50, 5, 29999, 7), (150, 15, 29999, 107)),         # strictly smaller: the later one's, moved by the earlier n
                    ((50, 0, 32768, 0), (150, 10, 30000, 40)),
                    ((0, 0, 32768, 0), (100, 10, 30000, 40))):          # the identity
        got = pkg.limit_add(a.copy(), np.array([b], pkg.LIMIT_DTYPE))
        assert tuple(int(v) for v in got[0]) == want
    ident = pkg.limit.limit_identity()
    assert pkg.limit_add(ident.copy(), a).tobytes() == a.tobytes()
    rep = pkg.limit_report(np.array([(48000, 12000, 16384, 24000), (0, 0, 32768, 0), (10, 0, 32768, 0)], pkg.LIMIT_DTYPE))
    assert abs(rep["reduction_db"][0] - 20 * np.log10(2.0)) < 1e-12 and rep["limited_frac"][0] == 0.25 and rep["at_seconds"][0] == 0.5
    assert all(np.isnan(rep[k][1]) for k in rep) and rep["reduction_db"][2] == 0.0 and rep["limited_frac"][2] == 0.0


def test_policies_on_hand_computed_values(pkg):
    assert [pkg.limit_ceiling(d) for d in (-1.0, -2.0, -6.0, 0.0, 3.0, -200.0)] == [29204, 26028, 16422, 32767, 32767, 1]
    assert pkg.limit_ceiling(float("nan")) == 1 and pkg.limit_ceiling(float("-inf")) == 1
    # 2^23 / (0.2 * 48000) = 873.8; 2^23 / 48000 = 174.8; one pair: 2^23
    assert pkg.limit_release(0.2) == 874 and pkg.limit_release(1.0) == 175 and pkg.limit_release(1.0 / 48000) == 1 << 23
    assert pkg.limit_release(0.0) == 1 << 23 and pkg.limit_release(1e9) == 1 and pkg.limit_release(0.2, 44100) == 951
    g = pkg.normalise_gain_q12([-23.0, -29.0, -30.0, -17.0, -60.0, float("-inf"), float("nan"), 40.0])
    # 0 dB; +6 dB: 4096 * 1.99526 = 8172.6; +7 dB: 4096 * 2.23872 = 9169.8; -6 dB: 4096 * 0.501187 = 2052.9; +37 dB limited to +12: 4096 * 3.98107 = 16306.5
    assert g.dtype == np.uint32 and g.tolist() == [4096, 8173, 9170, 2053, 16306, 4096, 4096, 3]
    assert pkg.normalise_gain_q12(-60.0, max_boost_db=40.0).tolist() == [65536]      # x 70.8 clamped to x 16
    assert pkg.normalise_gain_q12(-30.0, target=-16.0, max_boost_db=20.0).tolist() == [20529]   # +14 dB: 4096 * 5.01187 = 20528.6
