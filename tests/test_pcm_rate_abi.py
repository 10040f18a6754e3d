"""The PCM rate matcher's C-ABI (include/sdrfm.h) without a device: the symbols, the config struct's layout in the header and in
ctypes, the ABI version, and every refusal that is made before a device is looked for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_pcm_rate_create", "sdrfm_pcm_rate_destroy", "sdrfm_pcm_rate_reset", "sdrfm_pcm_rate_set_step", "sdrfm_pcm_rate_count",
           "sdrfm_pcm_rate_process_batch", "sdrfm_pcm_rate_get_state", "sdrfm_pcm_rate_set_stream", "sdrfm_pcm_rate_synchronize",
           "sdrfm_pcm_rate_kernel_name", "sdrfm_pcm_rate_s16", "sdrfm_pcm_rate_check_coef"]


def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrfm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sdrfm_pcm_rate_[a-z0-9_]+)\s*\(", src))
    assert declared == set(SYMBOLS)
    dyn = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and (" T " + sym) in dyn and getattr(lib, sym).argtypes is not None, sym
    assert lib.sdrfm_abi_version() == 1
    assert re.search(r"^#define\s+SDRFM_ABI_VERSION\s+1u?\s*$", open(os.path.join(ROOT, "include", "sdrfm.h")).read(), flags=re.M)


def test_config_layout_in_ctypes(pkg):
    cfg = pkg.lib.PcmRateConfig
    assert [(n, getattr(cfg, n).offset, getattr(cfg, n).size) for n, _ in cfg._fields_] == [
        ("n_streams", 0, 4), ("n_taps", 4, 4), ("log2_phases", 8, 4), ("flags", 12, 4), ("coef", 16, 8), ("device", 24, 4)]
    assert C.sizeof(cfg) == 32


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_config_layout_in_the_header(tmp_path):
    """the same offsets from the header itself, compiled as C99"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdrfm.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %u\\n", '
                   "offsetof(sdrfm_pcm_rate_config, n_streams), offsetof(sdrfm_pcm_rate_config, n_taps), offsetof(sdrfm_pcm_rate_config, log2_phases), "
                   "offsetof(sdrfm_pcm_rate_config, flags), offsetof(sdrfm_pcm_rate_config, coef), offsetof(sdrfm_pcm_rate_config, device), "
                   "sizeof(sdrfm_pcm_rate_config), (unsigned)SDRFM_ABI_VERSION); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True,
                   capture_output=True, text=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["0", "4", "8", "12", "16", "24", "32", "1"]


def _cfg(pkg, coef, n_streams=1, nt=None, logph=None, flags=0):
    c = np.ascontiguousarray(coef, np.int16)
    return pkg.lib.PcmRateConfig(n_streams, c.shape[1] if nt is None else nt, (c.shape[0] - 1).bit_length() - 1 if logph is None else logph, flags,
                                 c.ctypes.data_as(C.POINTER(C.c_int16)), 0), c


def test_create_refuses_before_any_device_is_looked_for(pkg):
    """bad config and a table over the bound: SDRFM_EINVAL with or without a device — on a box without one a legal config answers SDRFM_NO_DEVICE,
    which shows the order"""
    import torch
    lib = pkg.load_library()
    out = C.c_void_p(1)
    good = pkg.rate_coef(32, 8, 0.9)
    assert lib.sdrfm_pcm_rate_create(None, C.byref(out)) == pkg.lib.EINVAL and not out.value
    cfg, keep = _cfg(pkg, good)
    assert lib.sdrfm_pcm_rate_create(C.byref(cfg), None) == pkg.lib.EINVAL
    for kw in (dict(n_streams=0), dict(flags=1), dict(nt=0), dict(nt=30), dict(nt=68), dict(logph=3), dict(logph=9)):
        cfg, keep = _cfg(pkg, np.zeros((513, 68), np.int16), **dict(dict(nt=32, logph=8), **kw))
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_rate_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL and not out.value, kw
    cfg, keep = _cfg(pkg, good)
    cfg.coef = None
    assert lib.sdrfm_pcm_rate_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL
    over = good.copy()
    over[200, :16] = 4096                                              # 65536 in one half of one row
    cfg, keep = _cfg(pkg, over)
    assert lib.sdrfm_pcm_rate_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL and not out.value
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.PcmRateMatcher(1, over)
    assert e.value.status == pkg.lib.EINVAL
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.PcmRateMatcher(1, np.zeros((256, 32), np.int16))           # no 2^LOGPH + 1 rows
    assert e.value.status == pkg.lib.EINVAL
    if not torch.cuda.is_available():
        cfg, keep = _cfg(pkg, good)
        assert lib.sdrfm_pcm_rate_create(C.byref(cfg), C.byref(out)) == pkg.lib.NO_DEVICE and not out.value


def test_null_handles(pkg):
    lib = pkg.load_library()
    n = C.c_uint32()
    assert lib.sdrfm_pcm_rate_reset(None) == lib.sdrfm_pcm_rate_synchronize(None) == lib.sdrfm_pcm_rate_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_rate_set_step(None, None) == lib.sdrfm_pcm_rate_get_state(None, None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_rate_count(None, 1, None, C.byref(n)) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_rate_process_batch(None, None, 0, 0, None, 0, None, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_rate_kernel_name(None) is None
    lib.sdrfm_pcm_rate_destroy(None)


def test_host_routine_refusals_through_the_library(pkg):
    coef = pkg.rate_coef(32, 8, 0.9)
    x = np.zeros(64, np.int16)
    for step in (0, (1 << 30) - 1, (1 << 34) + 1, (1 << 64) - 1):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.pcm_rate_host(x, coef, step)
        assert e.value.status == pkg.lib.EINVAL, step
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_rate_host(np.zeros(2 * ((1 << 20) + 1), np.int16), coef, 1 << 32)
    assert e.value.status == pkg.lib.EINVAL
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_rate_host(x, np.zeros((17, 6), np.int16), 1 << 32)
    assert e.value.status == pkg.lib.EINVAL
