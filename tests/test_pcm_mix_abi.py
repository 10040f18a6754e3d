"""The PCM mix bus's C-ABI (include/sdrfm.h) without a device: the symbols, the structs' layouts in the header, in ctypes and in
numpy, the constants, every refusal of create (all are made before a device is looked for) and the NULL handles."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_pcm_mix_create", "sdrfm_pcm_mix_destroy", "sdrfm_pcm_mix_reset", "sdrfm_pcm_mix_set_routes", "sdrfm_pcm_mix_set_gains",
           "sdrfm_pcm_mix_get_slots", "sdrfm_pcm_mix_process_batch", "sdrfm_pcm_mix_read", "sdrfm_pcm_mix_set_stream", "sdrfm_pcm_mix_synchronize",
           "sdrfm_pcm_mix_kernel_name", "sdrfm_pcm_mix_s16", "sdrfm_pcm_mix_check_slots", "sdrfm_pcm_mix_check_curve", "sdrfm_pcm_mix_add",
           "sdrfm_pcm_mix_report"]
CONFIG = ("n_in", "n_bus", "n_slots", "slew", "flags", "device")
SLOT = ("src", "mode", "g0", "gt")
RECORD = ("n", "clipped_l", "clipped_r", "peak")
REPORT = ("peak_dbfs", "clipped_frac")
DEFINES = dict(SDRFM_PCM_MIX_SPAN=2048, SDRFM_PCM_MIX_NONE=0xFFFFFFFF, SDRFM_PCM_MIX_CURVE_LEN=129, SDRFM_PCM_MIX_STEREO=0, SDRFM_PCM_MIX_MONO=1,
               SDRFM_PCM_MIX_LEFT=2, SDRFM_PCM_MIX_RIGHT=3, SDRFM_PCM_MIX_SWAP=4)


def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    text = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdrfm_pcm_mix_[a-z0-9_]+)\s*\(", src))
    assert declared == set(SYMBOLS)
    dyn = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and (" T " + sym) in dyn and getattr(lib, sym).argtypes is not None, sym
    assert lib.sdrfm_abi_version() == 1
    for name, value in DEFINES.items():
        m = re.search(r"^#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, text, flags=re.M)
        assert m and int(m.group(1), 0) == value, name
    assert pkg.mix.SPAN == 2048 and pkg.mix.NONE == 0xFFFFFFFF and pkg.mix.MODES == dict(stereo=0, mono=1, left=2, right=3, swap=4)
    for name in ("PcmMixer", "MIX_DTYPE", "MIX_SLOT_DTYPE", "pcm_mix_host", "mix_add", "mix_report", "mix_curve", "slew_for", "fade_pairs",
                 "dead_channel_modes"):
        assert name in pkg.__all__ and hasattr(pkg, name), name


def test_struct_layouts_in_ctypes_and_numpy(pkg):
    cfg, slot, rec, rep = pkg.lib.PcmMixConfig, pkg.lib.PcmMixSlot, pkg.lib.PcmMixRec, pkg.lib.PcmMixReport
    lay = lambda s: [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]
    assert lay(cfg) == [(n, 4 * k, 4) for k, n in enumerate(CONFIG)] and C.sizeof(cfg) == 24
    assert lay(slot) == [(n, 4 * k, 4) for k, n in enumerate(SLOT)] and C.sizeof(slot) == 16
    assert lay(rec) == [(n, 8 * k, 8) for k, n in enumerate(RECORD)] and C.sizeof(rec) == 32
    assert lay(rep) == [(n, 8 * k, 8) for k, n in enumerate(REPORT)] and C.sizeof(rep) == 16
    d, s = pkg.MIX_DTYPE, pkg.MIX_SLOT_DTYPE
    assert d.itemsize == 32 and [(n, d.fields[n][1], d.fields[n][0].str) for n in d.names] == [(n, 8 * k, "<u8") for k, n in enumerate(RECORD)]
    assert s.itemsize == 16 and [(n, s.fields[n][1], s.fields[n][0].str) for n in s.names] == [(n, 4 * k, "<u4") for k, n in enumerate(SLOT)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_in_the_header(tmp_path):
    """the same offsets from the header itself, compiled as C99"""
    fields = [("sdrfm_pcm_mix_config", CONFIG), ("sdrfm_pcm_mix_slot", SLOT), ("sdrfm_pcm_mix_rec", RECORD), ("sdrfm_pcm_mix_report_t", REPORT)]
    args = ", ".join(["offsetof(%s, %s)" % (s, f) for s, fs in fields for f in fs] + ["sizeof(%s)" % s for s, _ in fields] +
                     ["_Alignof(sdrfm_pcm_mix_rec)"])
    count = sum(len(fs) for _, fs in fields) + len(fields) + 1
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdrfm.h"\nint main(void) { printf("%s%%u %%u\\n", %s, (unsigned)SDRFM_PCM_MIX_SPAN, '
                   "(unsigned)SDRFM_PCM_MIX_NONE); return 0; }\n" % ("%zu " * count, args))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True,
                   capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [4 * k for k in range(6)] + [4 * k for k in range(4)] + [8 * k for k in range(4)] + [0, 8] + [24, 16, 32, 16, 8, 2048, 0xFFFFFFFF]


def test_create_refuses_before_any_device_is_looked_for(pkg):
    """a bad config or curve: SDRFM_EINVAL with or without a device — on a box without one a legal config answers SDRFM_NO_DEVICE, which shows
    the order"""
    import torch
    lib = pkg.load_library()
    out = C.c_void_p(1)
    assert lib.sdrfm_pcm_mix_create(None, None, C.byref(out)) == pkg.lib.EINVAL and not out.value
    good = dict(n_in=1, n_bus=1, n_slots=2, slew=32, flags=0, device=0)
    cfg = pkg.lib.PcmMixConfig(**good)
    assert lib.sdrfm_pcm_mix_create(C.byref(cfg), None, None) == pkg.lib.EINVAL
    for kw in (dict(n_in=0), dict(n_in=65537), dict(n_bus=0), dict(n_bus=65537), dict(n_slots=0), dict(n_slots=9), dict(slew=0), dict(slew=32769),
               dict(flags=1), dict(flags=0x80000000), dict(n_in=0xFFFFFFFF)):
        cfg = pkg.lib.PcmMixConfig(**dict(good, **kw))
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_mix_create(C.byref(cfg), None, C.byref(out)) == pkg.lib.EINVAL and not out.value, kw
    cfg = pkg.lib.PcmMixConfig(**good)
    for j, v in ((0, 1), (128, 32767), (50, 0), (127, 40000)):
        bad = pkg.mix_curve("equal_power")
        bad[j] = v
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_mix_create(C.byref(cfg), bad.ctypes.data, C.byref(out)) == pkg.lib.EINVAL and not out.value, (j, v)
    # ... also where the device could not be had either: the refusal is about the config
    cfg = pkg.lib.PcmMixConfig(**dict(good, n_slots=0, device=12345))
    assert lib.sdrfm_pcm_mix_create(C.byref(cfg), None, C.byref(out)) == pkg.lib.EINVAL
    cfg = pkg.lib.PcmMixConfig(**dict(good, device=12345))
    assert lib.sdrfm_pcm_mix_create(C.byref(cfg), None, C.byref(out)) == pkg.lib.NO_DEVICE and not out.value
    cfg = pkg.lib.PcmMixConfig(**dict(good, device=-1))
    assert lib.sdrfm_pcm_mix_create(C.byref(cfg), pkg.mix_curve("linear").ctypes.data, C.byref(out)) == pkg.lib.NO_DEVICE
    if not torch.cuda.is_available():
        cfg = pkg.lib.PcmMixConfig(**dict(good, n_in=65536, n_bus=65536, n_slots=8, slew=32768))   # the largest legal config
        assert lib.sdrfm_pcm_mix_create(C.byref(cfg), None, C.byref(out)) == pkg.lib.NO_DEVICE and not out.value
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.PcmMixer(1, 1)
        assert e.value.status == pkg.lib.NO_DEVICE
    for args in ((0, 1), (1, 0), (1, 1, 0), (1, 1, 9), (1, 1, 2, 0), (-1, 1), (1 << 32, 1)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.PcmMixer(*args)
        assert e.value.status == pkg.lib.EINVAL, args
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.PcmMixer(1, 1, curve=np.zeros(129, np.uint16))
    assert e.value.status == pkg.lib.EINVAL


def test_null_handles(pkg):
    lib = pkg.load_library()
    rec = np.zeros(1, pkg.MIX_DTYPE)
    x, y = np.zeros(4, np.int16), np.full(4, 7, np.int16)
    u = np.zeros(2, np.uint32)
    J = C.c_uint32(9)
    assert lib.sdrfm_pcm_mix_process_batch(None, x.ctypes.data, 4, 2, y.ctypes.data, 4, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_process_batch(None, None, 0, 0, None, 0, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_reset(None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_set_routes(None, u.ctypes.data, u.ctypes.data) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_set_gains(None, u.ctypes.data, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_get_slots(None, None, C.byref(J)) == pkg.lib.EINVAL and J.value == 9
    assert lib.sdrfm_pcm_mix_read(None, rec.ctypes.data, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_synchronize(None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_mix_kernel_name(None) is None
    lib.sdrfm_pcm_mix_destroy(None)                                   # a no-op
    assert not rec.tobytes().strip(b"\0") and (y == 7).all()
