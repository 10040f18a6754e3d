"""The raw-capture IQ meter's C-ABI (include/sdrfm.h) without a device: the symbols, the structs' layouts in the header, in ctypes
and in numpy, the constants, every refusal of create (all are made before a device is looked for) and the NULL handles."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_iq_meter_create", "sdrfm_iq_meter_destroy", "sdrfm_iq_meter_process_batch", "sdrfm_iq_meter_set_stream", "sdrfm_iq_meter_synchronize",
           "sdrfm_iq_meter_kernel_name", "sdrfm_iq_meter_u8", "sdrfm_iq_meter_add", "sdrfm_iq_hist_add", "sdrfm_iq_meter_report", "sdrfm_iq_hist_report"]
RECORD = ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq", "rail_i", "rail_q")
REPORT = ("dc_i", "dc_q", "rms_dbfs", "total_dbfs", "rail_share_i", "rail_share_q", "gain_db", "skew_rad", "image_rejection_db")
HIST_REPORT = ("n", "peak_i", "peak_q", "level999_i", "level999_q", "codes_i", "codes_q", "headroom_db_i", "headroom_db_q")


def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    text = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sdrfm_iq_[a-z0-9_]+)\s*\(", src))
    assert declared == set(SYMBOLS)
    dyn = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and (" T " + sym) in dyn and getattr(lib, sym).argtypes is not None, sym
    assert lib.sdrfm_abi_version() == 1
    bins = re.search(r"^#define\s+SDRFM_IQ_HIST_BINS\s+(\d+)u?\b", text, flags=re.M)
    assert bins and int(bins.group(1)) == pkg.IQ_HIST_BINS == 512
    for name in ("IqMeter", "IQ_METER_DTYPE", "iq_meter_host", "iq_meter_add", "iq_hist_add", "iq_meter_report", "iq_hist_report", "gain_advice", "nearest_gain",
                 "impair_iq"):
        assert name in pkg.__all__ and hasattr(pkg, name), name


def test_struct_layouts_in_ctypes_and_numpy(pkg):
    cfg, rec, rep, hrep = pkg.lib.IqMeterConfig, pkg.lib.IqMeter, pkg.lib.IqReport, pkg.lib.IqHistReport
    lay = lambda s: [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]
    assert lay(cfg) == [("struct_size", 0, 4), ("n_streams", 4, 4), ("max_bytes_per_call", 8, 4), ("device", 12, 4), ("flags", 16, 4)] and C.sizeof(cfg) == 20
    assert lay(rec) == [(n, 8 * k, 8) for k, n in enumerate(RECORD)] and C.sizeof(rec) == 64
    assert lay(rep) == [(n, 8 * k, 8) for k, n in enumerate(REPORT)] and C.sizeof(rep) == 72
    assert lay(hrep) == [(n, 8 * k, 8) for k, n in enumerate(HIST_REPORT)] and C.sizeof(hrep) == 72
    d = pkg.IQ_METER_DTYPE
    assert d.itemsize == 64 and [(n, d.fields[n][1], d.fields[n][0].str) for n in d.names] == [(n, 8 * k, "<u8") for k, n in enumerate(RECORD)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layouts_in_the_header(tmp_path):
    """the same offsets from the header itself, compiled as C99"""
    fields = [("sdrfm_iq_meter_config", ("struct_size", "n_streams", "max_bytes_per_call", "device", "flags")), ("sdrfm_iq_meter", RECORD),
              ("sdrfm_iq_report_t", REPORT), ("sdrfm_iq_hist_report_t", HIST_REPORT)]
    args = ", ".join(["offsetof(%s, %s)" % (s, f) for s, fs in fields for f in fs] + ["sizeof(%s)" % s for s, _ in fields])
    count = sum(len(fs) for _, fs in fields) + len(fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdrfm.h"\nint main(void) { printf("%s%%u %%u\\n", %s, (unsigned)SDRFM_IQ_HIST_BINS, '
                   "(unsigned)SDRFM_IQ_MAX_BYTES); return 0; }\n" % ("%zu " * count, args))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True,
                   capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [0, 4, 8, 12, 16] + [8 * k for k in range(8)] + [8 * k for k in range(9)] + [8 * k for k in range(9)] + [20, 64, 72, 72, 512, 64 << 20]


def test_create_refuses_before_any_device_is_looked_for(pkg):
    """a bad config: SDRFM_EINVAL with or without a device — on a box without one a legal config answers SDRFM_NO_DEVICE, which shows the order"""
    import torch
    lib = pkg.load_library()
    out = C.c_void_p(1)
    assert lib.sdrfm_iq_meter_create(None, C.byref(out)) == pkg.lib.EINVAL and not out.value
    good = dict(struct_size=C.sizeof(pkg.lib.IqMeterConfig), n_streams=1, max_bytes_per_call=0, device=0, flags=0)
    cfg = pkg.lib.IqMeterConfig(**good)
    assert lib.sdrfm_iq_meter_create(C.byref(cfg), None) == pkg.lib.EINVAL
    for kw in (dict(struct_size=0), dict(struct_size=24), dict(n_streams=0), dict(n_streams=65537), dict(max_bytes_per_call=(64 << 20) + 1),
               dict(max_bytes_per_call=0xFFFFFFFF), dict(flags=1), dict(flags=0x80000000)):
        cfg = pkg.lib.IqMeterConfig(**dict(good, **kw))
        out = C.c_void_p(1)
        assert lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL and not out.value, kw
    # ... also where the device could not be had either: the refusal is about the config
    cfg = pkg.lib.IqMeterConfig(**dict(good, n_streams=0, device=12345))
    assert lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(out)) == pkg.lib.EINVAL
    cfg = pkg.lib.IqMeterConfig(**dict(good, device=12345))
    assert lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(out)) == pkg.lib.NO_DEVICE and not out.value
    cfg = pkg.lib.IqMeterConfig(**dict(good, device=-1))
    assert lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(out)) == pkg.lib.NO_DEVICE
    if not torch.cuda.is_available():
        cfg = pkg.lib.IqMeterConfig(**dict(good, max_bytes_per_call=64 << 20, n_streams=65536))   # the largest legal config
        assert lib.sdrfm_iq_meter_create(C.byref(cfg), C.byref(out)) == pkg.lib.NO_DEVICE and not out.value
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.IqMeter(1)
        assert e.value.status == pkg.lib.NO_DEVICE
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.IqMeter(0)
    assert e.value.status == pkg.lib.EINVAL


def test_null_handles(pkg):
    lib = pkg.load_library()
    rec = np.zeros(1, pkg.IQ_METER_DTYPE)
    x = np.zeros(4, np.uint8)
    assert lib.sdrfm_iq_meter_process_batch(None, x.ctypes.data, 4, 4, rec.ctypes.data, None, 0) == pkg.lib.EINVAL
    assert lib.sdrfm_iq_meter_process_batch(None, None, 0, 0, None, None, 3) == pkg.lib.EINVAL
    assert lib.sdrfm_iq_meter_set_stream(None, None) == pkg.lib.EINVAL
    assert lib.sdrfm_iq_meter_synchronize(None) == pkg.lib.EINVAL
    assert lib.sdrfm_iq_meter_kernel_name(None) == b""
    lib.sdrfm_iq_meter_destroy(None)                                  # a no-op
    assert not rec.tobytes().strip(b"\0")
