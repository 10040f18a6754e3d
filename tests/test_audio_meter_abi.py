"""CPU checks of the audio meter's C-ABI (include/sdrfm.h): the six symbols exported, declared and listed, the record's layout
in the header, in ctypes and in numpy, the free flag bit, and every refusal that needs no device.  (Those that need a sink are
tests/test_pcm_audio_meter_gpu.py's.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrfm_pcm_audio_meter_s16", "sdrfm_audio_meter_add", "sdrfm_audio_meter_report", "sdrfm_pcm_stereo_sink_meter_enable",
         "sdrfm_pcm_stereo_sink_meter_disable", "sdrfm_pcm_stereo_sink_meter_read"]


def _header():
    with open(os.path.join(ROOT, "include", "sdrfm.h")) as fh:
        return fh.read()


def test_symbols_are_exported_declared_and_listed(pkg):
    lib, header = pkg.load_library(), _header()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in pkg.ABI_SYMBOLS, n
        assert re.search(r"^int\s+%s\(" % n, header, re.M), n
    assert len(set(pkg.ABI_SYMBOLS)) == len(pkg.ABI_SYMBOLS)
    assert re.search(r"^#define SDRFM_ABI_VERSION\s+1u?\b", header, re.M) and lib.sdrfm_abi_version() == 1
    for m in ("enable_meter", "disable_meter", "read_meters"):
        assert callable(getattr(pkg.StereoPcmSink, m)), m
    for f in ("pcm_audio_meter_host", "audio_meter_add", "audio_meter_report", "audio_alarms", "AudioMonitor", "AUDIO_METER_DTYPE"):
        assert hasattr(pkg, f) and f in pkg.__all__, f
    # the header states the order of the join and the bound of exactness
    assert "ASSOCIATIVE AND NOT COMMUTATIVE" in header and "EXACT WHILE THE ACCUMULATED n <= 2^32" in header


def test_record_layout(pkg):
    L = pkg.lib
    assert C.sizeof(L.AudioRuns) == 32 and C.sizeof(L.AudioMeter) == 192 and C.alignment(L.AudioMeter) == 8
    assert L.AUDIO_METER_DTYPE.itemsize == 192
    for name, _ in L.AudioMeter._fields_:
        assert getattr(L.AudioMeter, name).offset == L.AUDIO_METER_DTYPE.fields[name][1], name
    assert [n for n, _ in L.AudioMeter._fields_] == list(L.AUDIO_METER_DTYPE.names)
    # the header's struct, field by field in its order
    body = re.search(r"typedef struct sdrfm_audio_meter \{(.*?)\} sdrfm_audio_meter;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(L.AUDIO_METER_DTYPE.names), names
    assert C.sizeof(L.AudioReport) == 8 * 21
    rep = re.search(r"typedef struct sdrfm_audio_report_t \{(.*?)\} sdrfm_audio_report_t;", _header(), re.S).group(1)
    assert [n.strip() for decl in rep.split(";") if decl.strip() for n in decl.replace("double", "").split(",")] == [n for n, _ in L.AudioReport._fields_]


def test_reset_flag_is_a_free_bit(pkg):
    header = _header()
    flags = {n: int(v) for n, v in re.findall(r"^#define (SDRFM_F_DEVICE_PTRS|SDRFM_F_OVERLAP|SDRFM_PCM_F_EXACT|SDRFM_AMETER_F_RESET) (\d+)u", header, re.M)}
    assert len(flags) == 4 and flags["SDRFM_AMETER_F_RESET"] == pkg.lib.AMETER_F_RESET == 8
    assert sorted(flags.values()) == [1, 2, 4, 8]


def test_refusals_that_need_no_device(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    rec = np.zeros(2, pkg.AUDIO_METER_DTYPE)
    rec["n"] = 77
    before = rec.tobytes()
    pcm = np.array([1, -1, 2, -2], np.int16)
    assert lib.sdrfm_pcm_audio_meter_s16(pcm.ctypes.data, 2, 0, None) == E
    assert lib.sdrfm_pcm_audio_meter_s16(None, 2, 0, rec.ctypes.data) == E
    assert lib.sdrfm_pcm_audio_meter_s16(pcm.ctypes.data, 2, 32768, rec.ctypes.data) == E
    assert lib.sdrfm_pcm_audio_meter_s16(pcm.ctypes.data, 2, 0xFFFFFFFF, rec.ctypes.data) == E
    assert lib.sdrfm_pcm_audio_meter_s16(None, 0, 32767, rec.ctypes.data) == 0
    assert lib.sdrfm_audio_meter_add(None, rec.ctypes.data) == E and lib.sdrfm_audio_meter_add(rec.ctypes.data, None) == E
    r = pkg.lib.AudioReport()
    assert lib.sdrfm_audio_meter_report(None, 48000.0, C.byref(r)) == E and lib.sdrfm_audio_meter_report(rec.ctypes.data, 48000.0, None) == E
    for bad in (0.0, -48000.0, float("nan"), float("inf")):
        assert lib.sdrfm_audio_meter_report(rec.ctypes.data, bad, C.byref(r)) == E
    # a NULL sink, and a threshold no int16 magnitude reaches: before any device is looked for
    assert lib.sdrfm_pcm_stereo_sink_meter_enable(None, 0) == E and lib.sdrfm_pcm_stereo_sink_meter_enable(None, 40000) == E
    assert lib.sdrfm_pcm_stereo_sink_meter_disable(None) == E
    for flags in (0, 1, 8, 9, 2):
        assert lib.sdrfm_pcm_stereo_sink_meter_read(None, rec.ctypes.data, flags) == E
    assert rec.tobytes() == before
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_audio_meter_host(pcm, 32768)
    assert e.value.status == E
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.pcm_audio_meter_host(pcm, -1)
    assert e.value.status == E
