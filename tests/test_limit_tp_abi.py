"""The C-ABI of the limiter's true-peak form (include/sdrfm.h) without a device: the symbols, that the sample form's set of
declarations is what it was, the sizes, every refusal of the constructor that is made before a device is looked for, NULL handles, and every
refusal of the host routine with nothing touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import limit_tp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_pcm_tplimit_create", "sdrfm_pcm_tplimit_get_detector", "sdrfm_pcm_tplimit_s16", "sdrfm_pcm_tplimit_state_words",
           "sdrfm_pcm_tplimit_state_init", "sdrfm_pcm_tplimit_latency"]


def test_symbols_are_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    text = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(sdrfm_pcm_tplimit_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)
    assert len(set(re.findall(r"\b(sdrfm_pcm_limit_[a-z0-9_]+)\s*\(", src))) == 19                 # the sample form's declarations: none added
    dyn = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and (" T " + sym) in dyn and getattr(lib, sym).argtypes is not None, sym
    assert lib.sdrfm_abi_version() == 1
    for name in ("PcmLimiter", "pcm_limit_tp_host"):
        assert name in pkg.__all__ and hasattr(pkg, name), name


def test_sizes(pkg):
    lib = pkg.load_library()
    for lw in range(0, 11):
        for nt in range(0, 72, 2):
            ok = 2 <= lw <= 8 and 4 <= nt <= 64 and nt % 4 == 0 and (1 << lw) >= nt // 2
            D = (1 << lw) - 1
            assert lib.sdrfm_pcm_tplimit_state_words(lw, nt) == (4 * D + nt if ok else 0), (lw, nt)
            assert lib.sdrfm_pcm_tplimit_latency(lw, nt) == (D + nt // 2 if ok else 0), (lw, nt)
            if ok:
                assert np.array_equal(pkg.limit.limit_tp_state_init(lw, nt)[0], ref.state_init(lw, nt))
            else:
                st = np.full(8, 77, np.int32)
                assert lib.sdrfm_pcm_tplimit_state_init(lw, nt, st.ctypes.data) == pkg.lib.EINVAL and (st == 77).all()
    assert lib.sdrfm_pcm_tplimit_state_init(6, 12, None) == pkg.lib.EINVAL


def test_create_refuses_before_any_device_is_looked_for(pkg):
    """a bad config, table or window: SDRFM_EINVAL with or without a device — on a box without one a legal call answers SDRFM_NO_DEVICE, which
    shows the order"""
    import torch
    lib = pkg.load_library()
    good = dict(n_streams=1, log2_window=6, gain_slew=1, flags=0, device=0)
    tab = np.ascontiguousarray(pkg.truepeak_coef(2, 64))
    over = np.ascontiguousarray(pkg.truepeak_default_coef()).copy()
    over[0, :3] = [32767, 32767, 2]
    cases = [(kw, None, 0, 0) for kw in (dict(n_streams=0), dict(flags=1), dict(log2_window=1), dict(log2_window=9), dict(gain_slew=0),
                                         dict(gain_slew=32769), dict(log2_window=2))]
    cases += [({}, tab, 3, 64), ({}, tab, 2, 62), ({}, tab, 2, 68), ({}, over, 4, 12), (dict(log2_window=4), tab, 2, 64)]
    for kw, coef, P, NT in cases:
        cfg = pkg.lib.PcmLimitConfig(**dict(good, **kw))
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_tplimit_create(C.byref(cfg), None if coef is None else coef.ctypes.data, P, NT, C.byref(out)) == pkg.lib.EINVAL, (kw, P, NT)
        assert not out.value
    cfg = pkg.lib.PcmLimitConfig(**good)
    out = C.c_void_p(1)
    assert lib.sdrfm_pcm_tplimit_create(C.byref(cfg), None, 0, 0, None) == pkg.lib.EINVAL
    assert lib.sdrfm_pcm_tplimit_create(None, None, 0, 0, C.byref(out)) == pkg.lib.EINVAL and not out.value
    for kw in (dict(detect="truepeak", log2_window=2), dict(detect="truepeak", log2_window=4, coef=tab), dict(detect="truepeak", log2_window=9)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.PcmLimiter(1, **kw)
        assert e.value.status == pkg.lib.EINVAL
    with pytest.raises(ValueError):
        pkg.PcmLimiter(1, 6, detect="peak")
    if not torch.cuda.is_available():
        out = C.c_void_p(1)
        assert lib.sdrfm_pcm_tplimit_create(C.byref(cfg), None, 0, 0, C.byref(out)) == pkg.lib.NO_DEVICE and not out.value
        assert lib.sdrfm_pcm_tplimit_create(C.byref(cfg), tab.ctypes.data, 2, 64, C.byref(out)) == pkg.lib.NO_DEVICE and not out.value


def test_null_handle(pkg):
    lib = pkg.load_library()
    v = C.c_uint32(7)
    assert lib.sdrfm_pcm_tplimit_get_detector(None, C.byref(v), C.byref(v), C.byref(v)) == pkg.lib.EINVAL and v.value == 7


def test_host_routine_refusals_leave_their_arguments_untouched(pkg):
    lib = pkg.load_library()
    x = np.arange(16, dtype=np.int16)
    good = (29204, 874, 4096, 4096)
    for kw in (dict(log2_window=1), dict(log2_window=9), dict(log2_window=2), dict(gain_slew=0), dict(gain_slew=32769), dict(J=65537),
               dict(params=(0, 874, 4096, 4096)), dict(params=(32768, 874, 4096, 4096)), dict(params=(29204, 0, 4096, 4096)),
               dict(params=(29204, (1 << 23) + 1, 4096, 4096)), dict(params=(29204, 874, 65537, 4096)), dict(params=(29204, 874, 4096, 65537)),
               dict(coef=np.zeros((3, 12), np.int16)), dict(coef=np.zeros((4, 10), np.int16)), dict(coef=np.full((2, 8), 32767, np.int16)),
               dict(coef=pkg.truepeak_coef(2, 64), log2_window=4)):
        with pytest.raises(pkg.SdrfmError) as e:
            pkg.pcm_limit_tp_host(x, **dict(dict(log2_window=3, params=good), **kw))
        assert e.value.status == pkg.lib.EINVAL, kw
    par = np.array([good], pkg.limit.LIMIT_PARAMS_DTYPE)
    bad = np.array([(29204, 874, 4096, 65537)], pkg.limit.LIMIT_PARAMS_DTYPE)
    tab = np.ascontiguousarray(pkg.truepeak_default_coef())
    over = tab.copy()
    over[3, 6:9] = [32767, -32768, 1]
    st, y, rec = pkg.limit.limit_tp_state_init(3), np.full(16, 77, np.int16), np.array([(5, 1, 30000, 2)], pkg.LIMIT_DTYPE)
    st0, rec0 = st.copy(), rec.copy()
    X, P_, S, Y, R, T = x.ctypes.data, par.ctypes.data, st.ctypes.data, y.ctypes.data, rec.ctypes.data, tab.ctypes.data
    for args in ((None, 8, 3, 1, 0, P_, T, 4, 12, S, Y, R), (X, 8, 3, 1, 0, P_, T, 4, 12, S, None, R), (X, 8, 3, 1, 0, None, T, 4, 12, S, Y, R),
                 (X, 8, 3, 1, 0, P_, T, 4, 12, None, Y, R), (X, 8, 3, 1, 0, P_, T, 4, 12, S, Y, None), (X, 8, 3, 1, 0, bad.ctypes.data, T, 4, 12, S, Y, R),
                 (X, (1 << 20) + 1, 3, 1, 0, P_, T, 4, 12, S, Y, R), (X, 8, 2, 1, 0, P_, T, 4, 12, S, Y, R), (X, 8, 2, 1, 0, P_, None, 0, 0, S, Y, R),
                 (X, 8, 3, 1, 0, P_, T, 3, 12, S, Y, R), (X, 8, 3, 1, 0, P_, T, 4, 10, S, Y, R),
                 (X, 8, 3, 1, 0, P_, over.ctypes.data, 4, 12, S, Y, R)):
        assert lib.sdrfm_pcm_tplimit_s16(*args) == pkg.lib.EINVAL
        assert np.array_equal(st, st0) and (y == 77).all() and rec.tobytes() == rec0.tobytes()
    assert lib.sdrfm_pcm_tplimit_s16(X, 8, 3, 1, 0, P_, T, 4, 12, S, Y, R) == 0 and not (y == 77).all()      # and the same call with nothing wrong
