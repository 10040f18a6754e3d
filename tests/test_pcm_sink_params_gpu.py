"""Every device form of the PCM sink's recursion — y = fmaf(alpha, x - y, y), pcm = rint(clamp(y * gain)) — held to the host routine across ALPHA and GAIN
(tests/pcm_params.py): the other PCM tests build every sink with alpha = sdrfm_pcm_alpha(48 kHz, 75 us) and the full-scale gain, but the library branches on
alpha (the chain inside design Q's launch serves [0.231f, 1 - 1.8e-5], the sink's own kernel the rest) and builds tables from it ((1 - alpha)^19 squared six
times in the scans; (1 - alpha)^8, its weights and (1 - alpha)^-k in the chain).

  stand-alone sinks   PcmSink and StereoPcmSink, exact and default forms, host buffers, two calls with the states carried, at one chunk of 19 samples and one
                      more, one segment of 4864 and one more, two segments and one more: the exact form bit for bit the host routine (PCM and state), the
                      default form against the exact form's output at the three caps of tests/test_pcm_sink_gpu.py (1 LSB; a share of differing outputs of
                      1e-3 + 2 / size; state within 1e-6 max(|st|, 0.25)), which tests/test_pcm_mono_scan_cpu.py and tests/test_pcm_stereo_scan_cpu.py show to hold by
                      the arithmetic alone; the stereo default form bit for bit two mono sinks.
  the chain           tests/test_pcm_oracle_gpu.py's smallest plan (64 streams, three overlapped calls of 48 000, 48 400 and 96 000 samples) and a mixed one:
                      first which kernels ran ("+ pcm" exactly where sdrfm_sink_chain_tables lets the chain serve), then audio, PCM, canaries, carried state
                      and the chain's error word against the oracle.  The PCM bound is derived (pcm_bound): 1 + ceil(|gain| TOL max(1, max |audio|)).
                      tests/test_pcm_chain_cpu.py runs the same plan's runs through the emulator first.
  the one-call forms  sdrfm_stereo_process_batch_pcm / sdrfm_bcast_process_batch_pcm on host buffers, against a separate handle's L and R and the host
                      routine, within 1 LSB; and one stream with pcm_stride = 0.
Every test prints its worst figures (pytest -s)."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest

import pcm_params as pp
import test_pcm_oracle_gpu as og
import test_pcm_stereo_sink_gpu as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_stereo_scan_emulate")

SHAPES = [(1, 19), (3, 20), (63, 4864), (65, 4865), (2, 9729)]
# every alpha at the default gain, every other gain at the 75 us alpha
PARAMS = [(a, pp.DEFAULT_GAIN) for a in pp.ALPHAS] + [("75us", g) for g in pp.GAINS[1:]]
PARAM_IDS = ["%s-%s" % (a, pp.gain_id(g)) for a, g in PARAMS]


def _pkg():
    return importlib.import_module("stm32f7-rtlsdr_amd")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _two_calls(kind, sink, x, n):
    if kind == "mono":
        return np.concatenate([sink.process_batch(x[:, :n]), sink.process_batch(x[:, n:])], axis=1), sink.state()
    return sg._two_calls(sink, x[0], x[1], n)


@functools.lru_cache(maxsize=None)
def _inputs(kind, ns, n):
    x = emu.mono_inputs(ns, n) if kind == "mono" else emu.sink_inputs(ns, n)
    for a in ([x] if kind == "mono" else x):
        a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _exact(kind, aname, gain, ns, n):
    """the exact form's PCM and states, computed once per (form, alpha, gain, shape): held to the host routine by the exact tests, the reference of the default
    form's (never modified)"""
    pkg = _pkg()
    alpha = pp.alpha_of(pkg.load_library(), aname)
    cls = pkg.PcmSink if kind == "mono" else pkg.StereoPcmSink
    with cls(ns, alpha, gain, exact=True) as sink:
        pcm, st = _two_calls(kind, sink, _inputs(kind, ns, n), n)
    pcm.setflags(write=False)
    st.setflags(write=False)
    return pcm, st


def _host(pkg, kind, alpha, gain, ns, n):
    x = _inputs(kind, ns, n)
    return emu.mono_host_reference(pkg, x, alpha, gain) if kind == "mono" else emu.host_reference(pkg, x[0], x[1], alpha, gain)


# ---- stand-alone sinks -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aname,gain", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_exact_form_is_the_host_routine_bit_for_bit(pkg, kind, aname, gain):
    alpha = pp.alpha_of(pkg.load_library(), aname)
    for ns, n in SHAPES:
        got, st_dev = _exact(kind, aname, gain, ns, n)
        want, st = _host(pkg, kind, alpha, gain, ns, n)
        assert np.array_equal(got, want), (ns, n, np.argwhere(got != want)[:4])
        assert np.array_equal(_bits(st_dev), _bits(st)), (ns, n, st_dev, st)
        if gain == 1e6 and n > 100:
            assert (np.abs(want.astype(np.int32)) >= 32767).mean() > 0.9       # nearly every output clips
        if gain < 0 and n > 100:
            pos, _ = _host(pkg, kind, alpha, -gain, ns, n)                      # mirrored: the negated PCM wherever the positive gain does not clip,
            free = np.abs(pos.astype(np.int32)) < 32767                         # -32768 where it clips high
            assert np.array_equal(want[free], -pos[free]) and (want == -32768).any() and (want[pos == 32767] <= -32767).all()
    print("%s exact, alpha %s = %.9g, gain %g: PCM and state equal the host routine's bit for bit at %s" % (kind, aname, alpha, gain, SHAPES))


@pytest.mark.parametrize("aname,gain", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("kind", ["mono", "stereo"])
def test_default_form_within_the_three_caps_of_the_exact_form(pkg, kind, aname, gain):
    alpha = pp.alpha_of(pkg.load_library(), aname)
    cls = pkg.PcmSink if kind == "mono" else pkg.StereoPcmSink
    worst = [0, 0.0, 0.0]
    fails = []
    for ns, n in SHAPES:
        with cls(ns, alpha, gain) as sink:
            a, sa = _two_calls(kind, sink, _inputs(kind, ns, n), n)
        b, sb = _exact(kind, aname, gain, ns, n)
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        rel = float(np.max(np.abs(sa - sb) / np.maximum(np.abs(sb), 0.25)))
        share = float((d != 0).mean())
        print("%s default, alpha %s, gain %g, %d x %d: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" %
              (kind, aname, gain, ns, n, int(d.max()), share, 1e-3 + 2.0 / d.size, rel))
        worst = [max(worst[0], int(d.max())), max(worst[1], share), max(worst[2], rel)]
        if not (d.max() <= 1 and share <= 1e-3 + 2.0 / d.size and np.all(np.abs(sa - sb) <= 1e-6 * np.maximum(np.abs(sb), 0.25))):
            fails.append((ns, n, int(d.max()), share, rel))
    print("%s default, alpha %s, gain %g: worst PCM %d LSB, share %.3g, state %.3g relative" % (kind, aname, gain, worst[0], worst[1], worst[2]))
    assert not fails, fails


@pytest.mark.parametrize("aname", ["50us", "0.05"])
def test_stereo_default_form_is_two_mono_default_sinks_bit_for_bit(pkg, aname):
    """tests/test_pcm_stereo_sink_gpu.py's test_default_form_is_the_mono_default_sink_channel_by_channel at another alpha and at the edges of a chunk and a segment"""
    alpha = pp.alpha_of(pkg.load_library(), aname)
    for ns, n in SHAPES:
        left, right = _inputs("stereo", ns, n)
        with pkg.StereoPcmSink(ns, alpha, pp.DEFAULT_GAIN) as sink:
            got, st = sg._two_calls(sink, left, right, n)
        for ch, x in enumerate((left, right)):
            with pkg.PcmSink(ns, alpha, pp.DEFAULT_GAIN) as mono:
                want, st_mono = _two_calls("mono", mono, x, n)
            assert np.array_equal(got[:, ch::2], want[:, 0::2]), (ns, n, ch, np.argwhere(got[:, ch::2] != want[:, 0::2])[:4])
            assert np.array_equal(_bits(st[:, ch]), _bits(st_mono)), (ns, n, ch)
        assert not np.array_equal(got[:, 0::2], got[:, 1::2])


# ---- the chain inside the launch ---------------------------------------------------------------------------------------------------------------------------
PLAN = [("pcm", 48000, True, True, "A"), ("pcm", 48400, True, True, "A"), ("pcm", 96000, True, True, "A")]
CHAIN_PARAMS = [(a, pp.DEFAULT_GAIN) for a in pp.ALPHAS] + [("75us", -pp.DEFAULT_GAIN), ("75us", 0.0)]


def _report(what, res, worst):
    print("%s: %s; worst PCM %d LSB (bound %d), worst state difference %.3g" % (what, sorted(set(res.names)), worst, res.lsb, res.worst_state))


@pytest.mark.parametrize("aname,gain", CHAIN_PARAMS, ids=["%s-%s" % (a, pp.gain_id(g)) for a, g in CHAIN_PARAMS])
def test_pcm_call_against_the_oracle_at_every_alpha(pkg, oracle_mod, aname, gain):
    """The run partition changes from call to call (11, 11 and 23 runs: tests/test_pcm_chain_cpu.py); rows that are not 16-byte aligned, canaries behind them.
    alpha >= 0.231f up to 1 - 1.8e-5: "+ pcm" on every call after the stream's first; below 0.231f and at alpha = 1: on none — the sink's own kernel follows
    every (overlapped) launch."""
    lib = pkg.load_library()
    alpha = pp.alpha_of(lib, aname)
    res = og.run_plan(pkg, oracle_mod, PLAN, ns=64, nu=16, astride=1921, pstride=3844, first_id=8400, alpha=alpha, gain=gain)
    chain = aname in pp.CHAIN_ALPHAS
    assert chain == (pp.MIN_ALPHA <= np.float32(alpha) <= np.float32(1 - 1.9e-5))
    og._names_ok(res, overlap=True, chain=chain)
    assert all(nm.startswith("fast-q") for nm in res.names), res.names      # design Q serves every call, with the chain or without
    worst = og.check_plan(res, derived_bound=True)
    assert res.lsb == og.pcm_bound(gain, np.pi) == (1 if gain == 0 else 2)
    _report("alpha %s = %.9g, gain %g" % (aname, alpha, gain), res, worst)


@pytest.mark.parametrize("aname", ["50us", "0.05"])
def test_pcm_call_against_the_oracle_in_a_mixed_launch_at_two_alphas(pkg, oracle_mod, aname):
    """tests/test_pcm_oracle_gpu.py's mixed plan at 64 streams: every 16th stream carries noise and is routed to design B inside design Q's launch.  At 50 us the
    clean streams' PCM is the chain's (k_mix_pcm) and the routed streams' the sink's list kernel's; at 0.05 the sink's own kernel follows for all."""
    alpha = pp.alpha_of(pkg.load_library(), aname)
    ops = [("pcm", 48000, True, True, "A")] * 2 + [("route", (5,))] + [("pcm", 48000, True, True, "A"), ("pcm", 48400, True, True, "A"),
                                                                      ("pcm", 96000, True, True, "A")]
    res = og.run_plan(pkg, oracle_mod, ops, ns=64, nu=16, astride=1921, pstride=3844, noisy_rows=(5,), first_id=8600, alpha=alpha)
    og._names_ok(res, overlap=True, chain=aname in pp.CHAIN_ALPHAS)
    assert all("in one launch" in nm for nm in res.names[2:]), res.names
    worst = og.check_plan(res, derived_bound=True)
    _report("mixed, alpha %s" % aname, res, worst)


# ---- the one-call stereo and broadcast forms ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(kind, ns):
    """a separate handle's plain calls over the first ns stations (the reference of every alpha: computed once)"""
    pkg = _pkg()
    cfg = dict(sg._front(pkg), n_streams=ns)
    if kind == "stereo":
        h = pkg.StereoDemod(pkg.StereoConfig(**cfg))
    else:
        h = pkg.BroadcastDemod(pkg.BroadcastConfig(rds_coeffs=pkg.rds_lowpass_taps(255, sg.FS / sg.D), rds_gain=pkg.rds_gain(sg.D, sg.FS), rds_decim=sg.DR, **cfg))
    with h as ref:
        return tuple(ref.process_batch(sg._chunk(k)[:ns]) for k in range(sg.NCALLS))


def _handle(pkg, kind, ns):
    cfg = dict(sg._front(pkg), n_streams=ns)
    if kind == "stereo":
        return pkg.StereoDemod(pkg.StereoConfig(**cfg))
    return pkg.BroadcastDemod(pkg.BroadcastConfig(rds_coeffs=pkg.rds_lowpass_taps(255, sg.FS / sg.D), rds_gain=pkg.rds_gain(sg.D, sg.FS), rds_decim=sg.DR, **cfg))


def _want_pcm(pkg, plain, ns, alpha, gain):
    na = plain[0][0].shape[1]
    want = [np.zeros((ns, 2 * na), np.int16) for _ in plain]
    want_st = np.zeros((ns, 2), np.float32)
    for s in range(ns):
        st = (0.0, 0.0)
        for k in range(len(plain)):
            want[k][s], st = pkg.pcm_deemph_stereo_s16_host(plain[k][0][s], plain[k][1][s], alpha, gain, st)
        want_st[s] = st
    return want, want_st


@pytest.mark.parametrize("aname,gain", [("50us", pp.DEFAULT_GAIN), ("0.05", pp.DEFAULT_GAIN), ("1", -pp.DEFAULT_GAIN)], ids=["50us", "0.05", "1-mirrored"])
@pytest.mark.parametrize("kind", ["stereo", "bcast"])
def test_one_call_from_iq_to_stereo_pcm_at_other_alphas(pkg, kind, aname, gain):
    """The host form of tests/test_pcm_stereo_sink_gpu.py's test_one_call_from_iq_to_stereo_pcm (4 streams x 3 calls): L and R bit-equal to a separate handle's,
    the PCM within 1 LSB of the host routine over THAT handle's L and R, the states within 1e-6 max(|st|, 0.25)."""
    alpha = pp.alpha_of(pkg.load_library(), aname)
    plain = _plain(kind, sg.NS)
    want, want_st = _want_pcm(pkg, plain, sg.NS, alpha, gain)
    assert max(int(np.abs(w).max()) for w in want) > 1000
    worst = 0
    with _handle(pkg, kind, sg.NS) as dm, pkg.StereoPcmSink(sg.NS, alpha, gain) as sink:
        for k in range(sg.NCALLS):
            r = dm.process_batch_pcm(sink, sg._chunk(k))
            assert np.array_equal(_bits(r[0]), _bits(plain[k][0])) and np.array_equal(_bits(r[1]), _bits(plain[k][1])), k
            d = np.abs(r[2].astype(np.int32) - want[k].astype(np.int32))
            worst = max(worst, int(d.max()))
            assert d.max() <= 1, (k, int(d.max()), np.argwhere(d > 1)[:4])
        st = sink.state()
    rel = float(np.max(np.abs(st - want_st) / np.maximum(np.abs(want_st), 0.25)))
    print("%s one call, alpha %s, gain %g: worst PCM %d LSB, state %.3g relative" % (kind, aname, gain, worst, rel))
    assert rel <= 1e-6, (st, want_st)


@pytest.mark.parametrize("kind", ["stereo", "bcast"])
def test_one_call_for_a_single_stream_takes_a_pcm_stride_of_zero(pkg, kind):
    """include/sdrfm.h: the strides matter 'with more than one stream'.  One stream, pcm_stride = 0, at 50 us: the same references."""
    lib = pkg.load_library()
    alpha, gain = pp.alpha_of(lib, "50us"), pp.DEFAULT_GAIN
    plain = _plain(kind, 1)
    want, want_st = _want_pcm(pkg, plain, 1, alpha, gain)
    na = plain[0][0].shape[1]
    with _handle(pkg, kind, 1) as dm, pkg.StereoPcmSink(1, alpha, gain) as sink:
        for k in range(sg.NCALLS):
            iq = np.ascontiguousarray(sg._chunk(k)[:1])
            left, right = np.zeros((1, na), np.float32), np.zeros((1, na), np.float32)
            pcm = np.full(2 * na + 8, 12345, np.int16)
            pc = np.zeros(1, np.uint32)
            n = C.c_uint32()
            if kind == "stereo":
                rc = lib.sdrfm_stereo_process_batch_pcm(dm._h, sink._h, iq.ctypes.data, iq.shape[1], iq.shape[1], left.ctypes.data, right.ctypes.data, na,
                                                        pcm.ctypes.data, 0, pc.ctypes.data, C.byref(n), 0)
            else:
                nr = plain[k][2].shape[1]
                bb = np.zeros((1, 2 * nr), np.float32)
                n2 = C.c_uint32()
                rc = lib.sdrfm_bcast_process_batch_pcm(dm._h, sink._h, iq.ctypes.data, iq.shape[1], iq.shape[1], left.ctypes.data, right.ctypes.data, na,
                                                       pcm.ctypes.data, 0, bb.ctypes.data, 2 * nr, pc.ctypes.data, C.byref(n), C.byref(n2), 0)
            assert rc == 0 and n.value == na, (k, rc, n.value)
            assert np.array_equal(_bits(left), _bits(plain[k][0])) and np.array_equal(_bits(right), _bits(plain[k][1])), k
            d = np.abs(pcm[:2 * na].astype(np.int32) - want[k][0].astype(np.int32))
            assert d.max() <= 1, (k, int(d.max()))
            assert (pcm[2 * na:] == 12345).all(), k
        st = sink.state()
    assert np.all(np.abs(st - want_st) <= 1e-6 * np.maximum(np.abs(want_st), 0.25)), (st, want_st)
