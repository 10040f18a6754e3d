"""Device-side STEREO PCM sink (csrc/sdrfm_sink_stereo.hip) and the one-call forms sdrfm_stereo_process_batch_pcm / sdrfm_bcast_process_batch_pcm:
the exact form (SDRFM_PCM_F_EXACT) against the host routine sdrfm_pcm_deemph_stereo_s16 and an exact-rational restatement, bit for bit; the default form
(the blocked scan, two chains in a lane) held to the exact one by the mono sink's three bounds (tests/test_pcm_sink_gpu.py) and to the mono default sink,
channel by channel, bit for bit.  The inputs are tools/pcm_stereo_scan_emulate.py's, on which tests/test_pcm_stereo_scan_cpu.py shows the bounds by the
arithmetic alone."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_stereo_scan_emulate")

FS, D, DA, DR = 2.4e6, 10, 5, 25


def _params(pkg):
    lib = pkg.load_library()
    return lib.sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _two_calls(sink, left, right, n):
    """two calls of n samples on host buffers (the states are carried): (pcm [ns, 4n], state [ns, 2])"""
    a = sink.process_batch(left[:, :n], right[:, :n])
    b = sink.process_batch(left[:, n:], right[:, n:])
    return np.concatenate([a, b], axis=1), sink.state()


@functools.lru_cache(maxsize=None)
def _exact(ns, n):
    """the exact form's PCM and states on the shape's inputs, computed once: the reference of the default form's tests (never modified)"""
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(ns, n)
    with pkg.StereoPcmSink(ns, alpha, gain, exact=True) as sink:
        pcm, st = _two_calls(sink, left, right, n)
    pcm.setflags(write=False)
    st.setflags(write=False)
    return pcm, st


@pytest.mark.parametrize("ns,n", [(1, 4800), (3, 1), (64, 63), (65, 130)])
def test_exact_form_equals_the_host_routine_bitwise(pkg, ns, n):
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(ns, n)
    got, st_dev = _exact(ns, n)
    want, st = emu.host_reference(pkg, left, right, alpha, gain)
    for s in range(ns):
        assert np.array_equal(got[s], want[s]), (s, int(np.argmax(got[s] != want[s])))
    assert np.array_equal(_bits(st_dev), _bits(st)), (st_dev, st)
    if 2 * n >= 6:
        assert want[0, 0::2].max() == 32767 and want[0, 1::2].min() == -32768              # both channels saturate


def test_exact_form_against_the_exact_rational_definition(pkg):
    """Per channel against the INDEPENDENT restatement of tests/test_pcm_sink.py (exact rationals, correctly rounded at every operation): saturation,
    ties and tiny values in both channels, the states carried across two calls."""
    from test_pcm_sink import pcm_reference
    alpha, gain = _params(pkg)
    rng = np.random.default_rng(7)
    ns, n = 3, 48
    left = (rng.standard_normal((ns, 2 * n)) * 1.5).astype(np.float32)
    right = (rng.standard_normal((ns, 2 * n)) * 1.5).astype(np.float32)
    left[0, :8] = [10.0, 10.0, -10.0, -10.0, 0.0, 1e-30, -1e-30, 0.5 / 3.0]
    right[0, :8] = -left[0, :8]
    left[1, :4] = [np.float32(0.5) / gain, np.float32(1.5) / gain, np.float32(-2.5) / gain, 0.0]
    right[2, :4] = left[1, :4]
    with pkg.StereoPcmSink(ns, alpha, gain, exact=True) as sink:
        got, st_dev = _two_calls(sink, left, right, n)
    for s in range(ns):
        for ch, x in enumerate((left, right)):
            want, y_end = pcm_reference(x[s], alpha, gain, 0.0)
            assert np.array_equal(got[s, ch::2], want[0::2]), (s, ch, int(np.argmax(got[s, ch::2] != want[0::2])))
            assert np.float32(y_end).view(np.uint32) == st_dev[s, ch].view(np.uint32), (s, ch)


@pytest.mark.parametrize("ns,n", [(1, 4800), (3, 1), (5, 255), (64, 257), (65, 1300), (2, 30000), (256, 4800)])
def test_default_form_within_one_lsb_of_the_exact_form(pkg, ns, n):
    """Lengths below, at and above the 256 chunks and above one LDS segment (4864); the mono sink's bounds."""
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(ns, n)
    with pkg.StereoPcmSink(ns, alpha, gain) as sink:
        a, sa = _two_calls(sink, left, right, n)
    b, sb = _exact(ns, n)
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    print("%d x %d: max |PCM difference| %d, share %.3g, worst state difference %.3g" % (ns, n, int(d.max()), float((d != 0).mean()), float(np.abs(sa - sb).max())))
    assert d.max() <= 1, (int(d.max()), np.argwhere(d > 1)[:4])
    assert (d != 0).mean() <= 1e-3 + 2.0 / d.size, float((d != 0).mean())
    assert np.all(np.abs(sa - sb) <= 1e-6 * np.maximum(np.abs(sb), 0.25)), (sa, sb)


@pytest.mark.parametrize("ns,n", [(5, 255), (65, 1300), (2, 30000)])
def test_default_form_is_the_mono_default_sink_channel_by_channel(pkg, ns, n):
    """Even slots: a mono PcmSink over the L rows; odd slots: another over the R rows; the states likewise.  Bit for bit: per channel the operations are
    k_pcm_sink_scan<false>'s.  A swapped channel, a carry shared between the channels or a wrong pack cannot pass."""
    alpha, gain = _params(pkg)
    left, right = emu.sink_inputs(ns, n)
    with pkg.StereoPcmSink(ns, alpha, gain) as sink:
        got, st = _two_calls(sink, left, right, n)
    for ch, x in enumerate((left, right)):
        with pkg.PcmSink(ns, alpha, gain) as mono:
            want = np.concatenate([mono.process_batch(x[:, :n]), mono.process_batch(x[:, n:])], axis=1)
            st_mono = mono.state()
        assert np.array_equal(got[:, ch::2], want[:, 0::2]), (ch, np.argwhere(got[:, ch::2] != want[:, 0::2])[:4])
        assert np.array_equal(_bits(st[:, ch]), _bits(st_mono)), (ch, st[:, ch], st_mono)
    assert not np.array_equal(got[:, 0::2], got[:, 1::2])


@pytest.mark.parametrize("exact", [False, True])
def test_device_pointer_form_with_padded_rows_and_refusals(pkg, exact):
    """audio_stride > n, pcm_stride > 2n, a canary behind every row's 2n PCM words; the refusals of the header, each leaving the states alone: the valid
    calls around them give what the host-buffer calls give."""
    import torch
    alpha, gain = _params(pkg)
    lib = pkg.load_library()
    EINVAL, ECAP = pkg.lib.EINVAL, pkg.lib.ECAPACITY
    ns, n, astride, pstride = 5, 255, 300, 2 * 255 + 6
    left, right = emu.sink_inputs(ns, n)
    want, want_st = _exact(ns, n) if exact else (None, None)
    if not exact:
        with pkg.StereoPcmSink(ns, alpha, gain) as ref:
            want, want_st = _two_calls(ref, left, right, n)
    dl = [torch.zeros((ns, astride), dtype=torch.float32, device="cuda") for _ in range(2)]
    dr = [torch.zeros((ns, astride), dtype=torch.float32, device="cuda") for _ in range(2)]
    for k in range(2):
        dl[k][:, :n] = torch.from_numpy(left[:, k * n:(k + 1) * n])
        dr[k][:, :n] = torch.from_numpy(right[:, k * n:(k + 1) * n])
    pcm = [torch.full((ns, pstride), 12345, dtype=torch.int16, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with pkg.StereoPcmSink(ns, alpha, gain, exact=exact) as sink:
        sink.process_batch_device(dl[0], dr[0], pcm[0], n)
        fl = pkg.lib.F_DEVICE_PTRS | (4 if exact else 0)
        lp, rp, pp = (C.c_void_p(t.data_ptr()) for t in (dl[1], dr[1], pcm[1]))
        call = lambda l, r, a_s, nn, p, p_s, f: lib.sdrfm_pcm_stereo_sink_process_batch(sink._h, l, r, a_s, nn, p, p_s, f)
        assert call(lp, rp, astride, n, pp, pstride, fl | 8) == EINVAL                     # an unknown flag
        assert call(lp, rp, astride, n, pp, pstride, fl | 2) == EINVAL                     # SDRFM_F_OVERLAP is not the sink's
        assert call(None, None, 0, 0, None, 0, fl) == 0                                    # n == 0: a no-op
        assert call(None, rp, astride, n, pp, pstride, fl) == EINVAL
        assert call(lp, None, astride, n, pp, pstride, fl) == EINVAL
        assert call(lp, rp, astride, n, None, pstride, fl) == EINVAL
        assert call(lp, rp, n - 1, n, pp, pstride, fl) == ECAP
        assert call(lp, rp, astride, n, pp, 2 * n - 2, fl) == ECAP
        assert call(lp, rp, astride, n, pp, pstride + 1, fl) == EINVAL                     # rows are written as (L, R) dwords
        assert call(lp, rp, astride, n, C.c_void_p(pcm[1].data_ptr() + 2), pstride, fl) == EINVAL
        sink.process_batch_device(dl[1], dr[1], pcm[1], n)
        sink.synchronize()
        st = sink.state()
    got = [p.cpu().numpy() for p in pcm]
    for k in range(2):
        assert np.array_equal(got[k][:, :2 * n], want[:, 2 * k * n:2 * (k + 1) * n]), k
        assert (got[k][:, 2 * n:] == 12345).all(), k                                       # nothing written past a row's samples
    assert np.array_equal(_bits(st), _bits(want_st))


def test_reset_makes_the_next_call_a_fresh_sinks(pkg):
    alpha, gain = _params(pkg)
    ns, n = 5, 255
    left, right = emu.sink_inputs(ns, n)
    with pkg.StereoPcmSink(ns, alpha, gain) as fresh:
        want = fresh.process_batch(left[:, n:], right[:, n:])
        want_st = fresh.state()
    with pkg.StereoPcmSink(ns, alpha, gain) as sink:
        sink.process_batch(left[:, :n], right[:, :n])
        assert np.abs(sink.state()).max() > 0
        sink.reset()
        assert not sink.state().any()
        got = sink.process_batch(left[:, n:], right[:, n:])
        assert np.array_equal(got, want) and np.array_equal(_bits(sink.state()), _bits(want_st))
        assert sink.process_batch(np.zeros((ns, 0), np.float32), np.zeros((ns, 0), np.float32)).shape == (ns, 0)


# ---- one call from IQ to PCM -------------------------------------------------------------------------------------------------------------------------
NS, NBYTES, NCALLS = 4, 48000, 3


def _front(pkg):
    return dict(fir_coeffs=pkg.lowpass_taps(64, 120e3 / FS), pilot_coeffs=pkg.stereo_pilot_taps(101, FS / D), audio_coeffs=pkg.lowpass_taps(32, 15e3 / (FS / D)),
                diff_gain=pkg.stereo_diff_gain(D, FS), pilot_min=0.05, fir_decim=D, audio_decim=DA, n_streams=NS, max_bytes_per_call=NBYTES)


def _handle(pkg, kind, generic):
    if kind == "stereo":
        return pkg.StereoDemod(pkg.StereoConfig(force_generic=generic, **_front(pkg)))
    return pkg.BroadcastDemod(pkg.BroadcastConfig(rds_coeffs=pkg.rds_lowpass_taps(255, FS / D), rds_gain=pkg.rds_gain(D, FS), rds_decim=DR, force_generic=generic,
                                                  **_front(pkg)))


@functools.lru_cache(maxsize=None)
def _stations():
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    nsamp = NCALLS * NBYTES // 2
    iq = np.stack([pkg.make_iq_rds(1, nsamp, pkg.rds_encode_groups(0x4000 + s, "SINK %03d" % s), rds_phase=0.5 * s, first_id=5200 + s)[0] for s in range(NS)])
    iq.setflags(write=False)
    return iq


def _chunk(k):
    return np.ascontiguousarray(_stations()[:, k * NBYTES:(k + 1) * NBYTES])


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "force_generic"])
@pytest.mark.parametrize("kind", ["stereo", "bcast"])
def test_one_call_from_iq_to_stereo_pcm(pkg, kind, generic):
    """Three calls of 48 000 B per stream.  L, R (bb, pilot_count) bit-equal to a SEPARATE handle making the plain call; the PCM within 1 LSB of the host
    routine over THAT handle's L and R with the states carried (never against the same launch's own audio); bit-equal to the two-call sequence (the plain
    call, then StereoPcmSink.process_batch_device on the same stream) and to the form without audio rows; in host and device forms.  A sink of another stream
    count and half-NULL audio are refused and change nothing: the calls behind the refusals match the same references."""
    import torch
    alpha, gain = _params(pkg)
    lib = pkg.load_library()
    bc = kind == "bcast"
    # the references: a separate handle's plain calls, the host routine over their audio
    plain = []
    with _handle(pkg, kind, generic) as ref:
        assert ("generic" in ref.kernel_name) == generic, ref.kernel_name
        for k in range(NCALLS):
            plain.append(ref.process_batch(_chunk(k)))
    na = plain[0][0].shape[1]
    assert na == NBYTES // 2 // D // DA
    want_pcm = [np.zeros((NS, 2 * na), np.int16) for _ in range(NCALLS)]
    want_st = np.zeros((NS, 2), np.float32)
    for s in range(NS):
        st = (0.0, 0.0)
        for k in range(NCALLS):
            want_pcm[k][s], st = pkg.pcm_deemph_stereo_s16_host(plain[k][0][s], plain[k][1][s], alpha, gain, st)
        want_st[s] = st
    assert max(int(np.abs(w).max()) for w in want_pcm) > 1000                               # (audible programme, not silence)

    def check(tag, k, out, pcm):
        """out: the plain call's tuple as the one-call form gave it (L, R[, bb], pc); None entries are not compared"""
        for got, want in zip(out, plain[k]):
            if got is not None:
                w = want.view(np.float32) if want.dtype == np.complex64 else want
                g = got.view(np.float32) if got.dtype == np.complex64 else got
                assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (tag, k)
        d = np.abs(pcm.astype(np.int32) - want_pcm[k].astype(np.int32))
        assert d.max() <= 1, (tag, k, int(d.max()))

    def check_state(tag, sink):
        st = sink.state()
        assert np.all(np.abs(st - want_st) <= 1e-6 * np.maximum(np.abs(want_st), 0.25)), (tag, st, want_st)

    # host form
    host_pcm = []
    with _handle(pkg, kind, generic) as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
        for k in range(NCALLS):
            r = dm.process_batch_pcm(sink, _chunk(k))
            out = (r[0], r[1], r[3], r[4]) if bc else (r[0], r[1], r[3])
            check("host", k, out, r[2])
            host_pcm.append(r[2].copy())
        check_state("host", sink)
    # host form without audio rows
    with _handle(pkg, kind, generic) as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
        for k in range(NCALLS):
            r = dm.process_batch_pcm(sink, _chunk(k), with_audio=False)
            assert r[0] is None and r[1] is None
            assert np.array_equal(r[2], host_pcm[k]), ("host, no audio rows", k)
            assert np.array_equal(r[-1], plain[k][-1])
    # device forms
    iq = [torch.from_numpy(_chunk(k)).cuda() for k in range(NCALLS)]
    nr = plain[0][2].shape[1] if bc else 0

    def buffers():
        b = dict(left=torch.zeros((NS, na + 3), dtype=torch.float32, device="cuda"), right=torch.zeros((NS, na + 3), dtype=torch.float32, device="cuda"),
                 pcm=torch.full((NS, 2 * na + 4), 12345, dtype=torch.int16, device="cuda"), pc=torch.zeros(NS, dtype=torch.int32, device="cuda"))
        if bc:
            b["bb"] = torch.zeros((NS, 2 * nr + 2), dtype=torch.float32, device="cuda")
        return b

    def one_call(dm, sink, k, b, audio=True):
        l, r = (b["left"], b["right"]) if audio else (None, None)
        if bc:
            return dm.process_batch_pcm_device(sink, iq[k], l, r, b["pcm"], b["bb"], b["pc"])
        return dm.process_batch_pcm_device(sink, iq[k], l, r, b["pcm"], b["pc"]), 0

    def read(b, audio=True):
        l = b["left"][:, :na].cpu().numpy() if audio else None
        r = b["right"][:, :na].cpu().numpy() if audio else None
        pc = b["pc"].cpu().numpy().view(np.uint32)
        pcm = b["pcm"].cpu().numpy()
        assert (pcm[:, 2 * na:] == 12345).all()
        out = (l, r, np.ascontiguousarray(b["bb"][:, :2 * nr].cpu().numpy()), pc) if bc else (l, r, pc)
        return out, pcm[:, :2 * na]

    torch.cuda.synchronize()
    with _handle(pkg, kind, generic) as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink, pkg.StereoPcmSink(NS - 1, alpha, gain) as other:
        for k in range(NCALLS):
            b = buffers()
            if k == 1:                                                                     # refusals between two valid calls
                n1, n2 = C.c_uint32(), C.c_uint32()
                ptr = lambda t: C.c_void_p(t.data_ptr())
                tail = (ptr(b["bb"]), b["bb"].stride(0), ptr(b["pc"]), C.byref(n1), C.byref(n2), 1) if bc else (ptr(b["pc"]), C.byref(n1), 1)
                fn = lib.sdrfm_bcast_process_batch_pcm if bc else lib.sdrfm_stereo_process_batch_pcm
                args = lambda k_, l, r, p, ps: (dm._h, k_._h, ptr(iq[k]), iq[k].stride(0), NBYTES, l, r, na + 3, p, ps) + tail
                E, ECAP = pkg.lib.EINVAL, pkg.lib.ECAPACITY
                assert fn(*args(other, ptr(b["left"]), ptr(b["right"]), ptr(b["pcm"]), 2 * na + 4)) == E          # a sink of another stream count
                assert fn(*args(sink, None, ptr(b["right"]), ptr(b["pcm"]), 2 * na + 4)) == E                       # half-NULL audio
                assert fn(*args(sink, ptr(b["left"]), None, ptr(b["pcm"]), 2 * na + 4)) == E
                assert fn(*args(sink, ptr(b["left"]), ptr(b["right"]), None, 2 * na + 4)) == E
                assert fn(*args(sink, ptr(b["left"]), ptr(b["right"]), ptr(b["pcm"]), 2 * na - 2)) == ECAP
                assert fn(*args(sink, ptr(b["left"]), ptr(b["right"]), ptr(b["pcm"]), 2 * na + 3)) == E
                assert fn(*args(sink, ptr(b["left"]), ptr(b["right"]), C.c_void_p(b["pcm"].data_ptr() + 2), 2 * na + 4)) == E
                dm.synchronize()
                assert (b["pcm"].cpu().numpy() == 12345).all() and not b["left"].cpu().numpy().any()
            assert one_call(dm, sink, k, b)[0] == na
            dm.synchronize()
            out, pcm = read(b)
            check("device", k, out, pcm)
            assert np.array_equal(pcm, host_pcm[k]), ("device against host form", k)
        check_state("device", sink)
    # device form without audio rows
    with _handle(pkg, kind, generic) as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
        for k in range(NCALLS):
            b = buffers()
            assert one_call(dm, sink, k, b, audio=False)[0] == na
            dm.synchronize()
            out, pcm = read(b, audio=False)
            check("device, no audio rows", k, out, pcm)
            assert np.array_equal(pcm, host_pcm[k]), ("device, no audio rows", k)
    # the two-call sequence on one stream
    stream = torch.cuda.Stream()
    with _handle(pkg, kind, generic) as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
        dm.set_stream(stream.cuda_stream)
        sink.set_stream(stream.cuda_stream)
        for k in range(NCALLS):
            b = buffers()
            if bc:
                n = dm.process_batch_device(iq[k], b["left"], b["right"], b["bb"], b["pc"])[0]
            else:
                n = dm.process_batch_device(iq[k], b["left"], b["right"], b["pc"])
            sink.process_batch_device(b["left"], b["right"], b["pcm"], n)
            stream.synchronize()
            assert np.array_equal(read(b)[1], host_pcm[k]), ("two calls", k)
