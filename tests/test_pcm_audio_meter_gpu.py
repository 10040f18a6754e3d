"""The stereo PCM sink's audio meter on the device (csrc/sdrfm_audio_meter.h).  The reference is tests/audio_meter_ref.py, a numpy
restatement of the record's definition, evaluated on the PCM THE DEVICE RETURNED; every comparison is integer equality of all fields, no
tolerance anywhere.  Exact integers are placed through a sink with alpha = 1 and gain = 1, whose chain gives pcm = rint(x)
(tests/test_audio_meter_cpu.py shows it on the host routine); where a case depends on an exact value — the threshold edge, the rails — the
exact form is used, and the default form's cases keep quiet samples at 0 and loud ones at 1000 or more with the threshold between them.
Each such test asserts that the returned PCM holds the values the case is about."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import audio_meter_ref as ref

pytestmark = pytest.mark.gpu

Q = 8          # the default form's threshold: between the quiet samples (0) and the loud ones (>= 1000), a 1-LSB difference moves nothing


def _sink(pkg, ns, exact=False):
    return pkg.StereoPcmSink(ns, ref.ALPHA, ref.GAIN, exact=exact)


def _agree(pkg, got, pcm, q, tag=None):
    """got == the reference on this PCM == the host C routine on it"""
    want = ref.records(pcm, q)
    assert ref.same(got, want), (tag, ref.diff(got, want))
    assert ref.same(pkg.pcm_audio_meter_host(pcm, q), want), (tag, "the C routine")


def _quiet_pattern_is(pcm, L):
    """the returned PCM is quiet exactly where the case's integers are 0, on both channels, and loud by a wide margin elsewhere"""
    lq = np.abs(pcm[:, 0::2].astype(np.int32))
    rq = np.abs(pcm[:, 1::2].astype(np.int32))
    want = np.asarray(L) == 0
    return bool(np.array_equal(lq <= Q, want) and np.array_equal(rq <= Q, want) and (lq[~want] >= 900).all() and (rq[~want] >= 900).all())


@pytest.mark.parametrize("case", ["one_loud_pair", "one_quiet_pair"])
def test_every_boundary_whatever_the_geometry(pkg, case):
    """n = 1100, 1100 streams: stream p is quiet except one loud pair at p — and the complement — so that every pair index is a run boundary in
    some stream, wherever the kernel cuts its row"""
    ns = n = 1100
    L, R = getattr(ref, case)(ns, n)
    xl, xr = ref.rows_of(L, R)
    with _sink(pkg, ns) as sink:
        sink.enable_meter(Q)
        pcm = sink.process_batch(xl, xr)
        got = sink.read_meters()
    assert _quiet_pattern_is(pcm, L)
    _agree(pkg, got, pcm, Q, case)
    p = np.arange(ns)
    if case == "one_loud_pair":
        assert np.array_equal(got["quiet_both"]["lead"], p) and np.array_equal(got["quiet_both"]["trail"], n - 1 - p)
        assert np.array_equal(got["quiet_both"]["longest"], np.maximum(p, n - 1 - p)) and (got["quiet_both"]["count"] == n - 1).all()
    else:
        assert (got["quiet_l"]["count"] == 1).all() and (got["quiet_l"]["longest"] == 1).all()
        assert np.array_equal(got["quiet_l"]["lead"], (p == 0).astype(np.uint64)) and np.array_equal(got["quiet_l"]["trail"], (p == n - 1).astype(np.uint64))


def test_boundaries_around_every_multiple_of_64_at_4800(pkg):
    n = 4800
    pos = sorted(set([0, n - 1] + [m + d for m in range(64, n, 64) for d in (-1, 0, 1)]))
    ns = len(pos)
    for loud_pair in (True, False):
        L = np.zeros((ns, n), np.int64) if loud_pair else np.full((ns, n), 1000, np.int64)
        L[np.arange(ns), pos] = 1000 if loud_pair else 0
        xl, xr = ref.rows_of(L, -L)
        with _sink(pkg, ns) as sink:
            sink.enable_meter(Q)
            pcm = sink.process_batch(xl, xr)
            got = sink.read_meters()
        assert _quiet_pattern_is(pcm, L)
        _agree(pkg, got, pcm, Q, loud_pair)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4800, 4801, 4865])
def test_lengths_and_stream_counts_on_random_full_range_rows(pkg, n):
    rng = np.random.default_rng(1000 + n)
    for ns in (1, 3, 65):
        L, R = ref.random_full_range(rng, ns, n)
        xl, xr = ref.rows_of(L, R)
        for exact in (False, True):
            with _sink(pkg, ns, exact) as sink:
                sink.enable_meter(3)
                pcm = sink.process_batch(xl, xr)
                got = sink.read_meters()
            if exact:
                assert np.array_equal(pcm, ref.interleave(L, R))
            assert int(np.abs(pcm.astype(np.int32)).max()) > 30000 or n < 8                # (full-range rows)
            _agree(pkg, got, pcm, 3, (n, ns, exact))


@pytest.mark.parametrize("n", [4, 65539])
def test_32_bit_traps(pkg, n):
    """exact form, L = -32768 and R = 32767 throughout: sum L^2 = 2^32 at n = 4; at n = 65 539 the cross sum passes -2^46"""
    ns = 2
    L, R = np.full((ns, n), -32768), np.full((ns, n), 32767)
    xl, xr = ref.rows_of(L, R)
    with _sink(pkg, ns, exact=True) as sink:
        sink.enable_meter(32767)
        pcm = sink.process_batch(xl, xr)
        got = sink.read_meters()
    assert np.array_equal(pcm, ref.interleave(L, R))
    _agree(pkg, got, pcm, 32767, n)
    for s in range(ns):
        g = got[s]
        assert int(g["n"]) == n and int(g["sq_l"]) == n << 30 and int(g["sq_r"]) == n * 32767 * 32767 and int(g["cross"]) == -n * 32768 * 32767
        assert int(g["sum_l"]) == -32768 * n and int(g["sum_r"]) == 32767 * n
        assert int(g["peak_l"]) == 32768 and int(g["peak_r"]) == 32767 and int(g["clip_l"]) == n and int(g["clip_r"]) == n
        assert int(g["quiet_l"]["count"]) == 0 and int(g["quiet_r"]["longest"]) == n
    if n == 4:
        assert int(got[0]["sq_l"]) == 1 << 32
    else:
        assert int(got[0]["cross"]) < -(1 << 46)


@pytest.mark.parametrize("q", [0, 5, 32767])
def test_threshold_edge(pkg, q):
    """exact form: pairs at quiet_lsb and quiet_lsb + 1 of either sign, on L only, on R only and on both, in runs of three"""
    edge = [v for v in (q, -q, q + 1, -(q + 1)) if -32768 <= v <= 32767]
    other = [0, -32768]                                                                    # quiet at every threshold, loud at every threshold
    combos = [(a, b) for a in edge + other for b in edge + other]
    L = np.repeat(np.array([c[0] for c in combos]), 3)[None, :]
    R = np.repeat(np.array([c[1] for c in combos]), 3)[None, :]
    xl, xr = ref.rows_of(L, R)
    with _sink(pkg, 1, exact=True) as sink:
        sink.enable_meter(q)
        pcm = sink.process_batch(xl, xr)
        got = sink.read_meters()
    assert np.array_equal(pcm, ref.interleave(L, R))                                       # the edge values are in the PCM as intended
    assert (np.abs(L) == q).any() and (np.abs(L) == q + 1).any() and (np.abs(R) == q).any() and (np.abs(R) == q + 1).any()
    _agree(pkg, got, pcm, q, q)
    assert int(got[0]["quiet_l"]["count"]) == int((np.abs(L) <= q).sum()) and int(got[0]["quiet_r"]["count"]) == int((np.abs(R) <= q).sum())
    assert int(got[0]["quiet_both"]["count"]) == int(((np.abs(L) <= q) & (np.abs(R) <= q)).sum())


@pytest.mark.parametrize("pad", [2, 6])
def test_device_rows_off_alignment_with_padding_and_a_canary(pkg, pad):
    """device rows 4 bytes into an allocation (not 16-byte aligned), pcm_stride = 2n + pad, the padding and a canary row behind the last stream
    filled with -32768 beforehand: neither counted nor changed.  On the caller's stream through set_stream; a device-pointer read with RESET."""
    import torch
    ns, n = 3, 257
    stride = 2 * n + pad
    rng = np.random.default_rng(40 + pad)
    L, R = rng.integers(-20000, 20001, (ns, n)), rng.integers(-20000, 20001, (ns, n))      # no rail value: a counted canary would show in clip_*
    L[:, 100:140] = 0
    xl, xr = ref.rows_of(L, R)
    base = torch.full((2 + (ns + 1) * stride,), -32768, dtype=torch.int16, device="cuda")
    rows = base[2:].view(ns + 1, stride)
    assert rows.data_ptr() % 16 == 4
    dl, dr = torch.from_numpy(xl).cuda(), torch.from_numpy(xr).cuda()
    out = torch.full((ns, 24), -1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _sink(pkg, ns) as sink:
        sink.set_stream(stream.cuda_stream)
        sink.enable_meter(Q)
        sink.process_batch_device(dl, dr, rows[:ns], n)
        sink.read_meters_device(out, reset=True)
        sink.synchronize()
        got = out.cpu().numpy().view(pkg.AUDIO_METER_DTYPE).reshape(ns)
        again = sink.read_meters(reset=False)
        sink.set_stream(None)
    back = rows.cpu().numpy()
    assert (back[:ns, 2 * n:] == -32768).all() and (back[ns] == -32768).all() and (base[:2].cpu().numpy() == -32768).all()
    pcm = np.ascontiguousarray(back[:ns, :2 * n])
    assert np.abs(pcm.astype(np.int32) - ref.interleave(L, R)).max() <= 1 and not (pcm == -32768).any()
    _agree(pkg, got, pcm, Q, pad)
    assert not got["clip_l"].any() and not got["clip_r"].any() and (got["n"] == n).all()
    assert ref.same(again, np.zeros(ns, pkg.AUDIO_METER_DTYPE))                             # the RESET behind the device copy


def test_one_stream_with_a_row_stride_of_zero(pkg):
    import torch
    n = 300
    rng = np.random.default_rng(41)
    L, R = ref.random_full_range(rng, 1, n)
    xl, xr = ref.rows_of(L, R)
    dl, dr = torch.from_numpy(xl).cuda(), torch.from_numpy(xr).cuda()
    pcm = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _sink(pkg, 1, exact=True) as sink:
        sink.enable_meter(2)
        st = pkg.load_library().sdrfm_pcm_stereo_sink_process_batch(sink._h, C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr()), 0, n,
                                                                    C.c_void_p(pcm.data_ptr()), 0, pkg.lib.F_DEVICE_PTRS | 4)
        assert st == 0
        got = sink.read_meters()
    back = pcm.cpu().numpy()[None, :]
    assert np.array_equal(back, ref.interleave(L, R))
    _agree(pkg, got, back, 2)


SEQUENCE = (1, 0, 2, 4799, 257, 64)


def test_accumulation_over_a_ragged_sequence_of_calls(pkg):
    """calls of 1, 0, 2, 4799, 257 and 64 pairs, quiet runs across the call boundaries at 1, 3, 4802 and 5059: one read equals the reference on
    the concatenation, the ordered sdrfm_audio_meter_add of per-call reads with RESET, and the C routine; a call of no pairs changes nothing;
    reset and a second enable zero the records"""
    ns, total = 2, sum(SEQUENCE)
    L = np.full((ns, total), 1000, np.int64)
    L[0, 0:11] = 0                                                                          # across 1 (twice: the empty call) and 3
    L[0, 4790:5070] = 0                                                                     # across 4802 and 5059
    L[1, 2:4803] = 0
    L[1, 5059:] = 0
    xl, xr = ref.rows_of(L, -L)
    zero = np.zeros(ns, pkg.AUDIO_METER_DTYPE)
    with _sink(pkg, ns) as whole, _sink(pkg, ns) as cut:
        whole.enable_meter(Q)
        cut.enable_meter(Q)
        added, pieces, at = zero.copy(), [], 0
        for k in SEQUENCE:
            before = whole.read_meters(reset=False)
            a = whole.process_batch(xl[:, at:at + k], xr[:, at:at + k])
            b = cut.process_batch(xl[:, at:at + k], xr[:, at:at + k])
            assert np.array_equal(a, b)
            if k == 0:
                assert ref.same(whole.read_meters(reset=False), before)                     # n == 0 changes nothing
            part = cut.read_meters(reset=True)
            _agree(pkg, part, a, Q, ("call", at, k))
            pkg.audio_meter_add(added, part)
            pieces.append(a)
            at += k
        pcm = np.concatenate(pieces, axis=1)
        assert _quiet_pattern_is(pcm, L)
        got = whole.read_meters(reset=False)
        _agree(pkg, got, pcm, Q, "whole")
        assert ref.same(added, got), ref.diff(added, got)
        assert int(got[0]["quiet_both"]["longest"]) == 280 and int(got[0]["quiet_both"]["lead"]) == 11
        assert int(got[1]["quiet_both"]["longest"]) == 4801 and int(got[1]["quiet_both"]["trail"]) == 64
        assert ref.same(cut.read_meters(reset=False), zero)
        assert ref.same(whole.read_meters(reset=False), got)                                # a read without RESET keeps the records
        whole.reset()
        assert ref.same(whole.read_meters(reset=False), zero)
        whole.process_batch(xl[:, :100], xr[:, :100])
        assert int(whole.read_meters(reset=False)["n"][0]) == 100
        whole.enable_meter(0)                                                               # again: zeroed, and the new threshold
        assert ref.same(whole.read_meters(reset=False), zero)
        a = whole.process_batch(xl[:, :100], xr[:, :100])
        _agree(pkg, whole.read_meters(), a, 0, "second enable")


def _params(pkg):
    return pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))


@pytest.mark.parametrize("hicut", [False, True], ids=["plain", "hicut"])
@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_no_bit_moves_in_the_four_sink_forms(pkg, exact, hicut):
    """PCM, states and hicut_state of a metered sink equal an unmetered sink's over three calls; the records follow the PCM"""
    alpha, gain = _params(pkg)
    ns, n = 5, 255
    rng = np.random.default_rng(50)
    xl = (0.4 * rng.standard_normal((ns, 3 * n))).astype(np.float32)
    xr = (0.4 * rng.standard_normal((ns, 3 * n))).astype(np.float32)
    xl[2, 300:500] = 0.0
    xr[2, 300:500] = 0.0
    with pkg.StereoPcmSink(ns, alpha, gain, exact=exact) as plain, pkg.StereoPcmSink(ns, alpha, gain, exact=exact) as metered:
        metered.enable_meter(2)
        pieces = []
        for k in range(3):
            if hicut and k < 2:
                for s_ in (plain, metered):
                    s_.set_hicut([8192, 32768, 2048, 16384, 1024] if k == 0 else 20000, ramp_ms=5.0)
            a = plain.process_batch(xl[:, k * n:(k + 1) * n], xr[:, k * n:(k + 1) * n])
            b = metered.process_batch(xl[:, k * n:(k + 1) * n], xr[:, k * n:(k + 1) * n])
            assert np.array_equal(a, b), k
            assert plain.state().tobytes() == metered.state().tobytes(), k
            ha, hb = plain.hicut_state(), metered.hicut_state()
            assert np.array_equal(ha[0], hb[0]) and np.array_equal(ha[1], hb[1]) and ha[2] == hb[2], k
            pieces.append(b)
        pcm = np.concatenate(pieces, axis=1)
        assert int(np.abs(pcm.astype(np.int32)).max()) > 1000
        _agree(pkg, metered.read_meters(), pcm, 2, (exact, hicut))
        with pytest.raises(pkg.SdrfmError) as e:                                            # a sink that never enabled its meter
            plain.read_meters()
        assert e.value.status == pkg.lib.EINVAL


# ---- behind the one-call forms, at the smallest shape their own tests use (tests/test_pcm_stereo_sink_gpu.py) ----------------------------------------
FS, D, DA, DR = 2.4e6, 10, 5, 25
NS, NBYTES, NCALLS = 4, 48000, 2


def _front(pkg):
    return dict(fir_coeffs=pkg.lowpass_taps(64, 120e3 / FS), pilot_coeffs=pkg.stereo_pilot_taps(101, FS / D), audio_coeffs=pkg.lowpass_taps(32, 15e3 / (FS / D)),
                diff_gain=pkg.stereo_diff_gain(D, FS), pilot_min=0.05, fir_decim=D, audio_decim=DA, n_streams=NS, max_bytes_per_call=NBYTES)


def _handle(pkg, kind):
    if kind == "stereo":
        return pkg.StereoDemod(pkg.StereoConfig(**_front(pkg)))
    return pkg.BroadcastDemod(pkg.BroadcastConfig(rds_coeffs=pkg.rds_lowpass_taps(255, FS / D), rds_gain=pkg.rds_gain(D, FS), rds_decim=DR, **_front(pkg)))


@functools.lru_cache(maxsize=None)
def _stations():
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    nsamp = NCALLS * NBYTES // 2
    iq = np.stack([pkg.make_iq_rds(1, nsamp, pkg.rds_encode_groups(0x4100 + s, "METER %02d" % s), rds_phase=0.5 * s, first_id=5300 + s)[0] for s in range(NS)])
    iq.setflags(write=False)
    return iq


def _call(dm, kind, sink, iq):
    if kind in ("stereo", "bcast"):
        return dm.process_batch_pcm(sink, iq)
    if kind == "metered":
        return dm.process_batch_metered(iq, sink=sink)
    return dm.process_batch_metered_hist(iq, sink=sink)


@pytest.mark.parametrize("kind", ["stereo", "bcast", "metered", "hist"])
def test_no_bit_moves_behind_the_one_call_forms(pkg, kind):
    """StereoDemod.process_batch_pcm, BroadcastDemod.process_batch_pcm, the metered call and the hist call on host buffers, two calls: every
    output equals the unmetered run's bit for bit, and the record equals the reference on the returned PCM"""
    alpha, gain = _params(pkg)
    outs = {}
    for metered in (False, True):
        with _handle(pkg, "stereo" if kind == "stereo" else "bcast") as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
            if metered:
                sink.enable_meter(4)
            outs[metered] = [_call(dm, kind, sink, np.ascontiguousarray(_stations()[:, k * NBYTES:(k + 1) * NBYTES])) for k in range(NCALLS)]
            dm.synchronize()
            state = sink.state()
            records = sink.read_meters() if metered else None
            outs[metered].append((state,))
    for a, b in zip(outs[False], outs[True]):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), kind
    pcm = np.concatenate([outs[True][k][2] for k in range(NCALLS)], axis=1)
    assert pcm.shape == (NS, NCALLS * 2 * (NBYTES // 2 // D // DA)) and int(np.abs(pcm.astype(np.int32)).max()) > 1000
    _agree(pkg, records, pcm, 4, kind)


def test_one_call_form_on_device_buffers(pkg):
    """the broadcast one-call form on device buffers with a padded PCM stride: the record equals the reference on the PCM left on the device"""
    import torch
    alpha, gain = _params(pkg)
    na = NBYTES // 2 // D // DA
    iq = torch.from_numpy(np.ascontiguousarray(_stations()[:, :NBYTES])).cuda()
    pcm = torch.full((NS, 2 * na + 6), -32768, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _handle(pkg, "bcast") as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
        sink.enable_meter(4)
        bb = torch.zeros((NS, 2 * dm.counts(NBYTES)[1] + 2), dtype=torch.float32, device="cuda")
        pc = torch.zeros(NS, dtype=torch.int32, device="cuda")
        assert dm.process_batch_pcm_device(sink, iq, None, None, pcm, bb, pc)[0] == na
        dm.synchronize()
        got = sink.read_meters()
    back = pcm.cpu().numpy()
    assert (back[:, 2 * na:] == -32768).all()
    _agree(pkg, got, np.ascontiguousarray(back[:, :2 * na]), 4)
    assert (got["n"] == na).all() and int(np.abs(back[:, :2 * na].astype(np.int32)).max()) > 1000


def test_refusals_on_a_sink(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    out = np.zeros(3 * 24 + 1, np.uint64)
    with _sink(pkg, 3) as sink:
        read = lambda ptr, flags: lib.sdrfm_pcm_stereo_sink_meter_read(sink._h, ptr, flags)
        assert read(out.ctypes.data, 0) == E                                                # not enabled
        assert lib.sdrfm_pcm_stereo_sink_meter_enable(sink._h, 32768) == E and read(out.ctypes.data, 0) == E
        assert lib.sdrfm_pcm_stereo_sink_meter_disable(sink._h) == 0                        # nothing to stop
        sink.enable_meter(32767)
        assert read(out.ctypes.data, 0) == 0 and read(out.ctypes.data, 8) == 0
        for flags in (2, 4, 16, 0x80000000):
            assert read(out.ctypes.data, flags) == E
        assert read(None, 0) == E and read(out.ctypes.data + 4, 0) == E                     # 8-byte aligned
        assert lib.sdrfm_pcm_stereo_sink_meter_enable(sink._h, 40000) == E
        sink.process_batch(np.ones((3, 10), np.float32), np.ones((3, 10), np.float32))
        assert int(sink.read_meters(reset=False)["quiet_both"]["count"][0]) == 10           # the refused enable changed nothing
        sink.disable_meter()
        assert read(out.ctypes.data, 0) == E
        with pytest.raises(pkg.SdrfmError) as e:
            sink.read_meters()
        assert e.value.status == E
        pcm = sink.process_batch(np.ones((3, 10), np.float32), np.ones((3, 10), np.float32))   # a disabled sink goes on as before
        assert (pcm == 1).all()
        sink.enable_meter(0)
        assert not sink.read_meters()["n"].any()                                            # enabling starts from zero records
