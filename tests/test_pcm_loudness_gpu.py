"""The stereo PCM sink's K-weighted loudness meter on the device (csrc/sdrfm_loudness.h).  The reference is the C routine
sdrfm_pcm_loudness_s16 on the PCM THE DEVICE RETURNED.  Energies are held to |e - e_host| <= RTOL e_host + ATOL block_len with the RTOL and
ATOL of tests/loudness_cases.py (measured on the CPU by tests/test_loudness_emulate_cpu.py, never from the device); pos, first_block and the
block counts are held exactly.  Integer patterns are placed through a sink with alpha = 1 and gain = 1, whose chain gives pcm = rint(x)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import loudness_cases as lc

pytestmark = pytest.mark.gpu


def _sink(pkg, ns, exact=False):
    return pkg.StereoPcmSink(ns, 1.0, 1.0, exact=exact)


def _rows(Li, Ri):
    return np.ascontiguousarray(Li, dtype=np.float32), np.ascontiguousarray(Ri, dtype=np.float32)


def _hold(got, want, bl, tag):
    ok, why = lc.within(got, want, bl)
    assert ok, (tag, why)


def _hold_state(pkg, sink, st, bl, tag):
    """pos exactly, the open sub-block's energy to the bound"""
    dev = sink.loudness_state()
    assert np.array_equal(dev["pos"], st["pos"]), (tag, dev["pos"][:4], st["pos"][:4])
    _hold(dev["e"], st["e"], bl, (tag, "open energy"))


@pytest.mark.parametrize("n", lc.LENGTHS)
def test_lengths_stream_counts_block_lengths_and_both_forms(pkg, n):
    for ns in lc.STREAMS:
        Li, Ri = lc.random_rows(n, ns)
        xl, xr = _rows(Li, Ri)
        for exact in (False, True):
            for bl in lc.BLOCK_LENS:
                with _sink(pkg, ns, exact) as sink:
                    sink.enable_loudness(bl, n // bl + 1)
                    pcm = sink.process_batch(xl, xr)
                    first, got = sink.read_loudness()
                    want, st = pkg.pcm_loudness_host(pcm, bl)
                    assert first == 0 and got.shape == (ns, n // bl, 2), (n, ns, bl, exact, first, got.shape)
                    _hold(got, want, bl, (n, ns, bl, exact))
                    _hold_state(pkg, sink, st, bl, (n, ns, bl, exact))
            if exact:
                assert np.array_equal(pcm, lc.interleave(Li, Ri))
            assert int(np.abs(pcm.astype(np.int32)).max()) > 30000 or n < 8                  # (full-range rows)


@pytest.mark.parametrize("bl", [64, 4800])
@pytest.mark.parametrize("name", ["dc_pos", "dc_neg", "burst_then_zeros", "tone_m60", "left_only"])
def test_hard_inputs(pkg, name, bl):
    """DC at either rail, a full-range burst followed by three calls of zeros, a -60 dBFS tone, L loud with R zero: call by call against the
    C routine with its state carried"""
    calls = lc.hard_rows()[name]
    st, at = None, 0
    with _sink(pkg, 2, exact=True) as sink:
        sink.enable_loudness(bl, 4800 // bl + 1)
        for k, (Li, Ri) in enumerate(calls):
            pcm = sink.process_batch(*_rows(Li, Ri))
            assert np.array_equal(pcm, lc.interleave(Li, Ri))                                # the case's values are in the PCM as intended
            first, got = sink.read_loudness()
            want, st = pkg.pcm_loudness_host(pcm, bl, state=st)
            assert first == at and got.shape == want.shape, (name, bl, k, first, got.shape)
            _hold(got, want, bl, (name, bl, k))
            _hold_state(pkg, sink, st, bl, (name, bl, k))
            at += got.shape[1]
    assert at == len(calls) * 4800 // bl


def test_cuts_of_a_ragged_sequence(pkg):
    """calls of 1, 0, 2, 4799, 257 and 64 pairs at block_len 100 — boundaries inside chunks, inside tiles and exactly at call ends: one read
    = the C routine on the concatenation = the C routine call by call = the reads taken after every call"""
    ns, bl, total = 2, 100, sum(lc.SEQUENCE)
    Li, Ri = lc.random_rows(total, ns)
    xl, xr = _rows(Li, Ri)
    with _sink(pkg, ns) as whole, _sink(pkg, ns) as cut:
        whole.enable_loudness(bl, 64)
        cut.enable_loudness(bl, 64)
        st, at, pieces, reads, firsts = None, 0, [], [], []
        by_call = []
        for k in lc.SEQUENCE:
            a = whole.process_batch(xl[:, at:at + k], xr[:, at:at + k])
            b = cut.process_batch(xl[:, at:at + k], xr[:, at:at + k])
            assert np.array_equal(a, b)
            first, e = cut.read_loudness()
            w, st = pkg.pcm_loudness_host(a, bl, state=st)
            assert e.shape == w.shape and (first == sum(r.shape[1] for r in reads) or e.shape[1] == 0), (k, first, e.shape)
            _hold_state(pkg, cut, st, bl, ("call", k))
            reads.append(e)
            by_call.append(w)
            pieces.append(a)
            at += k
        pcm = np.concatenate(pieces, axis=1)
        first, got = whole.read_loudness()
        want, st_whole = pkg.pcm_loudness_host(pcm, bl)
        assert first == 0 and got.shape == (ns, total // bl, 2) and int(st_whole["pos"][0]) == total
        _hold(got, want, bl, "whole")
        _hold(got, np.concatenate(by_call, axis=1), bl, "call by call")
        _hold(np.concatenate(reads, axis=1), want, bl, "reads")
        assert got.tobytes() == np.concatenate(reads, axis=1).tobytes()                     # the same calls: the same bits
        _hold_state(pkg, whole, st_whole, bl, "whole")


def test_ring_keeps_the_newest(pkg):
    lib = pkg.load_library()
    ns, bl, n = 3, 64, 4800
    Li, Ri = lc.random_rows(2 * n, ns)
    xl, xr = _rows(Li, Ri)
    with _sink(pkg, ns) as sink:
        sink.enable_loudness(bl, 4)
        a = sink.process_batch(xl[:, :n], xr[:, :n])
        want, st = pkg.pcm_loudness_host(a, bl)
        assert want.shape[1] == 75
        buf, first, nb = np.full((ns, 4, 2), -1.0), C.c_uint64(99), C.c_uint32(99)
        assert lib.sdrfm_pcm_stereo_sink_loudness_read(sink._h, buf.ctypes.data, 3, C.byref(first), C.byref(nb), 0) == pkg.lib.ECAPACITY
        assert (buf == -1.0).all() and first.value == 99 and nb.value == 99                  # refused: nothing written, nothing consumed
        first, got = sink.read_loudness()
        assert first == 71 and got.shape == (ns, 4, 2)
        _hold(got, want[:, 71:75], bl, "first call")
        first, got = sink.read_loudness()
        assert first == 75 and got.shape == (ns, 0, 2)                                       # nothing new
        b = sink.process_batch(xl[:, n:], xr[:, n:])
        want2, st = pkg.pcm_loudness_host(b, bl, state=st)
        first, got = sink.read_loudness()
        assert first == 146 and got.shape == (ns, 4, 2) and want2.shape[1] == 75
        _hold(got, want2[:, 71:75], bl, "second call")
        _hold_state(pkg, sink, st, bl, "ring")
    # a ring that wraps inside one read: 8 slots, calls of 100 pairs, reads after the calls 2, 5 and 7
    with _sink(pkg, ns) as sink:
        sink.enable_loudness(bl, 8)
        st, at, pending, nxt = None, 0, [], 0
        for k in range(7):
            a = sink.process_batch(xl[:, at:at + 100], xr[:, at:at + 100])
            w, st = pkg.pcm_loudness_host(a, bl, state=st)
            pending.append(w)
            at += 100
            if k in (1, 4, 6):
                first, got = sink.read_loudness()
                want = np.concatenate(pending, axis=1)
                assert first == nxt and got.shape == want.shape and want.shape[1] <= 8, (k, first, got.shape, want.shape)
                _hold(got, want, bl, ("wrap", k))
                nxt, pending = nxt + want.shape[1], []
        assert nxt == 700 // 64


@pytest.mark.parametrize("pad", [2, 6])
def test_device_rows_off_alignment_with_padding_and_a_canary(pkg, pad):
    """device rows 4 bytes into an allocation, pcm_stride = 2n + pad, the padding and a canary row behind the last stream filled with -32768
    beforehand: neither read into any energy nor changed.  On the caller's stream through set_stream."""
    import torch
    ns, n, bl = 3, 257, 64
    stride = 2 * n + pad
    rng = np.random.default_rng(40 + pad)
    Li, Ri = rng.integers(-20000, 20001, (ns, n)), rng.integers(-20000, 20001, (ns, n))
    xl, xr = _rows(Li, Ri)
    base = torch.full((2 + (ns + 1) * stride,), -32768, dtype=torch.int16, device="cuda")
    rows = base[2:].view(ns + 1, stride)
    assert rows.data_ptr() % 16 == 4
    dl, dr = torch.from_numpy(xl).cuda(), torch.from_numpy(xr).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _sink(pkg, ns) as sink:
        sink.set_stream(stream.cuda_stream)
        sink.enable_loudness(bl, 8)
        sink.process_batch_device(dl, dr, rows[:ns], n)
        first, got = sink.read_loudness()
        dev = sink.loudness_state()
        sink.set_stream(None)
    back = rows.cpu().numpy()
    assert (back[:ns, 2 * n:] == -32768).all() and (back[ns] == -32768).all() and (base[:2].cpu().numpy() == -32768).all()
    pcm = np.ascontiguousarray(back[:ns, :2 * n])
    assert np.abs(pcm.astype(np.int32) - lc.interleave(Li, Ri)).max() <= 1 and not (pcm == -32768).any()
    want, st = pkg.pcm_loudness_host(pcm, bl)
    assert first == 0 and got.shape == (ns, n // bl, 2) and (dev["pos"] == n).all()
    _hold(got, want, bl, pad)                                                                # a counted -32768 would be far outside
    _hold(dev["e"], st["e"], bl, (pad, "open energy"))


def test_one_stream_with_a_row_stride_of_zero(pkg):
    import torch
    n, bl = 300, 64
    Li, Ri = lc.random_rows(n, 1)
    xl, xr = _rows(Li, Ri)
    dl, dr = torch.from_numpy(xl).cuda(), torch.from_numpy(xr).cuda()
    pcm = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with _sink(pkg, 1, exact=True) as sink:
        sink.enable_loudness(bl, 8)
        st = pkg.load_library().sdrfm_pcm_stereo_sink_process_batch(sink._h, C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr()), 0, n,
                                                                    C.c_void_p(pcm.data_ptr()), 0, pkg.lib.F_DEVICE_PTRS | 4)
        assert st == 0
        first, got = sink.read_loudness()
    back = pcm.cpu().numpy()[None, :]
    assert np.array_equal(back, lc.interleave(Li, Ri)) and first == 0
    _hold(got, pkg.pcm_loudness_host(back, bl)[0], bl, "stride 0")


def test_the_same_calls_give_the_same_bits(pkg):
    ns = 3
    Li, Ri = lc.random_rows(lc.TILE + 500, ns)
    xl, xr = _rows(Li, Ri)
    runs = []
    for _ in range(2):
        with _sink(pkg, ns) as sink:
            sink.enable_loudness(100, 64)
            at, out = 0, []
            for k in (257, lc.TILE + 1, 242):
                sink.process_batch(xl[:, at:at + k], xr[:, at:at + k])
                at += k
                out.append(sink.read_loudness()[1])
            runs.append((np.concatenate(out, axis=1).tobytes(), sink.loudness_state().tobytes()))
    assert runs[0] == runs[1]


def _params(pkg):
    return pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))


@pytest.mark.parametrize("hicut", [False, True], ids=["plain", "hicut"])
@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_no_bit_moves_in_the_four_sink_forms(pkg, exact, hicut):
    """PCM, states, hicut_state and audio-meter records of a sink with loudness equal those of a sink without over three calls; with meter and
    loudness both enabled, both are right"""
    import audio_meter_ref as aref
    alpha, gain = _params(pkg)
    ns, n, bl = 5, 255, 64
    rng = np.random.default_rng(50)
    xl = (0.4 * rng.standard_normal((ns, 3 * n))).astype(np.float32)
    xr = (0.4 * rng.standard_normal((ns, 3 * n))).astype(np.float32)
    xl[2, 300:500] = 0.0
    xr[2, 300:500] = 0.0
    with pkg.StereoPcmSink(ns, alpha, gain, exact=exact) as plain, pkg.StereoPcmSink(ns, alpha, gain, exact=exact) as loud:
        plain.enable_meter(2)
        loud.enable_meter(2)
        loud.enable_loudness(bl, 16)
        pieces = []
        for k in range(3):
            if hicut and k < 2:
                for s_ in (plain, loud):
                    s_.set_hicut([8192, 32768, 2048, 16384, 1024] if k == 0 else 20000, ramp_ms=5.0)
            a = plain.process_batch(xl[:, k * n:(k + 1) * n], xr[:, k * n:(k + 1) * n])
            b = loud.process_batch(xl[:, k * n:(k + 1) * n], xr[:, k * n:(k + 1) * n])
            assert np.array_equal(a, b), k
            assert plain.state().tobytes() == loud.state().tobytes(), k
            ha, hb = plain.hicut_state(), loud.hicut_state()
            assert np.array_equal(ha[0], hb[0]) and np.array_equal(ha[1], hb[1]) and ha[2] == hb[2], k
            assert plain.read_meters(reset=False).tobytes() == loud.read_meters(reset=False).tobytes(), k
            pieces.append(b)
        pcm = np.concatenate(pieces, axis=1)
        assert int(np.abs(pcm.astype(np.int32)).max()) > 1000
        assert aref.same(loud.read_meters(), aref.records(pcm, 2))
        first, got = loud.read_loudness()
        want, st = pkg.pcm_loudness_host(pcm, bl)
        assert first == 0 and got.shape == want.shape == (ns, 3 * n // bl, 2)
        _hold(got, want, bl, (exact, hicut))
        _hold_state(pkg, loud, st, bl, (exact, hicut))
        with pytest.raises(pkg.SdrfmError) as e:                                            # a sink that never enabled loudness
            plain.read_loudness()
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
    iq = np.stack([pkg.make_iq_rds(1, nsamp, pkg.rds_encode_groups(0x4100 + s, "LOUD  %02d" % s), rds_phase=0.5 * s, first_id=5300 + s)[0] for s in range(NS)])
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
    """StereoDemod.process_batch_pcm, BroadcastDemod.process_batch_pcm, the metered call and the hist call on host buffers, two calls, an audio
    meter on both sinks: every output, the sink states and the meter records equal the run without loudness bit for bit, and the energies
    equal the C routine's on the returned PCM"""
    alpha, gain = _params(pkg)
    bl, outs = 64, {}
    for loud in (False, True):
        with _handle(pkg, "stereo" if kind == "stereo" else "bcast") as dm, pkg.StereoPcmSink(NS, alpha, gain) as sink:
            sink.enable_meter(4)
            if loud:
                sink.enable_loudness(bl, 64)
            outs[loud] = [_call(dm, kind, sink, np.ascontiguousarray(_stations()[:, k * NBYTES:(k + 1) * NBYTES])) for k in range(NCALLS)]
            dm.synchronize()
            outs[loud].append((sink.state(), sink.read_meters()))
            if loud:
                first, got = sink.read_loudness()
                dev = sink.loudness_state()
    for a, b in zip(outs[False], outs[True]):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), kind
    pcm = np.concatenate([outs[True][k][2] for k in range(NCALLS)], axis=1)
    na = NCALLS * (NBYTES // 2 // D // DA)
    assert pcm.shape == (NS, 2 * na) and int(np.abs(pcm.astype(np.int32)).max()) > 1000
    want, st = pkg.pcm_loudness_host(pcm, bl)
    assert first == 0 and got.shape == want.shape == (NS, na // bl, 2) and (dev["pos"] == na).all()
    _hold(got, want, bl, kind)
    _hold(dev["e"], st["e"], bl, (kind, "open energy"))


def test_lifecycle_and_refusals_on_a_live_sink(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    ns, bl = 3, 64
    Li, Ri = lc.random_rows(400, ns)
    xl, xr = _rows(Li, Ri)
    first, nb = C.c_uint64(), C.c_uint32()
    buf = np.zeros((ns, 16, 2))
    with _sink(pkg, ns) as sink:
        read = lambda out, cap, f, q, flags: lib.sdrfm_pcm_stereo_sink_loudness_read(sink._h, out, cap, f, q, flags)
        assert read(buf.ctypes.data, 16, C.byref(first), C.byref(nb), 0) == E               # not enabled
        assert lib.sdrfm_pcm_stereo_sink_loudness_disable(sink._h) == 0                     # nothing to stop
        assert lib.sdrfm_pcm_stereo_sink_loudness_get_state(sink._h, buf.ctypes.data) == E
        sink.enable_loudness(bl, 16)
        a = sink.process_batch(xl[:, :100], xr[:, :100])
        want_a, st = pkg.pcm_loudness_host(a, bl)
        # every refusal on the live sink ...
        nan = pkg.loudness_default_coef()
        nan[0] = np.nan
        unstable = pkg.loudness_default_coef()
        unstable[9] = 1.0
        outside = [lc.coef_sets()[k] for k in ("k192000", "hp r=0.999 th=pi-1e-3", "shelf r=0.999 th=0.01")]   # stable, but not in the device's domain
        assert all(lib.sdrfm_loudness_check_coef(c.ctypes.data) == 0 and lib.sdrfm_loudness_check_domain(c.ctypes.data, None, None) == E for c in outside)
        for coef, b_, cap in [(None, 63, 16), (None, (1 << 20) + 1, 16), (None, bl, 0), (None, bl, 4097), (nan, bl, 16), (unstable, bl, 16)] + [
                (c, bl, 16) for c in outside]:
            assert lib.sdrfm_pcm_stereo_sink_loudness_enable(sink._h, None if coef is None else coef.ctypes.data, b_, cap) == E
        for flags in (1, 2, 8, 0x80000000):
            assert read(buf.ctypes.data, 16, C.byref(first), C.byref(nb), flags) == E
        assert read(buf.ctypes.data, 16, None, C.byref(nb), 0) == E and read(buf.ctypes.data, 16, C.byref(first), None, 0) == E
        assert read(None, 16, C.byref(first), C.byref(nb), 0) == E
        assert read(buf.ctypes.data, 0, C.byref(first), C.byref(nb), 0) == pkg.lib.ECAPACITY
        assert lib.sdrfm_pcm_stereo_sink_loudness_get_state(sink._h, None) == E
        assert lib.sdrfm_pcm_stereo_sink_process_batch(sink._h, None, None, 100, 100, None, 200, 0) == E   # a refused sink call
        # ... leaves pos and the next energies unchanged
        _hold_state(pkg, sink, st, bl, "after the refusals")
        b = sink.process_batch(xl[:, 100:400], xr[:, 100:400])
        want_b, st = pkg.pcm_loudness_host(b, bl, state=st)
        f, got = sink.read_loudness()
        assert f == 0 and got.shape[1] == 6
        _hold(got, np.concatenate([want_a, want_b], axis=1), bl, "after the refusals")
        # reset: sub-block 0 again, from zero state
        sink.reset()
        assert not sink.loudness_state().tobytes().strip(b"\0")
        a = sink.process_batch(xl[:, :130], xr[:, :130])
        f, got = sink.read_loudness()
        assert f == 0 and got.shape[1] == 2
        _hold(got, pkg.pcm_loudness_host(a, bl)[0], bl, "reset")
        # re-enable with another block_len: starts over
        sink.enable_loudness(100, 2)
        assert not sink.loudness_state().tobytes().strip(b"\0")
        a = sink.process_batch(xl[:, :350], xr[:, :350])
        f, got = sink.read_loudness()
        assert f == 1 and got.shape[1] == 2                                                  # 3 completed, 2 kept
        _hold(got, pkg.pcm_loudness_host(a, 100)[0][:, 1:3], 100, "re-enable")
        sink.disable_loudness()
        with pytest.raises(pkg.SdrfmError) as e:
            sink.read_loudness()
        assert e.value.status == E
        pcm = sink.process_batch(np.ones((ns, 10), np.float32), np.ones((ns, 10), np.float32))   # a disabled sink goes on as before
        assert (pcm == 1).all()
        sink.enable_loudness()                                                              # the defaults: 4800, 64
        sink.process_batch(xl[:, :100], xr[:, :100])
        assert sink.read_loudness()[1].shape == (ns, 0, 2) and (sink.loudness_state()["pos"] == 100).all()


def test_end_to_end_a_minus_23_dbfs_tone(pkg):
    """thirty calls of a tenth of a second of a -23 dBFS-peak 1 kHz stereo sine: M = -23.0 +- 0.1 from the fourth sub-block on, S = -23.0 +- 0.1
    at the thirtieth; loudness_alarms quiet at target -23 and "too loud" at target -30"""
    n = 4800
    t = np.arange(30 * n)
    x = (32768.0 * 10.0 ** (-23.0 / 20.0) * np.sin(2 * np.pi * 1000.0 * t / 48000.0)).astype(np.float32)[None, :]
    mon = pkg.LoudnessMonitor(1, n)
    with _sink(pkg, 1) as sink:
        sink.enable_loudness(n, 64)
        for k in range(30):
            sink.process_batch(x[:, k * n:(k + 1) * n], x[:, k * n:(k + 1) * n])
            first, e = sink.read_loudness()
            assert first == k and e.shape == (1, 1, 2)
            assert mon.push(first, e) == 0
            s = mon.summary()[0]
            if k >= 3:
                assert abs(s["m"] + 23.0) <= 0.1, (k, s["m"])
            else:
                assert np.isnan(s["m"])
            assert np.isnan(s["s"]) == (k < 29)
    s = mon.summary()
    assert abs(s[0]["s"] + 23.0) <= 0.1 and abs(s[0]["i"] + 23.0) <= 0.1 and s[0]["gaps"] == 0 and s[0]["n_blocks"] == 30
    assert pkg.loudness_alarms(s, target=-23.0) == [dict(too_loud=False, too_quiet=False, gap=False)]
    assert pkg.loudness_alarms(s, target=-30.0) == [dict(too_loud=True, too_quiet=False, gap=False)]
    mon.close()
