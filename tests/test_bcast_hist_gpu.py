"""GPU tests of the broadcast handle's hist call (sdrfm_bcast_process_batch_metered_hist) at the default shape.  Rows are
compared as integers, without a tolerance: against a ScanDemod's hist rows for the same bytes and tuning, the fast kernels against the
generic ones, one call against a ragged sequence summed with sdrfm_scan_hist_add and against hist, plain, PCM and metered calls in turn;
every other output and all eight words of the records bitwise against a second handle's metered call; the sum and the freq_q bracket of
tests/bcast_hist_cases.py on every call; blended and re-tuned handles; 1 / 3 / 7 / 256 streams on one shared row; host and device rows at
stride 512 and 520 between canaries; the caller's stream; reset, tune and refused calls.  One tuned scenario against tests/scan_ref.py from
bytes, edge by edge."""
import ctypes as C

import numpy as np
import pytest

import bcast_hist_cases as bh
import scan_hist_cases as hc
import tuned_cases as tc
from test_bcast_meter_gpu import MAX_NDT, _bcast, _records_equal, _rows, _same, _scan, _tuning, _want_name
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

BINS, SHAPE = bh.BINS, tc.SHAPES["default"]
FORMS = pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])


def _words(m):
    """a METER_DTYPE array as its 64-bit words: all eight of every record"""
    return np.ascontiguousarray(m).view(np.uint64)


def _outputs_equal(got, want, where):
    """L, R, bb bitwise and pilot_count"""
    for g, w, what in zip(got[:3], want[:3], ("L", "R", "bb")):
        assert _same(g, w), (where, what)
    assert np.array_equal(got[3], want[3]), (where, got[3], want[3])


def _check(got, metered, scan_rows, where):
    """a hist call's (L, R, bb, pilot_count, records, rows) against a second handle's metered call and a scan handle's rows"""
    _outputs_equal(got, metered, where)
    assert np.array_equal(_words(got[4]), _words(metered[4])), (where, got[4], metered[4])
    bh.check_rows(got[4], got[5], where)
    assert np.array_equal(got[5], scan_rows), (where, np.argwhere(got[5] != scan_rows)[:8])


def _sink(pkg, ns):
    return pkg.StereoPcmSink(ns, pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))


def _names(bc, generic, tuned, blend=False):
    assert bc.kernel_name == _want_name(SHAPE, generic, tuned) + (" blend" if blend else ""), bc.kernel_name
    assert bc.hist_kernel_name() == bc.kernel_name + " + hist" == bh.hist_name(SHAPE, tuned, generic, blend), bc.hist_kernel_name()


# ---- 1. against the other handles: tuned on own rows and on one shared row, untuned ----------------------------------------------------
def test_tuned_rows_are_the_scan_handles_and_the_rest_the_metered_calls(pkg):
    """the five offsets on seven own rows (station / carrier / const in turn), then the three-station capture as one shared row"""
    su = tc.case_setup(pkg, tc.CASES[1])
    ns, pm = su["ns"], su["pilot_min"]
    row = tc.three_stations(pkg)[0][:, :tc.NBYTES]
    h = tc.shape_taps(pkg, SHAPE)[0]
    offs = [st["offset_hz"] for st in tc.STATIONS]
    ctaps3 = np.stack([pkg.tuned_channel_taps(h, f, 2.4e6) for f in offs])
    rot3 = np.array([pkg.tuned_rotation(f, 2.4e6, 10) for f in offs], np.float32)
    rows = {}
    for generic in (False, True):
        with _bcast(pkg, SHAPE, ns, pm, generic=generic) as bc, _bcast(pkg, SHAPE, ns, pm, generic=generic) as other, \
                _scan(pkg, SHAPE, su["ctaps"], su["rot"], pm, generic=generic) as scn:
            bc.tune(ctaps=su["ctaps"], rot=su["rot"])
            other.tune(ctaps=su["ctaps"], rot=su["rot"])
            _names(bc, generic, True)
            got = bc.process_batch_metered_hist(su["iq"])
            _names(bc, generic, True)
            _check(got, other.process_batch_metered(su["iq"]), scn.process_batch_hist(su["iq"])[1], "own rows, generic %s" % generic)
            assert (got[4]["n"] == tc.NBYTES // 2 // 10).all() and len({r.tobytes() for r in got[5]}) == ns
        with _bcast(pkg, SHAPE, 3, generic=generic) as bc, _bcast(pkg, SHAPE, 3, generic=generic) as other, \
                _scan(pkg, SHAPE, ctaps3, rot3, generic=generic, shared=True) as scn:
            bc.tune(ctaps=ctaps3, rot=rot3, shared_input=True)
            other.tune(ctaps=ctaps3, rot=rot3, shared_input=True)
            shared = bc.process_batch_metered_hist(row)
            _check(shared, other.process_batch_metered(row), scn.process_batch_hist(row)[1], "one shared row, generic %s" % generic)
            bc.tune(ctaps=ctaps3, rot=rot3)
            assert np.array_equal(bc.process_batch_metered_hist(np.repeat(row, 3, 0))[5], shared[5])
        rows[generic] = (got[5], shared[5])
    for a, b in zip(rows[False], rows[True]):
        assert np.array_equal(a, b)                                  # fast rows are generic rows


def test_untuned_rows_are_the_scan_handles_at_offset_zero(pkg):
    """a station, random bytes, the counter and constant bytes on an untuned handle against taps (h, 0) and rot 0; with a sink the PCM and
    the sink's state are the metered PCM call's"""
    ns, fs = 4, 2.4e6
    iq = np.stack([pkg.make_iq_rds(1, tc.NBYTES // 2, tc.GROUPS, fs=fs, first_id=9100)[0]] +
                  [pkg.make_iq(1, tc.NBYTES // 2, mode=m, fs=fs, first_id=9101 + k)[0] for k, m in enumerate(("random", "counter", "const"))])
    h = tc.shape_taps(pkg, SHAPE)[0]
    rows = []
    for generic in (False, True):
        with _bcast(pkg, SHAPE, ns, generic=generic) as bc, _bcast(pkg, SHAPE, ns, generic=generic) as other, \
                _scan(pkg, SHAPE, np.tile(pairs(h), (ns, 1)), np.zeros(ns, np.float32), generic=generic) as scn, \
                _sink(pkg, ns) as sink, _sink(pkg, ns) as other_sink:
            _names(bc, generic, False)
            want_rows = scn.process_batch_hist(iq)[1]
            got = bc.process_batch_metered_hist(iq)
            _check(got, other.process_batch_metered(iq), want_rows, "untuned, generic %s" % generic)
            bc.reset()
            other.reset()
            l, r, pcm, bb, pc, m, hist = bc.process_batch_metered_hist(iq, sink=sink)
            wl, wr, wpcm, wbb, wpc, wm = other.process_batch_metered(iq, sink=other_sink)
            _check((l, r, bb, pc, m, hist), (wl, wr, wbb, wpc, wm), want_rows, "untuned with a sink, generic %s" % generic)
            assert np.array_equal(pcm, wpcm) and _same(sink.state(), other_sink.state())
            l, r, pcm, bb, pc, m, hist = bc.process_batch_metered_hist(iq[:, :2 * 30001], sink=sink, with_audio=False)
            assert l is None and r is None and np.array_equal(pcm, other.process_batch_metered(iq[:, :2 * 30001], sink=other_sink)[2])
            bh.check_rows(m, hist)
        rows.append(got[5])
        # constant bytes: d = 0 but for the few d's while the 64 channel taps fill; noise fills the range
        assert int(got[5][3, 256]) >= tc.NBYTES // 2 // 10 - 7 and np.count_nonzero(got[5][3]) <= 8 and np.count_nonzero(got[5][1]) > 300
    assert np.array_equal(rows[0], rows[1])


# ---- 2. the ragged sequence: all hist calls, and in turn with plain, PCM and metered calls ------------------------------------------------
@FORMS
def test_ragged_calls_add_up_and_hist_calls_mix_with_the_others(pkg, generic):
    """tests/test_bcast_meter_gpu.py's cuts: 0 and 2 bytes, one short of an audio and of an RDS output, a call whose M is below H, a second
    0, one call of 64 * 1023 + 600 new d's (64 workgroups a stream at the most, 1023 d's a step at the most: every workgroup walks two
    steps at the least), random ones"""
    import torch
    T, D, P, Ta, Da, Tr, Dr = SHAPE
    H, ns = P - 1 + max(Ta, Tr) - 1, 3
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 64 * ns
    cuts = [0, 2, 2 * D * Da - 4, 2 * D * Dr - 4, 2 * D * (H // 2) - 2, 0, 2 * D * (64 * MAX_NDT + 600) + 6]
    cuts += [int(v) for v in 2 * np.random.default_rng(520 + generic).integers(1, D * MAX_NDT, 4)]
    nbytes = sum(cuts)
    iq = _rows(pkg, ns, nbytes // 2, 2.4e6, 9600)
    ctaps, rot = _tuning(pkg, SHAPE, ns, 1)
    with _bcast(pkg, SHAPE, ns, nbytes=nbytes, generic=generic) as bc, _scan(pkg, SHAPE, ctaps, rot, nbytes=nbytes, generic=generic) as scn, \
            _sink(pkg, ns) as sink:
        bc.tune(ctaps=ctaps, rot=rot)
        one = bc.process_batch_metered_hist(iq)
        bh.check_rows(one[4], one[5], "one call")
        assert np.array_equal(one[5], scn.process_batch_hist(iq)[1])
        seqs = {}
        for what in ("plain", "hist", "in turn"):
            bc.reset()
            parts, acc_m, acc_h, pos, each = ([], [], []), np.zeros(ns, pkg.METER_DTYPE), np.zeros((ns, BINS), np.uint64), 0, {}
            for k, c in enumerate(cuts):
                part = iq[:, pos:pos + c]
                kind = {"plain": 0, "hist": 1}.get(what, (1, 0, 2, 3)[k % 4])   # in turn: hist, plain, PCM, metered, ...
                if what == "in turn" and k == 6:
                    kind = 1                                        # ... and the long call a hist call, between a plain and a metered one
                if kind == 0:
                    out = bc.process_batch(part)
                elif kind == 2:
                    l, r, _, bb, pc = bc.process_batch_pcm(sink, part)
                    out = (l, r, bb, pc)
                elif kind == 3:
                    out = bc.process_batch_metered(part)
                else:
                    out = bc.process_batch_metered_hist(part)
                    bh.check_rows(out[4], out[5], (what, k))
                    if c == 0:
                        assert not out[5].any() and not out[4].tobytes().strip(b"\0")
                    pkg.meter_add(acc_m, out[4])
                    pkg.hist_add(acc_h, out[5])
                    each[k] = out[5]
                for a, v in zip(parts, out[:3]):
                    a.append(v)
                pos += c
            assert pos == nbytes
            seqs[what] = (tuple(np.concatenate(p, 1) for p in parts), acc_m, acc_h, each)
    for what in ("plain", "hist", "in turn"):
        for g, w, nm in zip(seqs[what][0], one[:3], ("L", "R", "bb")):
            assert _same(g, w), (what, nm)                           # every output is the one call's bits: the all-plain sequence's
    _records_equal(seqs["hist"][1], one[4], "the cuts summed")
    assert np.array_equal(seqs["hist"][2], one[5].astype(np.uint64))
    for k, rows in seqs["in turn"][3].items():                      # a hist call gives the rows it gave among hist calls only
        assert np.array_equal(rows, seqs["hist"][3][k]), k
    assert 6 in seqs["in turn"][3] and (one[4]["n"] == nbytes // 2 // D).all()


# ---- 3. blend and re-tune ------------------------------------------------------------------------------------------------------------------
@FORMS
def test_blended_handle_gives_the_unblended_rows(pkg, generic):
    """set_audio mid-ramp: the BL forms of the hist kernels.  The rows are the unblended handle's, L and R the blended metered call's"""
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, iq, half = su["ns"], su["iq"], 2 * 20000
    with _bcast(pkg, SHAPE, ns, generic=generic) as bc, _bcast(pkg, SHAPE, ns, generic=generic) as other, _bcast(pkg, SHAPE, ns, generic=generic) as plain:
        for h_ in (bc, other, plain):
            h_.tune(ctaps=su["ctaps"], rot=su["rot"])
        want = [plain.process_batch_metered_hist(iq[:, :half]), plain.process_batch_metered_hist(iq[:, half:])]
        for h_ in (bc, other):
            h_.process_batch(iq[:, :half])
            h_.set_audio(blend=[0.0, 0.5, 1.0], gain=[0.25, 1.0, 0.5], ramp_ms=50.0)   # 50 ms of ramp against 21 ms of audio: mid-ramp throughout
        _names(bc, generic, True, blend=True)
        got, met = bc.process_batch_metered_hist(iq[:, half:]), other.process_batch_metered(iq[:, half:])
        st = bc.audio_state()
        assert 0 < int(st["blend"][0]) < 32768 and 8192 < int(st["gain"][0]) < 32768, st
    _outputs_equal(got, met, "blended")
    assert np.array_equal(_words(got[4]), _words(met[4])) and np.array_equal(_words(got[4]), _words(want[1][4]))
    assert np.array_equal(got[5], want[1][5]) and not _same(got[0], want[1][0])
    bh.check_rows(got[4], got[5], "blended")


@FORMS
def test_retuned_handle_keeps_the_bracket_and_an_untouched_streams_rows(pkg, generic):
    """after a re-tune with a carry (stream 1 moved by 3 kHz) and a restart (stream 2), the sum and the bracket hold on every stream; stream
    0, whose taps stay, gives the scan handle's rows of the continued stream"""
    ns, fs, half = 3, 2.4e6, 2 * 31003
    row = tc.three_stations(pkg)[0][:, :tc.NBYTES]
    offs = np.array([st["offset_hz"] for st in tc.STATIONS])
    with _bcast(pkg, SHAPE, ns, generic=generic) as bc, _bcast(pkg, SHAPE, ns, generic=generic) as other:
        for h_ in (bc, other):
            h_.tune(offsets_hz=offs, fs=fs, shared_input=True)
        ctaps, rot = bc._ctaps.copy(), bc._rot.copy()
        first = bc.process_batch_metered_hist(row[:, :half])
        other.process_batch_metered(row[:, :half])
        for h_ in (bc, other):
            h_.retune(offsets_hz=offs + np.array([0.0, 3e3, 0.0]), fs=fs, restart=[0, 0, 1])
        _names(bc, generic, True)
        second = bc.process_batch_metered_hist(row[:, half:])
        met = other.process_batch_metered(row[:, half:])
    with _scan(pkg, SHAPE, ctaps, rot, generic=generic, shared=True) as scn:
        want = [scn.process_batch_hist(row[:, :half])[1], scn.process_batch_hist(row[:, half:])[1]]
    bh.check_rows(first[4], first[5], "before the re-tune")
    bh.check_rows(second[4], second[5], "after the re-tune")
    _outputs_equal(second, met, "after the re-tune")
    assert np.array_equal(_words(second[4]), _words(met[4]))
    assert np.array_equal(first[5], want[0]) and np.array_equal(second[5][0], want[1][0])
    assert not np.array_equal(second[5][1], want[1][1])             # (3 kHz are five bins)


# ---- 4. the stream count ---------------------------------------------------------------------------------------------------------------------
@FORMS
def test_stream_count_and_split_do_not_change_a_row(pkg, generic):
    """1, 3, 7 and 256 streams with one tuning on one shared row: 256 streams make the handle give a stream fewer workgroups than it gives
    one stream alone"""
    su = tc.case_setup(pkg, tc.CASES[0])
    row = su["iq"][0:1]
    with _scan(pkg, SHAPE, su["ctaps"][0:1], su["rot"][0:1], generic=generic, shared=True) as scn:
        want = scn.process_batch_hist(row)[1]
    for ns in (1, 3, 7, 256):
        with _bcast(pkg, SHAPE, ns, generic=generic) as bc:
            bc.tune(ctaps=np.tile(su["ctaps"][0], (ns, 1)), rot=np.tile(su["rot"][0], ns), shared_input=True)
            out = bc.process_batch_metered_hist(row)
        bh.check_rows(out[4], out[5], ns)
        assert out[4].tobytes() == out[4][0:1].tobytes() * ns and (out[5] == want[0]).all(), ns


# ---- 5. host and device rows, the row stride, the caller's stream ----------------------------------------------------------------------------
def _raw(pkg, bc, iq, nbytes, meters, hist, stride, sink=None, pcm=None, flags=0, ca=1 << 16, cr=1 << 14):
    """the C call on host buffers large enough for any call of these tests; meters and hist are addresses; returns the status"""
    ns = bc.cfg.n_streams
    left, right, bb = np.zeros((ns, ca), np.float32), np.zeros((ns, ca), np.float32), np.zeros((ns, 2 * cr), np.float32)
    pc, na, nr = np.zeros(ns, np.uint32), C.c_uint32(), C.c_uint32()
    return pkg.load_library().sdrfm_bcast_process_batch_metered_hist(
        bc._h, sink._h if sink is not None else None, iq.ctypes.data, iq.shape[1], nbytes, left.ctypes.data, right.ctypes.data, ca,
        pcm.ctypes.data if pcm is not None else None, 2 * ca, bb.ctypes.data, 2 * cr, pc.ctypes.data, meters, hist, stride, C.byref(na), C.byref(nr),
        flags)


@FORMS
def test_buffers_strides_and_the_callers_stream(pkg, generic):
    import torch
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, iq = su["ns"], np.ascontiguousarray(su["iq"])
    nbytes = iq.shape[1]
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    d_iq = torch.from_numpy(iq.copy()).cuda()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with _bcast(pkg, SHAPE, ns, generic=generic) as bc:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        want = bc.process_batch_metered_hist(iq)
        na, nr = want[0].shape[1], want[2].shape[1]
        for stride in (512, 520):
            # host: canary rows around the array, canary words behind each row
            host = np.full((ns + 2, stride), 0xDEADBEEF, np.uint32)
            m = np.zeros(ns, pkg.METER_DTYPE)
            bc.reset()
            assert _raw(pkg, bc, iq, nbytes, m.ctypes.data, host[1:].ctypes.data, stride) == pkg.lib.OK
            assert np.array_equal(_words(m), _words(want[4])) and np.array_equal(host[1:ns + 1, :BINS], want[5]), ("host", stride)
            assert (host[0] == 0xDEADBEEF).all() and (host[ns + 1] == 0xDEADBEEF).all() and (host[:, BINS:] == 0xDEADBEEF).all(), ("host", stride)
            # device
            d_h = torch.full((ns + 2, stride), -7, dtype=torch.int32, device="cuda")
            d_m = torch.full((ns + 2, 8), -7, dtype=torch.int64, device="cuda")
            d_l, d_r = torch.zeros((ns, na), dtype=torch.float32, device="cuda"), torch.zeros((ns, na), dtype=torch.float32, device="cuda")
            d_w, d_pc = torch.zeros((ns, 2 * nr), dtype=torch.float32, device="cuda"), torch.zeros(ns, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            bc.reset()
            n1, n2 = C.c_uint32(), C.c_uint32()
            call = lambda src, nb: lib.sdrfm_bcast_process_batch_metered_hist(
                bc._h, None, src, d_iq.stride(0), nb, ptr(d_l), ptr(d_r), d_l.stride(0), None, 0, ptr(d_w), d_w.stride(0), ptr(d_pc), ptr(d_m, 64),
                ptr(d_h, 4 * stride), stride, C.byref(n1), C.byref(n2), DEV)
            assert call(ptr(d_iq), nbytes) == pkg.lib.OK and (n1.value, n2.value) == (na, nr)
            bc.synchronize()
            gh, gm = d_h.cpu().numpy(), d_m.cpu().numpy()
            assert np.array_equal(np.ascontiguousarray(gm[1:ns + 1]).view(np.uint64), _words(want[4]).reshape(ns, 8)), ("device", stride)
            assert np.array_equal(gh[1:ns + 1, :BINS].view(np.uint32), want[5]), ("device", stride)
            assert (gh[0] == -7).all() and (gh[ns + 1] == -7).all() and (gh[:, BINS:] == -7).all() and (gm[0] == -7).all() and (gm[ns + 1] == -7).all()
            assert _same(d_l.cpu().numpy(), want[0]) and _same(d_r.cpu().numpy(), want[1])
            assert _same(d_w.cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32)) and np.array_equal(d_pc.cpu().numpy(), want[3])
            # a device call of no bytes zeroes the rows' 512 words and the records, and nothing else
            assert call(None, 0) == pkg.lib.OK and (n1.value, n2.value) == (0, 0)
            bc.synchronize()
            gh, gm = d_h.cpu().numpy(), d_m.cpu().numpy()
            assert not gh[1:ns + 1, :BINS].any() and (gh[0] == -7).all() and (gh[ns + 1] == -7).all() and (gh[:, BINS:] == -7).all()
            assert not gm[1:ns + 1].any() and (gm[0] == -7).all() and (gm[ns + 1] == -7).all() and not d_pc.cpu().numpy().any()
        # the Python form on the caller's stream, rows of 520 words, with and without a sink
        d_h = torch.full((ns, 520), -7, dtype=torch.int32, device="cuda")
        d_m = torch.full((ns, 8), -7, dtype=torch.int64, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        bc.reset()
        bc.set_stream(stream.cuda_stream)
        assert bc.process_batch_metered_hist_device(d_iq, d_l, d_r, d_w, d_m, d_h, pilot_count=d_pc) == (na, nr)
        bc.synchronize()
        stream.synchronize()
        gh = d_h.cpu().numpy()
        assert np.array_equal(gh[:, :BINS].view(np.uint32), want[5]) and (gh[:, BINS:] == -7).all()
        assert np.array_equal(d_m.cpu().numpy().view(np.uint64), _words(want[4]).reshape(ns, 8)) and _same(d_l.cpu().numpy(), want[0])
        with _sink(pkg, ns) as sink, _sink(pkg, ns) as ref_sink:
            d_p = torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda")
            d_h.fill_(-7)
            stream.synchronize()
            bc.reset()
            assert bc.process_batch_metered_hist_device(d_iq, None, None, d_w, d_m.data_ptr(), d_h, sink=sink, pcm=d_p) == (na, nr)
            bc.synchronize()
            assert np.array_equal(d_h.cpu().numpy()[:, :BINS].view(np.uint32), want[5])
            assert np.array_equal(d_p.cpu().numpy(), ref_sink.process_batch(want[0], want[1]))
        bc.reset()                                                   # a host call on the caller's stream
        again = bc.process_batch_metered_hist(iq)
        assert np.array_equal(again[5], want[5]) and np.array_equal(_words(again[4]), _words(want[4])) and _same(again[0], want[0])
        bc.set_stream(None)


# ---- 6. reset, tune and refused calls ----------------------------------------------------------------------------------------------------------
def test_reset_and_tune_restart_the_rows(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    iq, half = su["iq"], 2 * 30001
    other = np.roll(su["ctaps"], 1, axis=0), np.roll(su["rot"], 1)
    with _bcast(pkg, SHAPE, su["ns"]) as bc:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        first = bc.process_batch_metered_hist(iq[:, :half])
        second = bc.process_batch_metered_hist(iq[:, half:])
        bc.reset()
        again = bc.process_batch_metered_hist(iq[:, :half])
        bc.process_batch_metered_hist(iq[:, half:half + 2 * 777])    # (state to be dropped)
        bc.tune(ctaps=other[0], rot=other[1])
        moved = bc.process_batch_metered_hist(iq[:, :half])
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        third = bc.process_batch_metered_hist(iq[:, :half])
        rest = bc.process_batch_metered_hist(iq[:, half:])
        bc.tune()                                                    # back to the untuned kernels and their hist forms
        _names(bc, False, False)
        untuned = bc.process_batch_metered_hist(iq[:, :half])
    same = lambda a, b: np.array_equal(a[5], b[5]) and np.array_equal(_words(a[4]), _words(b[4])) and _same(a[0], b[0])
    assert same(first, again) and same(first, third) and same(second, rest)
    assert not np.array_equal(first[5], moved[5]) and not np.array_equal(first[5], second[5]) and not np.array_equal(first[5], untuned[5])
    bh.check_rows(moved[4], moved[5], "tuned elsewhere")
    bh.check_rows(untuned[4], untuned[5], "untuned")


def test_every_refusal_leaves_the_next_call_unchanged(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, iq = su["ns"], np.ascontiguousarray(su["iq"])
    m = np.full(ns, 3, pkg.METER_DTYPE)
    hist = np.full((ns, BINS), 9, np.uint32)
    pcm = np.zeros((ns, 2 << 16), np.int16)
    M_, H_ = m.ctypes.data, hist.ctypes.data
    EINVAL, EODD, ECAP = pkg.lib.EINVAL, pkg.lib.EODD, pkg.lib.ECAPACITY
    with _bcast(pkg, SHAPE, ns) as bc, _sink(pkg, ns) as sink:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        one = bc.process_batch_metered_hist(iq)
        bc.reset()
        refusals = [(lambda: _raw(pkg, bc, iq, 1000, M_, None, BINS), EINVAL),                   # hist NULL
                    (lambda: _raw(pkg, bc, iq, 1001, M_, H_, BINS - 1), EINVAL),                 # the stride's refusal before the odd count's
                    (lambda: _raw(pkg, bc, iq, 1000, M_, H_, 0), EINVAL),
                    (lambda: _raw(pkg, bc, iq, 1000, None, H_, BINS), EINVAL),                   # meters NULL
                    (lambda: _raw(pkg, bc, iq, 1000, M_, H_ + 2, BINS), EINVAL),                 # rows off 4 bytes
                    (lambda: _raw(pkg, bc, iq, 1000, M_, H_, BINS, pcm=pcm), EINVAL),            # pcm without sink
                    (lambda: _raw(pkg, bc, iq, 1001, M_, H_, BINS, flags=pkg.lib.F_OVERLAP), EINVAL),
                    (lambda: _raw(pkg, bc, iq, 1001, M_, H_, BINS), EODD),
                    (lambda: _raw(pkg, bc, iq, 1001, M_, H_, BINS, sink=sink, pcm=pcm), EODD),
                    (lambda: _raw(pkg, bc, iq, tc.NBYTES + 2, M_, H_, BINS), ECAP),
                    (lambda: _raw(pkg, bc, iq[:, :98], 100, M_, H_, BINS), ECAP)]                 # iq_stride < nbytes
        cuts = [2 * 3001] * len(refusals)
        cuts.append(tc.NBYTES - sum(cuts))
        state0 = sink.state()
        parts, acc, pos = ([], [], []), np.zeros((ns, BINS), np.uint64), 0
        for k, c in enumerate(cuts):
            out = bc.process_batch_metered_hist(iq[:, pos:pos + c])
            pkg.hist_add(acc, out[5])
            for a, v in zip(parts, out[:3]):
                a.append(v)
            pos += c
            if k < len(refusals):
                call, want = refusals[k]
                assert call() == want, (k, want)
                assert (m["n"] == 3).all() and (m["reserved"] == 3).all() and (hist == 9).all()   # a refusal writes no record and no row
        for a, o, what in zip(parts, one[:3], "LRw"):
            assert _same(np.concatenate(a, 1), o), what
        assert np.array_equal(acc, one[5].astype(np.uint64)) and _same(sink.state(), state0)
        with pytest.raises(pkg.SdrfmError) as e:
            bc.process_batch_metered_hist(iq[:, :1001])
        assert e.value.status == EODD


def test_a_hist_call_takes_4_mib_at_the_most_and_tap_sums_refuse_it(pkg):
    four = 4 << 20
    iq = pkg.make_iq(1, four // 2 + 1, mode="fm", first_id=9400)
    m, hist = np.zeros(1, pkg.METER_DTYPE), np.full((1, BINS), 9, np.uint32)
    with _bcast(pkg, SHAPE, 1, nbytes=8 << 20) as bc:
        na, nr = bc.counts(four + 2)
        assert _raw(pkg, bc, iq, four + 2, m.ctypes.data, hist.ctypes.data, BINS, ca=na + 1, cr=nr + 1) == pkg.lib.ECAPACITY
        assert bc.counts(four + 2) == (na, nr) and (hist == 9).all()
    h = tc.shape_taps(pkg, SHAPE)[0]
    big_h = (h * np.float32(16.5 / np.abs(h.astype(np.float64)).sum())).astype(np.float32)
    with _bcast(pkg, SHAPE, 1, h=big_h) as bc:
        assert _raw(pkg, bc, iq, 1000, m.ctypes.data, hist.ctypes.data, BINS) == pkg.lib.EINVAL and (hist == 9).all()
        assert bc.process_batch(iq[:, :1000])[0].shape[1] == 10


# ---- 7. against the reference from bytes --------------------------------------------------------------------------------------------------------
@FORMS
def test_tuned_scenario_against_the_reference(pkg, generic):
    """tests/scan_hist_cases.py's criterion: the device's d lies within 1e-5 rad of the reference's, so for every bin edge
    |cumulative device count - cumulative reference count| <= the reference d's within 1e-5 rad of that edge"""
    cs = bh.ref_case(pkg)
    with _bcast(pkg, SHAPE, cs["ns"], generic=generic, h=cs["h"], b=cs["b"]) as bc:
        bc.tune(ctaps=cs["ctaps"], rot=cs["rot"])
        out = bc.process_batch_metered_hist(cs["iq"])
        name = bc.hist_kernel_name()
    bh.check_rows(out[4], out[5], name)
    for s, r in enumerate(cs["refs"]):
        want, slack = hc.hist_of(r["d"]), hc.near_edge(r["d"])
        moved = int(np.abs(np.cumsum(out[5][s].astype(np.int64)) - np.cumsum(want.astype(np.int64))).max())
        print("%s stream %d (%s at %+.4f): %d bins in use, the cumulative counts differ by %d at the most, %d d's (%.3f %%) at an edge" % (
            name, s, cs["names"][s], cs["cycles"][s], np.count_nonzero(want), moved, int(slack.sum()), 100 * hc.edge_share(r["d"])))
        assert int(out[4]["n"][s]) == r["d"].size and hc.edge_share(r["d"]) <= hc.EDGE_CAP
        assert hc.cumulative_ok(out[5][s], want, slack) == [], (name, s, hc.cumulative_ok(out[5][s], want, slack))
