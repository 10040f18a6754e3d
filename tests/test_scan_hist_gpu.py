"""GPU tests of the scan handle's hist call (sdrfm_scan_process_batch_hist) at the default shape.  Rows are compared as
integers: the call's records against the plain call's on a second handle, the fast kernel against the generic one, one call against a ragged
sequence summed with sdrfm_scan_hist_add and against plain and hist calls alternating on one handle, 1 / 3 / 7 / 256 streams on one shared
row and against replicated rows, host and device buffers with hist_stride 512 and 520 between canaries, the caller's stream, reset, tune and
refused calls.  Exact against the device's own d at offset 0 (the bit-exact mono handle hands d back); against tests/scan_ref.py from bytes
at the tuned offsets of tests/scan_hist_cases.py, edge by edge."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as sc
import scan_hist_cases as hc
from test_scan_gpu import _handle, _ndt, _rows, _same, _split, _want_name
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

BINS = hc.BINS


def _check_rows(meters, hist):
    """what holds of every call: uint32 [ns, 512], the bins outside [54, 457] empty, a row's sum its record's n"""
    assert hist.dtype == np.uint32 and hist.shape == (meters.size, BINS), (hist.dtype, hist.shape)
    assert not hist[:, :54].any() and not hist[:, 458:].any(), np.flatnonzero(hist.sum(0))
    assert (hist.sum(1, dtype=np.uint64) == meters["n"]).all(), (hist.sum(1), meters["n"])


def _hist_in_calls(pkg, scn, iq, cuts, plain=()):
    """the calls one after the other — those whose index is in `plain` as plain calls — summed with sdrfm_scan_meter_add and
    sdrfm_scan_hist_add; returns (records, rows uint64, the per-call (records, rows or None))"""
    acc, rows, pos, each = np.zeros(scn.n_streams, pkg.METER_DTYPE), np.zeros((scn.n_streams, BINS), np.uint64), 0, []
    for i, c in enumerate(cuts):
        if i in plain:
            m, hist = scn.process_batch(iq[:, pos:pos + c]), None
            assert c == 0 or not scn.kernel_name.endswith(" + hist")
        else:
            m, hist = scn.process_batch_hist(iq[:, pos:pos + c])
            _check_rows(m, hist)
            assert c == 0 or scn.kernel_name.endswith(" + hist")
            if c == 0:
                assert not hist.any() and not m.tobytes().strip(b"\0")
            pkg.hist_add(rows, hist)
        pkg.meter_add(acc, m)
        each.append((m, hist))
        pos += c
    assert pos == iq.shape[1]
    return acc, rows, each


# ---- 1. the records are the plain call's; the two kernel forms -------------------------------------------------------------------------
def test_records_are_the_plain_calls_and_fast_is_generic(pkg):
    su = sc.case_setup(pkg, sc.CASES[2])                            # default shape, 7 streams, the five offsets
    got = []
    for generic in (False, True):
        with _handle(pkg, su["shape"], su["ctaps"], su["rot"], generic=generic) as scn, _handle(pkg, su["shape"], su["ctaps"], su["rot"], generic=generic) as pl:
            assert scn.kernel_name == _want_name(su["shape"], generic)
            m, hist = scn.process_batch_hist(su["iq"])
            assert scn.kernel_name == _want_name(su["shape"], generic) + " + hist"
            want = pl.process_batch(su["iq"])
        assert _same(m, want), (m, want)                              # all eight words of every record
        _check_rows(m, hist)
        got.append(hist)
    assert np.array_equal(got[0], got[1])
    assert (got[0].sum(1) == sc.NBYTES // 2 // 10).all() and len({r.tobytes() for r in got[0]}) == 7


# ---- 2. one call against a ragged sequence; plain and hist calls alternating ------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_ragged_and_alternating_calls_add_up_to_the_one_call(pkg, generic):
    """tests/test_scan_gpu.py's cuts: 0 and 2 bytes, a call whose M is below H, a second 0, one call of more than 64 steps (>= 3 workgroups
    a stream, >= 2 steps each), random ones.  All as hist calls they sum to the one call's rows; with every second call a plain one, each
    call gives what it gave in the first sequence: the carried state is one"""
    import torch
    shape = sc.SHAPES["default"]
    T, D, P = shape
    H, ndt, fs, ns = P - 1, _ndt(T, D, P), sc.tc.fs_of(D), 3
    cuts = [0, 2, 2 * D * (H // 2) - 2, 0, 2 * D * (64 * ndt + ndt // 2) + 6]
    cuts += [int(v) for v in 2 * np.random.default_rng(410 + generic).integers(1, D * ndt, 5)]
    long_, nbytes = cuts[4], sum(cuts)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (1, 2, 3):
        bps = _split(long_ // 2 // D, ndt, H, ns, per_cu * cus)
        assert bps >= 3 and (long_ // 2 // D + bps - 1) // bps > ndt, (bps, ndt)
    iq = _rows(pkg, ns, nbytes // 2, fs, 8400)
    h = sc.shape_taps(pkg, shape)[0]
    cyc = sc.OFFSETS[:ns]
    ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cyc])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cyc], np.float32)
    with _handle(pkg, shape, ctaps, rot, nbytes=nbytes, generic=generic) as scn:
        m1, h1 = scn.process_batch_hist(iq)
        _check_rows(m1, h1)
        scn.reset()
        acc, rows, each = _hist_in_calls(pkg, scn, iq, cuts)
        scn.reset()
        plain = set(range(1, len(cuts), 2))                         # the long call (index 4) stays a hist call, between two plain ones
        acc2, _, each2 = _hist_in_calls(pkg, scn, iq, cuts, plain)
    assert _same(acc, m1) and np.array_equal(rows, h1.astype(np.uint64)), (acc, m1)
    assert _same(acc2, m1)
    for i, ((ma, ha), (mb, hb)) in enumerate(zip(each, each2)):
        assert _same(ma, mb), (i, ma, mb)
        assert hb is None or np.array_equal(ha, hb), i
    assert (m1["n"] == nbytes // 2 // D).all()


# ---- 3. the stream count and the shared row ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_stream_count_split_and_sharing_do_not_change_a_row(pkg, generic):
    """1, 3, 7 and 256 streams with stream 0's tuning on one shared row (256 streams make the handle give a stream fewer workgroups than it
    gives one stream alone), and three replicated rows against the shared one"""
    su = sc.case_setup(pkg, sc.CASES[0])
    shape, row = su["shape"], su["iq"][0:1]
    got = []
    for ns in (1, 3, 7, 256):
        with _handle(pkg, shape, np.tile(su["ctaps"][0], (ns, 1)), np.tile(su["rot"][0], ns), generic=generic, shared=True) as scn:
            m, hist = scn.process_batch_hist(row)
        _check_rows(m, hist)
        assert m.tobytes() == m[0:1].tobytes() * ns
        got.append(hist)
    for hist in got:
        assert (hist == got[0][0]).all()
    with _handle(pkg, shape, np.tile(su["ctaps"][0], (3, 1)), np.tile(su["rot"][0], 3), generic=generic) as scn:
        m, hist = scn.process_batch_hist(np.repeat(row, 3, 0))
    assert np.array_equal(hist, got[1])


# ---- 4. host and device buffers, the row stride, the caller's stream --------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_buffers_strides_and_the_callers_stream(pkg, generic):
    import torch
    su = sc.case_setup(pkg, sc.CASES[1])                            # default shape, 3 streams
    shape, iq, ns = su["shape"], su["iq"], su["ns"]
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    d_iq = torch.from_numpy(iq.copy()).cuda()
    with _handle(pkg, shape, su["ctaps"], su["rot"], generic=generic) as scn:
        want_m, want_h = scn.process_batch_hist(iq)
        _check_rows(want_m, want_h)
        for stride in (512, 520):
            # host: canary rows around the array, canary words behind each row
            host = np.full((ns + 2, stride), 0xDEADBEEF, np.uint32)
            m = np.zeros(ns, pkg.METER_DTYPE)
            scn.reset()
            rc = lib.sdrfm_scan_process_batch_hist(scn._h, iq.ctypes.data, iq.shape[1], iq.shape[1], m.ctypes.data, host[1:].ctypes.data, stride, 0)
            assert rc == pkg.lib.OK, rc
            assert _same(m, want_m) and np.array_equal(host[1:ns + 1, :BINS], want_h), ("host", stride)
            assert (host[0] == 0xDEADBEEF).all() and (host[ns + 1] == 0xDEADBEEF).all() and (host[:, BINS:] == 0xDEADBEEF).all(), ("host", stride)
            # device
            d_h = torch.full((ns + 2, stride), -7, dtype=torch.int32, device="cuda")
            d_m = torch.full((ns + 2, 8), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            scn.reset()
            rc = lib.sdrfm_scan_process_batch_hist(scn._h, C.c_void_p(d_iq.data_ptr()), d_iq.stride(0), iq.shape[1], C.c_void_p(d_m.data_ptr() + 64),
                                                   C.c_void_p(d_h.data_ptr() + 4 * stride), stride, DEV)
            assert rc == pkg.lib.OK, rc
            scn.synchronize()
            gh, gm = d_h.cpu().numpy(), d_m.cpu().numpy()
            assert _same(np.ascontiguousarray(gm[1:ns + 1]).view(pkg.METER_DTYPE).reshape(ns), want_m), ("device", stride)
            assert np.array_equal(gh[1:ns + 1, :BINS].view(np.uint32), want_h), ("device", stride)
            assert (gh[0] == -7).all() and (gh[ns + 1] == -7).all() and (gh[:, BINS:] == -7).all() and (gm[0] == -7).all() and (gm[ns + 1] == -7).all()
            # a device call of no bytes zeroes the rows' 512 words and nothing else
            rc = lib.sdrfm_scan_process_batch_hist(scn._h, None, 0, 0, C.c_void_p(d_m.data_ptr() + 64), C.c_void_p(d_h.data_ptr() + 4 * stride), stride, DEV)
            assert rc == pkg.lib.OK, rc
            scn.synchronize()
            gh = d_h.cpu().numpy()
            assert not gh[1:ns + 1, :BINS].any() and (gh[0] == -7).all() and (gh[ns + 1] == -7).all() and (gh[:, BINS:] == -7).all()
            assert not d_m.cpu().numpy()[1:ns + 1].any()
        # the Python form on the caller's stream, rows of 520 words
        d_h = torch.full((ns, 520), -7, dtype=torch.int32, device="cuda")
        d_m = torch.full((ns, 8), -7, dtype=torch.int64, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        scn.reset()
        scn.set_stream(stream.cuda_stream)
        scn.process_batch_hist_device(d_iq, d_m, d_h)
        scn.synchronize()
        stream.synchronize()
        gh = d_h.cpu().numpy()
        assert np.array_equal(gh[:, :BINS].view(np.uint32), want_h) and (gh[:, BINS:] == -7).all()
        assert _same(d_m.cpu().numpy().view(pkg.METER_DTYPE).reshape(ns), want_m)
        scn.reset()                                                  # a host call on the caller's stream
        m, hist = scn.process_batch_hist(iq)
        assert _same(m, want_m) and np.array_equal(hist, want_h)
        scn.set_stream(None)


# ---- 5. reset, tune and refused calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_reset_tune_and_refused_calls(pkg, generic):
    su = sc.case_setup(pkg, sc.CASES[1])
    iq, half, ns = su["iq"], 2 * 30001, su["ns"]
    other = np.roll(su["ctaps"], 1, axis=0), np.roll(su["rot"], 1)
    lib = pkg.load_library()
    with _handle(pkg, su["shape"], su["ctaps"], su["rot"], generic=generic) as scn:
        first = scn.process_batch_hist(iq[:, :half])
        second = scn.process_batch_hist(iq[:, half:])
        scn.reset()
        again = scn.process_batch_hist(iq[:, :half])
        scn.process_batch_hist(iq[:, half:half + 2 * 777])           # (state to be dropped)
        scn.tune(ctaps=other[0], rot=other[1])
        moved = scn.process_batch_hist(iq[:, :half])
        scn.tune(ctaps=su["ctaps"], rot=su["rot"])
        third = scn.process_batch_hist(iq[:, :half])
        # refused calls write nothing and leave the state alone: the second half continues the stream
        m = np.full(ns, 5, pkg.METER_DTYPE)
        hist = np.full((ns, BINS), 9, np.uint32)
        call = lambda iqp, stride, nb, mp, hp, hs, fl: lib.sdrfm_scan_process_batch_hist(scn._h, iqp, stride, nb, mp, hp, hs, fl)
        I, M_, H_ = iq.ctypes.data, m.ctypes.data, hist.ctypes.data
        assert call(I, iq.shape[1], 100, M_, None, BINS, 0) == pkg.lib.EINVAL
        assert call(I, iq.shape[1], 100, M_, H_, BINS - 1, 0) == pkg.lib.EINVAL
        assert call(I, iq.shape[1], 101, M_, H_, BINS - 1, 0) == pkg.lib.EINVAL          # the stride's refusal comes before the odd count's
        assert call(I, iq.shape[1], 100, None, H_, BINS, 0) == pkg.lib.EINVAL
        assert call(I, iq.shape[1], 101, M_, H_, BINS, 0) == pkg.lib.EODD
        assert call(I, iq.shape[1], 101, M_, H_, BINS, pkg.lib.F_OVERLAP) == pkg.lib.EINVAL    # the flags' before the odd count's, as in the plain call
        assert call(I, iq.shape[1], sc.NBYTES + 2, M_, H_, BINS, 0) == pkg.lib.ECAPACITY
        assert call(I, 98, 100, M_, H_, BINS, 0) == pkg.lib.ECAPACITY
        assert call(None, iq.shape[1], 100, M_, H_, BINS, 0) == pkg.lib.EINVAL
        assert (m["n"] == 5).all() and (m["reserved"] == 5).all() and (hist == 9).all()
        rest = scn.process_batch_hist(iq[:, half:])
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert same(first, again) and same(first, third) and not np.array_equal(first[1], moved[1])
    assert same(second, rest)


# ---- 6. exact against the device's own d at offset 0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_offset_zero_rows_are_exact_on_the_devices_own_d(pkg, generic):
    """taps (h, 0) and rot 0 give the untuned d bit for bit; the bit-exact mono handle with a one-tap unit audio filter hands that d back, and
    the rows are the numpy bincount of it"""
    shape = sc.SHAPES["default"]
    T, D, P = shape
    ns, fs = 3, sc.tc.fs_of(D)
    iq = np.stack([pkg.make_iq_rds(1, sc.NBYTES // 2, sc.tc.GROUPS, fs=fs, first_id=8500)[0], pkg.make_iq(1, sc.NBYTES // 2, mode="fm", fs=fs, first_id=8501)[0],
                   pkg.make_iq(1, sc.NBYTES // 2, mode="random", fs=fs, first_id=8502)[0]])
    h, b = sc.shape_taps(pkg, shape)
    one = np.ones(1, np.float32)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True,
                                  max_bytes_per_call=sc.NBYTES)) as mono:
        d = mono.process_batch(iq)
    with _handle(pkg, shape, np.tile(pairs(h), (ns, 1)), np.zeros(ns, np.float32), generic=generic) as scn:
        m, hist = scn.process_batch_hist(iq)
    _check_rows(m, hist)
    for s in range(ns):
        want = hc.hist_of(d[s])
        assert np.array_equal(hist[s].astype(np.uint64), want), (s, np.flatnonzero(hist[s] != want))
    assert np.count_nonzero(hist[2]) > 300 and np.count_nonzero(hist[0]) < 300     # noise fills the range, a station does not


# ---- 7. against the reference from bytes, at the tuned offsets ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.TUNED_CASES, ids=["%s-%dstreams" % (c[0], len(c[1])) for c in hc.TUNED_CASES])
def test_tuned_offsets_against_the_reference(pkg, case):
    """the device's d lies within 1e-5 rad of the reference's, so a d may change its bin only where the reference's d lies within 1e-5 of the
    edge between them: for every bin edge, |cumulative device count - cumulative reference count| <= the reference d's within 1e-5 of it"""
    cs = hc.tuned_case(pkg, case)
    for generic in ((False, True) if case[0] == "default" else (True,)):
        with _handle(pkg, cs["shape"], cs["ctaps"], cs["rot"], generic=generic) as scn:
            m, hist = scn.process_batch_hist(cs["iq"])
            name = scn.kernel_name
        _check_rows(m, hist)
        for s, r in enumerate(cs["refs"]):
            want, slack = hc.hist_of(r["d"]), hc.near_edge(r["d"])
            moved = int(np.abs(np.cumsum(hist[s].astype(np.int64)) - np.cumsum(want.astype(np.int64))).max())
            print("%s stream %d (%s at %+.4f): %d bins in use, the cumulative counts differ by %d at the most, %d d's (%.3f %%) at an edge" % (
                name, s, cs["names"][s], cs["cycles"][s], np.count_nonzero(want), moved, int(slack.sum()), 100 * hc.edge_share(r["d"])))
            assert int(m["n"][s]) == r["d"].size and hc.edge_share(r["d"]) <= hc.EDGE_CAP
            assert hc.cumulative_ok(hist[s], want, slack) == [], (name, s, hc.cumulative_ok(hist[s], want, slack))
