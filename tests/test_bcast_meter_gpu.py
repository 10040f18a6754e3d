"""GPU tests of the metered broadcast call (sdrfm_bcast_process_batch_metered).  The records are exact integer sums, so
the yardstick is the scan handle itself: a metered call's 64 bytes per stream are the scan handle's for the same bytes, tuning, pilot
taps and pilot_min, field by field — tuned at the per-stream offsets of tests/tuned_cases.py, untuned against taps (h, 0) and rot 0 —
and L, R, bb, PCM and pilot_count are bit for bit a plain call's.  Then any cut into calls, metered and plain calls mixed, one shared
row against replicated rows, host against device buffers, 256 streams on one row, the PCM form, the refusals, and one scan scenario end
to end: records against tests/scan_ref.py, stream_status, a re-tune to what it returned."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as sc
import scan_ref as sr
import tuned_cases as tc
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

FIELDS = ("n", "n_pilot", "rf_q", "freq_q", "dev_q", "pilot_q", "pilot2_q")
KERNELS = [("default", False), ("default", True), ("T7-D3-P5", True), ("Ta>Tr", True)]
KERNEL_IDS = ["%s-%s" % (n, "generic" if g else "fast") for n, g in KERNELS]
MAX_NDT = 1023                                                  # new d's per step: no kernel of the handle takes more


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bcast(pkg, shape, ns, pilot_min=0.05, nbytes=tc.NBYTES, generic=False, h=None, b=None):
    T, D, P, Ta, Da, Tr, Dr = shape
    h0, ga, gr, b0, dg, rg = tc.shape_taps(pkg, shape)
    return pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h0 if h is None else h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b0 if b is None else b,
                                                  pilot_min=float(pilot_min), diff_gain=dg, rds_gain=rg, fir_decim=D, audio_decim=Da, rds_decim=Dr,
                                                  n_streams=ns, max_bytes_per_call=nbytes, force_generic=generic))


def _scan(pkg, shape, ctaps, rot, pilot_min=0.05, nbytes=tc.NBYTES, generic=False, shared=False):
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=tc.shape_taps(pkg, shape)[3], ctaps=ctaps, rot=rot, pilot_min=float(pilot_min), fir_decim=shape[1],
                                        shared_input=shared, max_bytes_per_call=nbytes, force_generic=generic))


def _want_name(shape, generic, tuned):
    kind = "generic" if generic or shape[:3] != (64, 10, 101) else "fast"
    return "bcast-%s%s T%d D%d P%d Ta%d Da%d Tr%d Dr%d" % ((kind, "-tuned" if tuned else "") + tuple(shape))


def _records_equal(got, want, where):
    """two METER_DTYPE arrays as integers, field by field; reserved is 0"""
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.shape, want.shape)
    for s in range(got.size):
        for f in FIELDS:
            assert int(got[f][s]) == int(want[f][s]), (where, "stream %d" % s, f, int(got[f][s]), int(want[f][s]))
    assert (got["reserved"] == 0).all(), (where, got["reserved"])


def _check(pkg, metered, plain, scan, M, where):
    """a metered call's (L, R, bb, pilot_count, records) against a plain call's outputs and the scan handle's records"""
    L, R, bb, pc, m = metered
    _records_equal(m, scan, where)
    assert (m["n"] == M).all(), (where, m["n"], M)
    assert np.array_equal(m["n_pilot"], pc.astype(np.uint64)), (where, m["n_pilot"], pc)
    for g, w, what in zip((L, R, bb), plain[:3], ("L", "R", "bb")):
        assert _same(g, w), (where, what)
    assert np.array_equal(pc, plain[3]), (where, pc, plain[3])


def _rows(pkg, ns, nsamp, fs, first_id):
    """ns rows of bytes: the FM generator, random bytes, the counter and constant bytes in turn"""
    return np.stack([pkg.make_iq(1, nsamp, mode=("fm", "random", "counter", "const")[s % 4], fs=fs, first_id=first_id + s)[0] for s in range(ns)])


def _tuning(pkg, shape, ns, idx):
    h, fs = tc.shape_taps(pkg, shape)[0], tc.fs_of(shape[1])
    cyc = [tc.OFFSETS[(s + idx) % len(tc.OFFSETS)] for s in range(ns)]
    return (np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cyc]), np.array([pkg.tuned_rotation(c * fs, fs, shape[1]) for c in cyc], np.float32))


# ---- 1. tuned: every case of tests/tuned_cases.py --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_tuned_records_are_the_scan_handles_and_the_outputs_the_plain_calls(pkg, case):
    su = tc.case_setup(pkg, case)
    shape, ns, pm = su["shape"], su["ns"], su["pilot_min"]
    M = tc.NBYTES // 2 // shape[1]
    for generic in ((False, True) if case[0] == "default" else (True,)):
        with _bcast(pkg, shape, ns, pm, generic=generic) as bc, _bcast(pkg, shape, ns, pm, generic=generic) as other, \
                _scan(pkg, shape, su["ctaps"], su["rot"], pm, generic=generic) as scn:
            bc.tune(ctaps=su["ctaps"], rot=su["rot"])
            other.tune(ctaps=su["ctaps"], rot=su["rot"])
            name = bc.kernel_name
            assert name == _want_name(shape, generic, True), name
            got = bc.process_batch_metered(su["iq"])
            assert bc.kernel_name == name                           # (the name is the handle's, metered or not)
            _check(pkg, got, other.process_batch(su["iq"]), scn.process_batch(su["iq"]), M, name)
        print("%s: %s, n %d, n_pilot %s, rf_q %s" % (name, "/".join(su["names"]), M, list(got[4]["n_pilot"]), list(got[4]["rf_q"])))
        if case[2] == "signal":
            assert int(got[4]["n_pilot"][0]) > 0 and int(got[4]["rf_q"][0]) > 0


# ---- 2. untuned: the offset-0 identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_untuned_records_are_the_scan_handles_at_offset_zero(pkg, name, generic):
    """an untuned handle's y and d are a scan stream's with taps (h, 0) and rot 0 bit for bit; a station, random bytes,
    the counter and constant bytes"""
    shape = tc.SHAPES[name]
    D, fs, ns = shape[1], tc.fs_of(shape[1]), 4
    iq = np.stack([pkg.make_iq_rds(1, tc.NBYTES // 2, tc.GROUPS, fs=fs, first_id=9100)[0]] +
                  [pkg.make_iq(1, tc.NBYTES // 2, mode=m, fs=fs, first_id=9101 + k)[0] for k, m in enumerate(("random", "counter", "const"))])
    h = tc.shape_taps(pkg, shape)[0]
    with _bcast(pkg, shape, ns, generic=generic) as bc, _bcast(pkg, shape, ns, generic=generic) as other, \
            _scan(pkg, shape, np.tile(pairs(h), (ns, 1)), np.zeros(ns, np.float32), generic=generic) as scn:
        assert bc.kernel_name == _want_name(shape, generic, False)
        got = bc.process_batch_metered(iq)
        _check(pkg, got, other.process_batch(iq), scn.process_batch(iq), tc.NBYTES // 2 // D, bc.kernel_name)
    assert 0 < int(got[4]["n_pilot"][0]) and int(got[4]["rf_q"][0]) > 0


# ---- 3. any cut into calls, metered and plain calls mixed, reset -------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_cuts_add_up_and_metered_calls_mix_with_plain_ones(pkg, name, generic):
    """0 and 2 bytes, one short of an audio and of an RDS output, a call whose M is below H, a second 0, one call of 64 * 1023 + 600 new d's —
    a stream gets 64 workgroups at the most and a step takes 1023 d's at the most, so every workgroup walks two steps at the least, and
    3 streams x 64 workgroups run at once on any device of 192 units, which is what makes 64 the split — then random ones"""
    import torch
    shape = tc.SHAPES[name]
    T, D, P, Ta, Da, Tr, Dr = shape
    H, ns, idx = P - 1 + max(Ta, Tr) - 1, 3, KERNELS.index((name, generic))
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 64 * ns
    cuts = [0, 2, 2 * D * Da - 4, 2 * D * Dr - 4, 2 * D * (H // 2) - 2, 0, 2 * D * (64 * MAX_NDT + 600) + 6]
    rng = np.random.default_rng(500 + idx)
    cuts += [int(v) for v in 2 * rng.integers(1, D * MAX_NDT, 4)]
    assert all(c >= 0 and c % 2 == 0 for c in cuts)
    nbytes = sum(cuts)
    iq = _rows(pkg, ns, nbytes // 2, tc.fs_of(D), 9200 + 10 * idx)
    ctaps, rot = _tuning(pkg, shape, ns, idx)
    with _bcast(pkg, shape, ns, nbytes=nbytes, generic=generic) as bc, _scan(pkg, shape, ctaps, rot, nbytes=nbytes, generic=generic) as scn:
        bc.tune(ctaps=ctaps, rot=rot)
        one = bc.process_batch_metered(iq)
        _records_equal(one[4], scn.process_batch(iq), "one call")
        assert (one[4]["n"] == nbytes // 2 // D).all()
        # the all-plain sequence
        bc.reset()
        plain, pos = ([], [], []), 0
        for c in cuts:
            for acc, v in zip(plain, bc.process_batch(iq[:, pos:pos + c])[:3]):
                acc.append(v)
            pos += c
        # the all-metered sequence, its records summed
        bc.reset()
        seq, acc_m, pos = ([], [], []), np.zeros(ns, pkg.METER_DTYPE), 0
        for c in cuts:
            want = bc.counts(c)
            l, r, w, pc, m = bc.process_batch_metered(iq[:, pos:pos + c])
            assert (l.shape[1], w.shape[1]) == want and (m["reserved"] == 0).all()
            assert (m["n"] == m["n"][0]).all() and np.array_equal(m["n_pilot"], pc.astype(np.uint64)), (c, m, pc)
            if c == 0:
                assert not m.tobytes().strip(b"\0")
            for a, v in zip(seq, (l, r, w)):
                a.append(v)
            pkg.meter_add(acc_m, m)
            pos += c
        assert pos == nbytes
        _records_equal(acc_m, one[4], "the cuts summed")
        # metered and plain calls in turn
        bc.reset()
        mixed, pos = ([], [], []), 0
        for k, c in enumerate(cuts):
            out = bc.process_batch_metered(iq[:, pos:pos + c]) if k % 2 == 0 else bc.process_batch(iq[:, pos:pos + c])
            for a, v in zip(mixed, out[:3]):
                a.append(v)
            pos += c
    for what, parts in (("plain", plain), ("metered", seq), ("mixed", mixed)):
        for p_, o, nm in zip(parts, one[:3], ("L", "R", "bb")):
            assert _same(np.concatenate(p_, 1), o), (name, what, nm)


def test_records_after_reset_are_the_first_calls(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    iq, half = su["iq"], 2 * 30001
    with _bcast(pkg, su["shape"], su["ns"]) as bc:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        first = bc.process_batch_metered(iq[:, :half])
        second = bc.process_batch_metered(iq[:, half:])
        bc.reset()
        again = bc.process_batch_metered(iq[:, :half])
        bc.process_batch(iq[:, half:half + 2 * 777])                # (state to be dropped)
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])                    # a re-tune is a restart
        third = bc.process_batch_metered(iq[:, :half])
        rest = bc.process_batch_metered(iq[:, half:])
    _records_equal(again[4], first[4], "after reset")
    _records_equal(third[4], first[4], "after tune")
    _records_equal(rest[4], second[4], "the second half")
    assert first[4].tobytes() != second[4].tobytes()
    for a, b_ in zip(first[:3] + second[:3], third[:3] + rest[:3]):
        assert _same(a, b_)


# ---- 4. rows and buffers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_shared_row_replicated_rows_and_device_buffers(pkg, generic):
    import torch
    shape, ns, nbytes = tc.SHAPES["default"], 3, tc.NBYTES
    row = tc.three_stations(pkg)[0][:, :nbytes]
    h = tc.shape_taps(pkg, shape)[0]
    offs = [st["offset_hz"] for st in tc.STATIONS]
    ctaps = np.stack([pkg.tuned_channel_taps(h, f, 2.4e6) for f in offs])
    rot = np.array([pkg.tuned_rotation(f, 2.4e6, 10) for f in offs], np.float32)
    cuts = [2 * 20001, 0, 2 * 7, nbytes - 2 * 20008]
    lib = pkg.load_library()

    def in_calls(bc, iq):
        acc, parts, pos = np.zeros(ns, pkg.METER_DTYPE), ([], [], []), 0
        for c in cuts:
            out = bc.process_batch_metered(iq[:, pos:pos + c])
            for a, v in zip(parts, out[:3]):
                a.append(v)
            pkg.meter_add(acc, out[4])
            pos += c
        return tuple(np.concatenate(p, 1) for p in parts), acc

    with _bcast(pkg, shape, ns, generic=generic) as bc, _scan(pkg, shape, ctaps, rot, generic=generic, shared=True) as scn:
        bc.tune(ctaps=ctaps, rot=rot)
        want, want_m = in_calls(bc, np.repeat(row, ns, 0))
        bc.tune(ctaps=ctaps, rot=rot, shared_input=True)
        got, got_m = in_calls(bc, row)
        _records_equal(got_m, want_m, "shared against replicated rows")
        _records_equal(got_m, scn.process_batch(row), "against the scan handle")
        assert len({m.tobytes() for m in got_m}) == ns               # (the streams do receive different stations)
        for a, b_ in zip(want, got):
            assert _same(a, b_)
        # device buffers: the row between canaries and an iq_stride that would run off it if it were used; the records between canary records
        na, nr = want[0].shape[1], want[2].shape[1]
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[32:32 + nbytes] = torch.from_numpy(row[0].copy()).cuda()
        rows3 = torch.from_numpy(np.repeat(row, ns, 0).copy()).cuda()
        for shared in (True, False):
            d_l = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
            d_r = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
            d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
            d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
            d_m = torch.full((ns + 2, 8), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            bc.tune(ctaps=ctaps, rot=rot, shared_input=shared)
            n1, n2 = C.c_uint32(), C.c_uint32()
            pos, oa, ow, acc = 0, 0, 0, np.zeros(ns, pkg.METER_DTYPE)
            ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
            for c in cuts:
                src, stride = (ptr(buf, 32 + pos), 1 << 40) if shared else (ptr(rows3, pos), rows3.stride(0))
                rc = lib.sdrfm_bcast_process_batch_metered(bc._h, None, src, stride, c, ptr(d_l, 4 * oa), ptr(d_r, 4 * oa), d_l.stride(0), None, 0,
                                                           ptr(d_w, 4 * ow), d_w.stride(0), ptr(d_pc), ptr(d_m, 64), C.byref(n1), C.byref(n2),
                                                           pkg.lib.F_DEVICE_PTRS)
                assert rc == pkg.lib.OK, rc
                bc.synchronize()
                host = d_m.cpu().numpy()
                assert (host[0] == -7).all() and (host[ns + 1] == -7).all(), host
                m = np.ascontiguousarray(host[1:ns + 1]).view(pkg.METER_DTYPE).reshape(ns)
                assert np.array_equal(m["n_pilot"], d_pc.cpu().numpy().astype(np.uint64))
                pkg.meter_add(acc, m)
                pos, oa, ow = pos + c, oa + n1.value, ow + 2 * n2.value
            assert (oa, ow) == (na, 2 * nr)
            _records_equal(acc, want_m, "device buffers, shared %s" % shared)
            assert _same(d_l[:, :na].cpu().numpy(), want[0]) and _same(d_r[:, :na].cpu().numpy(), want[1])
            assert _same(d_w[:, :2 * nr].cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32))
            assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all()
        assert (buf[:32] == 0xA5).all() and (buf[32 + nbytes:] == 0xA5).all()
        # process_batch_metered_device: the Python form of the same call, with and without a sink
        bc.tune(ctaps=ctaps, rot=rot, shared_input=True)
        d_l, d_r = torch.zeros((ns, na), dtype=torch.float32, device="cuda"), torch.zeros((ns, na), dtype=torch.float32, device="cuda")
        d_w, d_m = torch.zeros((ns, 2 * nr), dtype=torch.float32, device="cuda"), torch.full((ns, 8), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert bc.process_batch_metered_device(buf[32:32 + nbytes].unsqueeze(0), d_l, d_r, d_w, d_m) == (na, nr)
        bc.synchronize()
        one = d_m.cpu().numpy().view(pkg.METER_DTYPE).reshape(ns)
        _records_equal(one, want_m, "process_batch_metered_device")
        assert _same(d_l.cpu().numpy(), want[0]) and _same(d_w.cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32))
        alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
        with pkg.StereoPcmSink(ns, alpha, gain) as sink, pkg.StereoPcmSink(ns, alpha, gain) as ref_sink:
            d_p = torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda")
            d_m.fill_(-7)
            torch.cuda.synchronize()
            bc.reset()
            assert bc.process_batch_metered_device(buf[32:32 + nbytes].unsqueeze(0), None, None, d_w, d_m.data_ptr(), sink=sink, pcm=d_p) == (na, nr)
            bc.synchronize()
            _records_equal(d_m.cpu().numpy().view(pkg.METER_DTYPE).reshape(ns), want_m, "process_batch_metered_device with a sink")
            assert np.array_equal(d_p.cpu().numpy(), ref_sink.process_batch(want[0], want[1]))


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_256_streams_on_one_shared_row(pkg, generic):
    """256 streams x the workgroups one stream alone would get are more than the device runs at a time, so the handle gives a stream fewer;
    the five offsets in turn on one row of a station, against the scan handle's 256 records"""
    su = tc.case_setup(pkg, tc.CASES[0])
    shape, ns = su["shape"], 256
    ctaps, rot = _tuning(pkg, shape, ns, 0)
    row = su["iq"][0:1]
    with _bcast(pkg, shape, ns, generic=generic) as bc, _scan(pkg, shape, ctaps, rot, generic=generic, shared=True) as scn, \
            _bcast(pkg, shape, ns, generic=generic) as other:
        bc.tune(ctaps=ctaps, rot=rot, shared_input=True)
        other.tune(ctaps=ctaps, rot=rot, shared_input=True)
        _check(pkg, bc.process_batch_metered(row), other.process_batch(row), scn.process_batch(row), tc.NBYTES // 2 // shape[1], "256 streams")


# ---- 5. the PCM form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_pcm_form_is_the_pcm_call_and_the_plain_metered_records(pkg, generic):
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, half = su["ns"], 2 * 30001
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    chunks = [su["iq"][:, :half], su["iq"][:, half:]]
    with _bcast(pkg, su["shape"], ns, generic=generic) as bc, pkg.StereoPcmSink(ns, alpha, gain) as sink, \
            _bcast(pkg, su["shape"], ns, generic=generic) as other, pkg.StereoPcmSink(ns, alpha, gain) as other_sink:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        other.tune(ctaps=su["ctaps"], rot=su["rot"])
        records = [bc.process_batch_metered(c)[4] for c in chunks]  # the form without a sink
        bc.reset()
        for k, c in enumerate(chunks):
            audio = k == 0                                          # the second call passes no audio rows
            l, r, pcm, w, pc, m = bc.process_batch_metered(c, sink=sink, with_audio=audio)
            wl, wr, wpcm, ww, wpc = other.process_batch_pcm(other_sink, c, with_audio=audio)
            if audio:
                assert _same(l, wl) and _same(r, wr)
            else:
                assert l is None and r is None
            assert np.array_equal(pcm, wpcm) and _same(w, ww) and np.array_equal(pc, wpc), k
            assert _same(sink.state(), other_sink.state()), k
            _records_equal(m, records[k], "with a sink, call %d" % k)
            assert np.array_equal(m["n_pilot"], pc.astype(np.uint64))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def _raw(pkg, bc, iq, nbytes, meters, sink=None, pcm=None, flags=0, ca=1 << 16, cr=1 << 14):
    """the C call on host buffers large enough for any call of these tests; returns the status"""
    ns = bc.cfg.n_streams
    left, right, bb = np.zeros((ns, ca), np.float32), np.zeros((ns, ca), np.float32), np.zeros((ns, 2 * cr), np.float32)
    pc, na, nr = np.zeros(ns, np.uint32), C.c_uint32(), C.c_uint32()
    return pkg.load_library().sdrfm_bcast_process_batch_metered(
        bc._h, sink._h if sink is not None else None, iq.ctypes.data, iq.shape[1], nbytes, left.ctypes.data, right.ctypes.data, ca,
        pcm.ctypes.data if pcm is not None else None, 2 * ca, bb.ctypes.data, 2 * cr, pc.ctypes.data,
        meters.ctypes.data if meters is not None else None, C.byref(na), C.byref(nr), flags)


def test_every_refusal_leaves_the_next_call_unchanged(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, iq = su["ns"], np.ascontiguousarray(su["iq"])
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    m = np.full(ns, 3, pkg.METER_DTYPE)
    pcm = np.zeros((ns, 2 << 16), np.int16)
    EINVAL, EODD, ECAP = pkg.lib.EINVAL, pkg.lib.EODD, pkg.lib.ECAPACITY
    with _bcast(pkg, su["shape"], ns) as bc, pkg.StereoPcmSink(ns, alpha, gain) as sink:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        one = bc.process_batch_metered(iq)
        bc.reset()
        refusals = [(lambda: _raw(pkg, bc, iq, 1000, None), EINVAL),                            # meters NULL
                    (lambda: _raw(pkg, bc, iq, 1000, m, pcm=pcm), EINVAL),                      # pcm without sink
                    (lambda: _raw(pkg, bc, iq, 1000, m, flags=pkg.lib.F_OVERLAP), EINVAL),
                    (lambda: _raw(pkg, bc, iq, 1000, m, sink=sink, pcm=pcm, flags=pkg.lib.F_OVERLAP), EINVAL),
                    (lambda: _raw(pkg, bc, iq, 1001, m), EODD),                                 # odd bytes
                    (lambda: _raw(pkg, bc, iq, 1001, m, sink=sink, pcm=pcm), EODD),
                    (lambda: _raw(pkg, bc, iq, tc.NBYTES + 2, m), ECAP),
                    (lambda: _raw(pkg, bc, iq[:, :98], 100, m), ECAP)]                          # iq_stride < nbytes
        cuts = [2 * 3001] * len(refusals)
        cuts.append(tc.NBYTES - sum(cuts))
        state0 = sink.state()
        parts, acc, pos = ([], [], []), np.zeros(ns, pkg.METER_DTYPE), 0
        for k, c in enumerate(cuts):
            out = bc.process_batch_metered(iq[:, pos:pos + c]) if k % 2 else bc.process_batch(iq[:, pos:pos + c]) + (None,)
            for a, v in zip(parts, out[:3]):
                a.append(v)
            pos += c
            if k < len(refusals):
                call, want = refusals[k]
                assert call() == want, (k, want)
                assert (m["n"] == 3).all() and (m["reserved"] == 3).all()   # a refusal writes no record
        for a, o, what in zip(parts, one[:3], "LRw"):
            assert _same(np.concatenate(a, 1), o), what
        assert _same(sink.state(), state0)


def test_tap_sums_above_the_bounds_refuse_the_metered_call_only(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    shape, ns, iq, half = su["shape"], su["ns"], np.ascontiguousarray(su["iq"]), 2 * 30001
    h, b = tc.shape_taps(pkg, shape)[0], tc.shape_taps(pkg, shape)[3]
    m = np.zeros(ns, pkg.METER_DTYPE)
    # the configuration's h on an untuned handle: sum |h| > 16
    big_h = (h * np.float32(16.5 / np.abs(h.astype(np.float64)).sum())).astype(np.float32)
    assert np.abs(big_h.astype(np.float64)).sum() > 16.0
    with _bcast(pkg, shape, ns, h=big_h) as bc:
        one = bc.process_batch(iq)
        bc.reset()
        first = bc.process_batch(iq[:, :half])
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.EINVAL
        rest = bc.process_batch(iq[:, half:])
        for a, b_, o in zip(first[:3], rest[:3], one[:3]):
            assert _same(np.concatenate([a, b_], 1), o)
        # tuned within the bound, the same handle takes the metered call
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.OK and (m["n"] == 50).all()
        bc.tune()
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.EINVAL
    # tuned: one stream's sum(|hr| + |hi|) > 16
    big_t = np.ascontiguousarray(su["ctaps"], np.float32).copy()
    big_t[ns - 1] *= np.float32(16.5 / np.abs(big_t[ns - 1].astype(np.float64)).sum())
    assert np.abs(big_t[ns - 1].astype(np.float64)).sum() > 16.0 and np.abs(big_t[0].astype(np.float64)).sum() <= 16.0
    with _bcast(pkg, shape, ns) as bc:
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.OK             # untuned: the configuration's h is within the bound
        bc.tune(ctaps=big_t, rot=su["rot"])
        one = bc.process_batch(iq)
        bc.reset()
        first = bc.process_batch(iq[:, :half])
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.EINVAL
        with pytest.raises(pkg.SdrfmError) as e:
            bc.process_batch_metered(iq[:, :1000])
        assert e.value.status == pkg.lib.EINVAL
        rest = bc.process_batch(iq[:, half:])
        for a, b_, o in zip(first[:3], rest[:3], one[:3]):
            assert _same(np.concatenate([a, b_], 1), o)
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.OK
    # pilot taps: sum(|br| + |bi|) > 8, tuned or not
    bsum = float(np.abs(np.asarray(b).real.astype(np.float64)).sum() + np.abs(np.asarray(b).imag.astype(np.float64)).sum())
    big_b = (np.asarray(b, np.complex64) * np.float32(8.5 / bsum)).astype(np.complex64)
    assert float(np.abs(big_b.real.astype(np.float64)).sum() + np.abs(big_b.imag.astype(np.float64)).sum()) > 8.0
    with _bcast(pkg, shape, ns, b=big_b) as bc:
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.EINVAL
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        assert _raw(pkg, bc, iq, 1000, m) == pkg.lib.EINVAL
        assert bc.process_batch(iq)[0].shape[1] == tc.NBYTES // 2 // 10 // 5


def test_a_metered_call_takes_4_mib_at_the_most(pkg):
    shape, four = tc.SHAPES["default"], 4 << 20
    iq = pkg.make_iq(1, four // 2 + 1, mode="fm", first_id=9400)
    m = np.zeros(1, pkg.METER_DTYPE)
    with _bcast(pkg, shape, 1, nbytes=8 << 20) as bc:
        na, nr = bc.counts(four + 2)
        assert _raw(pkg, bc, iq, four + 2, m, ca=na + 1, cr=nr + 1) == pkg.lib.ECAPACITY
        assert bc.counts(four + 2) == (na, nr)                      # the refusal moved nothing
        L, R, bb, pc, rec = bc.process_batch_metered(iq[:, :four])
        assert int(rec["n"][0]) == four // 2 // 10 and int(rec["n_pilot"][0]) == int(pc[0])
        want = bc.counts(four + 2)
        assert bc.process_batch(iq[:, :four + 2])[0].shape[1] == want[0] > 0   # the plain call takes what max_bytes_per_call allows


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------
def test_a_drifted_receiver_finds_its_stations_again(pkg):
    """scenario "crystal+7kHz-and-mono": four streams on the grid candidates nearest the four stations, all reading the one capture.  n and
    rf_q are the reference's exactly (K2 holds no transcendental), freq_err_hz within 1 Hz of it (the device's arctangent; the bound of
    tests/test_scan_gpu.py), n_pilot within the count of d's at the gate; stream_status says what it says on the reference's records; tuned
    to its offsets, every stream is within 100 Hz (a tune restarts the streams: the second call starts from a zeroed state)"""
    name = "crystal+7kHz-and-mono"
    row, truth = sc.scenario_capture(pkg, name)
    truth = sorted(truth, key=lambda t: t["offset_hz"])
    offsets, ref_m, ref_rep = sc.scenario_reference(pkg, name)
    cand = [int(np.argmin(np.abs(offsets - t["offset_hz"]))) for t in truth]
    tuned = offsets[cand]
    h, b = sc.scenario_taps(pkg)
    assert row.size == 480000
    with _bcast(pkg, tc.SHAPES["default"], 4, pilot_min=sc.PILOT_MIN, nbytes=row.size) as bc:
        bc.tune(offsets_hz=tuned, fs=sc.FS, shared_input=True)
        assert bc.kernel_name.startswith("bcast-fast-tuned")
        L, R, bb, pc, m = bc.process_batch_metered(row)
        rep = pkg.meter_report(m, sc.FS, 10)
        for s, c in enumerate(cand):
            r = sr.scan_ref(row, pkg.tuned_channel_taps(h, offsets[c], sc.FS), pkg.tuned_rotation(offsets[c], sc.FS, 10), 10, b, sc.PILOT_MIN)
            assert r["rec"] == sr.rec_of(ref_m[c])
            amb = sr.ambiguous(r["pw"], r["pmin2"])
            lo = int(((r["pw"] >= r["pmin2"]) & ~amb).sum())
            print("stream %d at %+.0f Hz: freq_err %.2f Hz (reference %.2f), n_pilot %d in [%d, %d], pilot_count %d" % (
                s, tuned[s], rep["freq_err_hz"][s], ref_rep["freq_err_hz"][c], int(m["n_pilot"][s]), lo, lo + int(amb.sum()), int(pc[s])))
            assert int(m["n"][s]) == int(ref_m["n"][c]) == row.size // 2 // 10 and int(m["rf_q"][s]) == int(ref_m["rf_q"][c]), (s, m[s], ref_m[c])
            assert lo <= int(m["n_pilot"][s]) <= lo + int(amb.sum()) and int(m["n_pilot"][s]) == int(pc[s])
            assert abs(rep["freq_err_hz"][s] - ref_rep["freq_err_hz"][c]) <= 1.0, (s, rep["freq_err_hz"][s], ref_rep["freq_err_hz"][c])
        status = pkg.stream_status(rep, tuned)
        want = pkg.stream_status({k: v[cand] for k, v in ref_rep.items()}, tuned)
        for s, (st, w, t) in enumerate(zip(status, want, truth)):
            assert st["present"] is True and w["present"] is True and st["stereo"] is w["stereo"] is t["stereo"], (s, st, w, t)
            assert abs(st["offset_hz"] - t["offset_hz"]) < 100.0, (st, t)
        bc.tune(offsets_hz=[st["offset_hz"] for st in status], fs=sc.FS, shared_input=True)
        rep2 = pkg.meter_report(bc.process_batch_metered(row)[4], sc.FS, 10)
    assert np.abs(rep2["freq_err_hz"]).max() < 100.0, rep2["freq_err_hz"]
