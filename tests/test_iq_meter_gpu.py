"""The raw-capture IQ meter on the device, against the host routine sdrfm_iq_meter_u8 (which tests/test_iq_meter_cpu.py holds to the
numpy restatement of the definition).  Every comparison of records and rows is integer equality; nothing here has a tolerance.  Every case runs
record-only (k_iq_meter<false>) and with the histogram (k_iq_meter<true>).  Device buffers sit between canaries: the capture must come back as it
went in, and nothing before or behind meters and hist may change."""
import ctypes as C
import time

import numpy as np
import pytest

import iq_meter_cases as cases
import iq_meter_ref as ref

pytestmark = pytest.mark.gpu

FORMS = [False, True]
PAD = 256                    # canary bytes in front of and behind the capture
CANARY = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def geometry(pkg):
    return pkg.iqmeter.iq_meter_geometry


def _place(torch, rows, off=0, stride=None):
    """the rows in a device buffer of canaries: row s starts PAD + off + s * stride bytes into it.  Returns (buffer, a host copy, address of row 0)."""
    ns, nbytes = rows.shape
    stride = nbytes if stride is None else stride
    host = np.full(PAD + off + ns * stride + PAD, CANARY, np.uint8)
    for s in range(ns):
        host[PAD + off + s * stride:PAD + off + s * stride + nbytes] = rows[s]
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0                     # so that `off` IS the row's alignment
    return buf, host, buf.data_ptr() + PAD + off


class Outputs:
    """meters and hist on the device, one record and one row of canaries on either side"""

    def __init__(self, torch, ns, hist):
        self.ns = ns
        self.m = torch.full((8 * (ns + 2),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.h = torch.full((512 * (ns + 2),), 0x5B5B5B5B, dtype=torch.int32, device="cuda") if hist else None

    @property
    def meters_ptr(self):
        return self.m.data_ptr() + 64

    @property
    def hist_ptr(self):
        return None if self.h is None else self.h.data_ptr() + 2048

    def read(self, pkg):
        m = self.m.cpu().numpy()
        assert (m[:8] == 0x5A5A5A5A5A5A5A5A).all() and (m[-8:] == 0x5A5A5A5A5A5A5A5A).all(), "a record outside meters was written"
        rec = np.ascontiguousarray(m[8:-8]).view(pkg.IQ_METER_DTYPE)
        if self.h is None:
            return rec, None
        h = self.h.cpu().numpy()
        assert (h[:512] == 0x5B5B5B5B).all() and (h[-512:] == 0x5B5B5B5B).all(), "a row outside hist was written"
        return rec, np.ascontiguousarray(h[512:-512]).view(np.uint32).reshape(self.ns, 512)


def _device(pkg, torch, m, rows, hist, off=0, stride=None):
    """one device call on `rows` placed at (off, stride): (records, rows or None), the canaries and the capture checked"""
    buf, host, ptr = _place(torch, rows, off, stride)
    out = Outputs(torch, rows.shape[0], hist)
    m.process_batch_ptr(ptr, rows.shape[1] if stride is None else stride, rows.shape[1], out.meters_ptr, out.hist_ptr)
    m.synchronize()
    assert m.kernel_name == ("iq-meter-hist" if hist else "iq-meter")
    assert np.array_equal(buf.cpu().numpy(), host), "the capture or its canaries changed"
    return out.read(pkg)


def _same(pkg, got, rows, hist):
    want = pkg.iq_meter_host(rows, with_hist=True)
    if got[0].tobytes() != want[0].tobytes():
        return False
    return (got[1] is None) if not hist else np.array_equal(got[1].astype(np.uint64), want[1])


@pytest.mark.parametrize("hist", FORMS)
def test_small_rows_and_one_step(pkg, torch, hist):
    """around one and two vectors, and one step of a workgroup +- 2, on 3 streams"""
    x = cases.random_rows(61, 3, max(cases.STEP))
    with pkg.IqMeter(3) as m:
        for nbytes in cases.SMALL + cases.STEP:
            assert _same(pkg, _device(pkg, torch, m, x[:, :nbytes], hist, stride=nbytes), x[:, :nbytes], hist), nbytes


@pytest.mark.parametrize("hist", FORMS)
def test_a_workgroups_whole_share_on_65_streams(pkg, torch, geometry, hist):
    """32 workgroups per stream with a share of exactly three steps each, and that +- 2 bytes"""
    S = cases.share_bytes(geometry, 65)
    bps, share = geometry(65, S)
    assert bps > 1 and share == 3 * 256 and geometry(65, S + 2) == (bps, share)
    x = cases.random_rows(62, 65, S + 2)
    with pkg.IqMeter(65, S + 2) as m:
        for nbytes in (S - 2, S, S + 2):
            assert _same(pkg, _device(pkg, torch, m, x[:, :nbytes], hist, stride=S + 2), x[:, :nbytes], hist), nbytes


@pytest.mark.parametrize("hist", FORMS)
def test_row_offsets_and_odd_strides(pkg, torch, hist):
    """rows that start 0 .. 17 bytes behind a 256-byte aligned address, on odd strides: the streams' rows alternate between even and odd
    addresses, and every residue of 16 is the head of some row"""
    x = cases.random_rows(63, 3, cases.CHUNK + 34)
    with pkg.IqMeter(3) as m:
        for off in cases.OFFSETS:
            for nbytes, stride in ((cases.CHUNK + 34, cases.CHUNK + 71), (30, 31), (2, 3)):
                assert _same(pkg, _device(pkg, torch, m, x[:, :nbytes], hist, off, stride), x[:, :nbytes], hist), (off, nbytes, stride)


@pytest.mark.parametrize("hist", FORMS)
@pytest.mark.parametrize("value", [0, 255, 128])
def test_constant_rows_of_4_mib(pkg, torch, hist, value):
    """The one-bin case: every byte of the row counts into one bin per component.  The bound on the duration: with every count fully serialised on
    ONE compute unit at one LDS atomic per cycle and 1 GHz, 4 Mi counts take 4.2 ms; 20 ms leaves five times that for the launch and the
    synchronise.  A form that serialised worse than that, or spun, fails here rather than at a time limit."""
    n = 4 << 20
    d = torch.full((n,), value, dtype=torch.uint8, device="cuda")
    out = Outputs(torch, 1, hist)
    with pkg.IqMeter(1, n) as m:
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.process_batch_ptr(d.data_ptr(), n, n, out.meters_ptr, out.hist_ptr)
            m.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    rec, rows = out.read(pkg)
    p = n // 2
    rail = p if value in (0, 255) else 0
    assert ref.rec_tuple(rec[0]) == (p, p * value, p * value, p * value ** 2, p * value ** 2, p * value ** 2, rail, rail)
    if hist:
        want = np.zeros(512, np.uint32)
        want[value] = want[256 + value] = p
        assert np.array_equal(rows[0], want)
    print("constant %d, hist %s: %.3f ms" % (value, hist, 1e3 * best))
    assert best <= 20e-3, best


@pytest.mark.parametrize("hist", FORMS)
def test_64_mib_of_255_against_the_closed_form(pkg, torch, hist):
    """the overflow case for the lanes' 32-bit sums: the largest call there is, every byte at its largest"""
    n = 64 << 20
    d = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    out = Outputs(torch, 1, hist)
    with pkg.IqMeter(1, n) as m:
        m.process_batch_ptr(d.data_ptr(), n, n, out.meters_ptr, out.hist_ptr)
        m.synchronize()
    rec, rows = out.read(pkg)
    p = n // 2
    assert ref.rec_tuple(rec[0]) == (p, 255 * p, 255 * p, 65025 * p, 65025 * p, 65025 * p, p, p)
    if hist:
        assert int(rows[0, 255]) == p and int(rows[0, 511]) == p and int(rows[0].astype(np.uint64).sum()) == 2 * p


@pytest.mark.parametrize("hist", FORMS)
def test_ramp_of_all_pairs(pkg, torch, hist):
    x = cases.ramp()[None, :]
    with pkg.IqMeter(1) as m:
        got = _device(pkg, torch, m, x, hist)
    assert ref.rec_tuple(got[0][0]) == (65536, 256 * 32640, 256 * 32640, 256 * 5559680, 256 * 5559680, 32640 ** 2, 512, 512)
    assert _same(pkg, got, x, hist) and (not hist or (got[1] == 256).all())


@pytest.mark.parametrize("hist", FORMS)
def test_a_capture_cut_into_calls_adds_up(pkg, torch, hist):
    x = cases.random_rows(64, 3, 3 * cases.CHUNK + 10)
    total = x.shape[1]
    with pkg.IqMeter(3) as m:
        whole = _device(pkg, torch, m, x, hist)
        acc, hacc, at = np.zeros(3, pkg.IQ_METER_DTYPE), np.zeros((3, 512), np.uint64), 0
        for c in cases.CUTS + (total,):
            c = min(c, total - at)
            piece = x[:, at:at + c]
            got = _device(pkg, torch, m, piece, hist, stride=max(c, 1)) if c else _zero_call(pkg, torch, m, hist)
            assert _same(pkg, got, piece, hist), (at, c)
            pkg.iq_meter_add(acc, got[0])
            if hist:
                pkg.iq_hist_add(hacc, got[1])
            at += c
    assert at == total and acc.tobytes() == whole[0].tobytes()
    assert not hist or np.array_equal(hacc, whole[1].astype(np.uint64))


def _zero_call(pkg, torch, m, hist):
    """a device call of 0 bytes: zero records and rows, enqueued like any other"""
    out = Outputs(torch, m.n_streams, hist)
    m.process_batch_ptr(None, 0, 0, out.meters_ptr, out.hist_ptr)
    m.synchronize()
    rec, rows = out.read(pkg)
    assert not rec.tobytes().strip(b"\0") and (rows is None or not rows.any())
    return rec, rows


@pytest.mark.parametrize("hist", FORMS)
def test_eight_calls_back_to_back_on_a_callers_stream(pkg, torch, hist):
    """enqueued with no synchronise between them, on a stream the caller made; one synchronise behind them"""
    x = cases.random_rows(65, 3, 8 * 5000)
    stream = torch.cuda.Stream()
    placed = [_place(torch, x[:, 5000 * k:5000 * (k + 1)], off=k, stride=5001 + 2 * k) for k in range(8)]
    outs = [Outputs(torch, 3, hist) for _ in range(8)]
    torch.cuda.synchronize()
    with pkg.IqMeter(3) as m:
        m.set_stream(stream.cuda_stream)
        for k in range(8):
            m.process_batch_ptr(placed[k][2], 5001 + 2 * k, 5000, outs[k].meters_ptr, outs[k].hist_ptr)
        m.synchronize()
        for k in range(8):
            assert _same(pkg, outs[k].read(pkg), x[:, 5000 * k:5000 * (k + 1)], hist), k
        m.set_stream(None)                                # back on its own stream
        assert _same(pkg, _device(pkg, torch, m, x[:, :5000], hist, stride=5000), x[:, :5000], hist)


@pytest.mark.parametrize("hist", FORMS)
def test_host_buffers_against_device_buffers(pkg, torch, hist):
    x = cases.random_rows(66, 5, 2 * cases.CHUNK + 18)
    with pkg.IqMeter(5) as m:
        for nbytes in (x.shape[1], 18, 0, cases.CHUNK):      # (growing and shrinking: the staging is reused)
            host = m.process_batch(x[:, :nbytes], hist=hist)
            host = host if hist else (host, None)
            assert m.kernel_name == ("iq-meter-hist" if hist else "iq-meter")
            assert _same(pkg, host, x[:, :nbytes], hist), nbytes
            if nbytes:
                dev = _device(pkg, torch, m, x[:, :nbytes], hist, stride=nbytes)
                assert dev[0].tobytes() == host[0].tobytes() and (not hist or np.array_equal(dev[1], host[1]))
        d_iq = torch.from_numpy(x).cuda()                 # ... and the tensor form of the device call
        d_m = torch.zeros(8 * 5, dtype=torch.int64, device="cuda")
        d_h = torch.zeros(512 * 5, dtype=torch.int32, device="cuda") if hist else None
        m.process_batch_device(d_iq, d_m, d_h)
        m.synchronize()
        got = (d_m.cpu().numpy().view(pkg.IQ_METER_DTYPE), None if d_h is None else d_h.cpu().numpy().view(np.uint32).reshape(5, 512))
        assert _same(pkg, got, x, hist)


@pytest.mark.parametrize("hist", FORMS)
def test_host_staging_grows_and_is_reused_below_capacity(pkg, torch, hist):
    """host-buffer calls of 1000, 1025 and 3 byte-pairs in that order on one handle of 3 streams, then 2049 byte-pairs, the first length past the
    4096 bytes the staging is rounded up to, and 3 again: the staging is made, reused, outgrown, and used far below its capacity with the last
    call's bytes still behind the valid ones.  Every call's records and rows are the host routine's"""
    x = cases.random_rows(67, 3, 2 * 2049 + 8)
    with pkg.IqMeter(3) as m:
        for k, pairs in enumerate((1000, 1025, 3, 2049, 3)):
            rows = np.ascontiguousarray(x[:, k:k + 2 * pairs])
            got = m.process_batch(rows, hist=hist)
            assert _same(pkg, got if hist else (got, None), rows, hist), pairs


@pytest.mark.parametrize("hist", FORMS)
def test_one_stream_fills_the_machine_like_sixteen(pkg, torch, geometry, hist):
    """the shared-capture case: one row of 1 MiB on a 1-stream handle (256 workgroups) against a 16-stream handle given that row sixteen times"""
    row = cases.random_rows(67, 1, 1 << 20)
    assert geometry(1, 1 << 20)[0] == 256 and geometry(16, 1 << 20)[0] == 128
    with pkg.IqMeter(1) as one, pkg.IqMeter(16) as many:
        a = _device(pkg, torch, one, row, hist)
        b = _device(pkg, torch, many, np.repeat(row, 16, axis=0), hist)
    assert _same(pkg, a, row, hist)
    for s in range(16):
        assert b[0][s].tobytes() == a[0][0].tobytes() and (not hist or np.array_equal(b[1][s], a[1][0])), s


def test_a_demodulator_call_on_the_same_rows_and_stream_is_untouched(pkg, torch):
    """BroadcastDemod and the meter on the same device rows and the same stream, the meter between two demodulator calls: L, R, bb and the pilot
    counts bit for bit what they are without the meter, and the meter's records those of the bytes"""
    h, g = pkg.default_config(fir_taps=64)
    nbytes = 2 * 66000
    x = np.stack([pkg.make_iq_rds(1, 2 * nbytes // 2, pkg.rds_encode_groups(0x2200 + k, "IQM %02d" % k), first_id=730 + k)[0] for k in range(2)])
    cfg = dict(fir_coeffs=pkg.lowpass_taps(64, 120e3 / 2.4e6), pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), n_streams=2, max_bytes_per_call=nbytes,
               audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3), diff_gain=pkg.stereo_diff_gain(10, 2.4e6), rds_gain=pkg.rds_gain(10, 2.4e6))
    d_iq = torch.from_numpy(x).cuda()
    stream = torch.cuda.Stream()
    results = []
    for with_meter in (False, True):
        with pkg.BroadcastDemod(pkg.BroadcastConfig(**cfg)) as bc, pkg.IqMeter(2, nbytes) as m:
            na, nr = bc.counts(nbytes)
            outs = [[torch.zeros((2, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((2, na + 8), dtype=torch.float32, device="cuda"),
                     torch.zeros((2, 2 * nr + 8), dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")] for _ in range(2)]
            recs = [Outputs(torch, 2, True) for _ in range(2)]
            torch.cuda.synchronize()
            bc.set_stream(stream.cuda_stream)
            m.set_stream(stream.cuda_stream)
            for c in range(2):
                iq = d_iq[:, c * nbytes:(c + 1) * nbytes]
                bc.process_batch_device(iq, *outs[c], nbytes=nbytes)
                if with_meter:
                    m.process_batch_ptr(iq.data_ptr(), iq.stride(0), nbytes, recs[c].meters_ptr, recs[c].hist_ptr)
            bc.synchronize()
            results.append([[t.cpu().numpy() for t in o] for o in outs])
            if with_meter:
                for c in range(2):
                    assert _same(pkg, recs[c].read(pkg), x[:, c * nbytes:(c + 1) * nbytes], True), c
    for c in range(2):
        for a, b in zip(results[0][c], results[1][c]):
            assert a.tobytes() == b.tobytes()
    assert np.abs(results[0][1][0]).max() > 0.0
    assert np.array_equal(d_iq.cpu().numpy(), x)


def test_refusals_that_need_a_device(pkg, torch):
    L = pkg.lib
    lib = pkg.load_library()
    x = cases.random_rows(68, 2, 4096)
    d = torch.from_numpy(x).cuda()
    out = Outputs(torch, 2, True)
    rec, rows = np.zeros(2, pkg.IQ_METER_DTYPE), np.zeros((2, 512), np.uint32)
    with pkg.IqMeter(2, 4096) as m:
        call = lambda iq, stride, nbytes, meters, hist, flags: lib.sdrfm_iq_meter_process_batch(m._h, iq, stride, nbytes, meters, hist, flags)
        dp, mp, hp = d.data_ptr(), out.meters_ptr, out.hist_ptr
        assert call(dp, 4096, 4096, None, hp, L.F_DEVICE_PTRS) == L.EINVAL                      # NULL meters
        for flags in (L.F_OVERLAP, L.F_DEVICE_PTRS | L.F_OVERLAP, 4, 0x80000000):
            assert call(dp, 4096, 4096, mp, hp, flags) == L.EINVAL                              # SDRFM_F_OVERLAP and unknown flags
        assert call(dp, 4096, 4096, mp + 4, hp, L.F_DEVICE_PTRS) == L.EINVAL                    # meters not 8-byte aligned
        assert call(dp, 4096, 4096, mp, hp + 2, L.F_DEVICE_PTRS) == L.EINVAL                    # hist not 4-byte aligned
        assert call(dp, 4096, 4095, mp, hp, L.F_DEVICE_PTRS | L.F_OVERLAP) == L.EINVAL          # the flags come before the parity
        assert call(dp, 4096, 4095, mp, hp, L.F_DEVICE_PTRS) == L.EODD
        assert call(dp, 8192, 4099, mp, hp, L.F_DEVICE_PTRS) == L.EODD                          # ... and the parity before the capacity
        assert call(dp, 8192, 4098, mp, hp, L.F_DEVICE_PTRS) == L.ECAPACITY                     # over the maximum
        assert call(dp, 4094, 4096, mp, hp, L.F_DEVICE_PTRS) == L.ECAPACITY                     # rows that overlap
        assert call(None, 4096, 4096, mp, hp, L.F_DEVICE_PTRS) == L.EINVAL                      # NULL iq
        assert call(x.ctypes.data, 4095, 4096, rec.ctypes.data, rows.ctypes.data, 0) == L.ECAPACITY
        assert call(None, 4096, 4096, rec.ctypes.data, None, 0) == L.EINVAL
        m.synchronize()
        got = out.read(pkg)                                                                     # nothing was written by a refused call
        assert (got[0].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all() and (got[1] == 0x5B5B5B5B).all() and not rec.tobytes().strip(b"\0")
        assert call(dp, 4096, 4096, mp, hp, L.F_DEVICE_PTRS) == L.OK                            # and the handle still works
        m.synchronize()
        assert _same(pkg, out.read(pkg), x, True)
        assert call(dp, 4096, 0, mp, None, L.F_DEVICE_PTRS) == L.OK                             # nbytes == 0: zero records, hist left alone
        m.synchronize()
        got = out.read(pkg)
        assert not got[0].tobytes().strip(b"\0") and _same(pkg, (pkg.iq_meter_host(x), got[1]), x, True)
    with pkg.IqMeter(1, 4096) as one:                                                           # one stream: the stride is not looked at
        r = np.zeros(1, pkg.IQ_METER_DTYPE)
        assert lib.sdrfm_iq_meter_process_batch(one._h, x.ctypes.data, 0, 4096, r.ctypes.data, None, 0) == L.OK
        assert r.tobytes() == pkg.iq_meter_host(x[0]).tobytes()
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.IqMeter(1, device=99)
    assert e.value.status == L.NO_DEVICE
