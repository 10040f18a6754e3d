"""GPU sweep of the scan handle's hist call (sdrfm_scan_process_batch_hist) over the shapes of tests/test_scan_shapes_gpu.py
and the default one on the generic kernel: P = 1 (no carried d's), T = 1, D = 1, T = 256, and the four shapes whose step the LDS budget
cuts — there the bins take LDS from the step, so the hist call walks in shorter steps than the plain call and must give the same integers.
Per shape, 1 / 3 / 7 streams, rows as integers: exactly the numpy bincount of the device's own d at offset 0, the records equal to the
plain call's, and a ragged sequence of calls (with the long call of 128 plain steps' worth of d's) summed with sdrfm_scan_hist_add against
the one call.  Then the top of the range: 4 MiB a stream at T = 1, D = 1 — 2^21 counts in one bin, and both extreme bins."""
import numpy as np
import pytest

import pilot_shape_cases as ps
import scan_hist_cases as hc
from test_scan_shapes_gpu import _handle, _records_equal
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

BINS = hc.BINS
DEFAULT = (64, 10, 101)
SHAPES = ps.SCAN_SHAPES + [DEFAULT]
SHAPE_IDS = [ps.scan_id(s) for s in SHAPES]
_default = {}


def _case(pkg, shape):
    """tests/pilot_shape_cases.py's case of a shape (its references are not used here); the default shape gets one made the same way"""
    if shape != DEFAULT:
        return ps.scan_case(pkg, shape)
    if not _default:
        T, D, P = shape
        idx, ns, step = len(ps.SCAN_SHAPES), 3, ps.scan_step(shape)
        cuts, long_ = ps.ragged_cuts(D, step["H"], step["NDT"], ns, (), 600 + idx)
        names, cycles, iq, h, ctaps, rot = ps._front(pkg, T, D, ns, idx, sum(cuts) // 2, 7600)
        _default.update(shape=shape, idx=idx, ns=ns, names=names, cycles=cycles, iq=iq, h=h, b=ps.pilot_taps(pkg, shape), ctaps=ctaps, rot=rot, cuts=cuts,
                        long=long_, step=step)
    return _default


def _check_rows(meters, hist):
    assert hist.dtype == np.uint32 and hist.shape == (meters.size, BINS)
    assert not hist[:, :54].any() and not hist[:, 458:].any(), np.flatnonzero(hist.sum(0))
    assert (hist.sum(1, dtype=np.uint64) == meters["n"]).all(), (hist.sum(1), meters["n"])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_offset_zero_rows_are_exact_on_the_devices_own_d(pkg, shape):
    """taps (h, 0) and rot 0 give the untuned d bit for bit; the bit-exact mono handle with a one-tap unit audio filter hands that d back.
    One call over the case's whole input: more than the long call of 128 plain steps' worth of d's"""
    case = _case(pkg, shape)
    T, D, P = shape
    ns, iq, h, b, nbytes = case["ns"], case["iq"], case["h"], case["b"], case["iq"].shape[1]
    ndt_plain, ndt_hist = hc.step_of(hc.scan_lds, shape)[0], hc.step_of(hc.hist_lds, shape)[0]
    assert ndt_plain == case["step"]["NDT"] and (ndt_hist < ndt_plain) == (shape in ps.SCAN_LDS_LIMITED), (ndt_plain, ndt_hist)
    assert nbytes // 2 // D >= case["long"] // 2 // D >= 6 * ndt_plain
    one = np.ones(1, np.float32)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True, max_bytes_per_call=nbytes)) as mono:
        d = mono.process_batch(iq)
    hz = np.tile(pairs(h), (ns, 1))
    with _handle(pkg, shape, b, hz, np.zeros(ns, np.float32), 0.05, nbytes) as scn, _handle(pkg, shape, b, hz, np.zeros(ns, np.float32), 0.05, nbytes) as pl:
        m, hist = scn.process_batch_hist(iq)
        assert scn.kernel_name == "scan-generic T%d D%d P%d + hist" % shape
        want_m = pl.process_batch(iq)
    _records_equal(m, want_m, "the hist call's records against the plain call's")
    _check_rows(m, hist)
    for s in range(ns):
        want = hc.hist_of(d[s])
        assert np.array_equal(hist[s].astype(np.uint64), want), (shape, s, case["names"][s], np.flatnonzero(hist[s] != want))
    print("scan-generic T%d D%d P%d + hist at offset 0: %d streams x %d d's, steps of %d d's (the plain call's: %d), bins in use %s: exact on the device's own d" % (
        shape + (ns, d.shape[1], ndt_hist, ndt_plain, [int(np.count_nonzero(r)) for r in hist])))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_ragged_calls_add_up_to_the_one_call(pkg, shape):
    """the case's cuts at its tuned offsets — 0 and 2 bytes, a call whose M is below H, a call that leaves the input phase off 0, the long
    call of three workgroups a stream and two full steps a workgroup, random ones — as hist calls with every third a plain one in between"""
    case = _case(pkg, shape)
    ns, iq, cuts = case["ns"], case["iq"], case["cuts"]
    with _handle(pkg, shape, case["b"], case["ctaps"], case["rot"], 0.05, iq.shape[1]) as scn:
        m1, h1 = scn.process_batch_hist(iq)
        scn.reset()
        acc, rows, pos = np.zeros(ns, pkg.METER_DTYPE), np.zeros((ns, BINS), np.uint64), 0
        for c in cuts:
            m, hist = scn.process_batch_hist(iq[:, pos:pos + c])
            _check_rows(m, hist)
            pkg.meter_add(acc, m)
            pkg.hist_add(rows, hist)
            pos += c
        scn.reset()
        rows2, pos = np.zeros((ns, BINS), np.uint64), 0
        for i, c in enumerate(cuts):                                 # the same cuts, every third call a plain one: its d's are left out
            if i % 3 == 1 and c != case["long"]:
                scn.process_batch(iq[:, pos:pos + c])
            else:
                pkg.hist_add(rows2, scn.process_batch_hist(iq[:, pos:pos + c])[1])
            pos += c
        scn.reset()
        left_out, pos = np.zeros((ns, BINS), np.uint64), 0
        for i, c in enumerate(cuts):                                 # what the plain calls left out, from a third pass with the roles swapped
            if i % 3 == 1 and c != case["long"]:
                pkg.hist_add(left_out, scn.process_batch_hist(iq[:, pos:pos + c])[1])
            else:
                scn.process_batch(iq[:, pos:pos + c])
            pos += c
    _check_rows(m1, h1)
    _records_equal(acc, m1, "the cuts summed")
    assert np.array_equal(rows, h1.astype(np.uint64)), (shape, np.flatnonzero((rows != h1).any(0)))
    assert np.array_equal(rows2 + left_out, rows), shape
    assert (m1["n"] == iq.shape[1] // 2 // shape[1]).all()


def test_top_of_the_range(pkg):
    """T = 1, D = 1, 4 MiB a stream, n = 2^21: stream 0's constant bytes put every count into bin 256 — the largest count a bin can hold,
    all of it added to one LDS word —; stream 1's d's are +-(pi - 3.1e-5) in turn, the two extreme bins 457 and 54; stream 2's phase falls
    2.5 rad a sample.  Every row exact against the device's own d"""
    iq = hc.top_case()
    h, b, one, n = np.array([1.0], np.float32), np.array([2, -2, 2, -1, 1], np.complex64), np.ones(1, np.float32), 1 << 21
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=1, audio_decim=1, n_streams=3, bit_exact=True,
                                  max_bytes_per_call=hc.TOP_BYTES)) as mono:
        d = mono.process_batch(iq)
    assert d.shape == (3, n)
    with _handle(pkg, hc.TOP_SHAPE, b, np.tile(pairs(h), (3, 1)), np.zeros(3, np.float32), 0.05, hc.TOP_BYTES) as scn:
        assert scn.kernel_name == "scan-generic T1 D1 P5"
        m, hist = scn.process_batch_hist(iq)
    _check_rows(m, hist)
    assert (m["n"] == n).all()
    for s in range(3):
        assert np.array_equal(hist[s].astype(np.uint64), hc.hist_of(d[s])), (s, np.flatnonzero(hist[s]))
    assert int(hist[0, 256]) == n and np.count_nonzero(hist[0]) == 1
    # d[0] of stream 1 is 0 (no sample before it); the others alternate between the two extreme bins
    assert int(hist[1, 256]) == 1 and int(hist[1, 54]) + int(hist[1, 457]) == n - 1 and abs(int(hist[1, 54]) - int(hist[1, 457])) <= 1, np.flatnonzero(hist[1])
    assert int(np.argmax(hist[2])) in (95, 96), np.flatnonzero(hist[2])   # d = -2.5 rad is the edge between the two
    print("scan-generic T1 D1 P5 + hist: bin 256 holds %d; bins 54 and 457 hold %d and %d; the falling phase sits in bin %d" % (
        hist[0, 256], hist[1, 54], hist[1, 457], int(np.argmax(hist[2]))))
