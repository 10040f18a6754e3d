"""GPU sweep of the scan handle (sdrfm_scan_*) over its configuration space: the shapes of tests/pilot_shape_cases.py — P = 1
(no carried d's), T = 1 (no carried samples), D = 1, D = 64, T = 256, and the four whose step the LDS budget cuts below 1023 d's — each
with a call of three workgroups a stream and two full steps a workgroup.  Records are compared as integers, field by field: against
tests/scan_ref.py from bytes at the tuned offsets (the bounds of tests/test_scan_gpu.py), exactly against the device's own d at offset 0,
a ragged sequence of calls against the one call, one stream against seven on one row, and the call forms (unaligned device rows, a record
array 8 bytes into its allocation, the caller's stream, one stream with a short iq_stride).  Then the record at the top of its range: taps
on the refusal bounds and 4 MiB of full-scale input, where pw 2^24 passes 2^33 and a 32-bit conversion would not do."""
import ctypes as C

import numpy as np
import pytest

import pilot_shape_cases as ps
import scan_cases as sc
import scan_ref as sr
from rds_ref import rds_ref
from test_bcast_shapes_gpu import _split
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

TOL_D = 1e-5                                                    # the project's tolerance on d (radians): the device's arctangent
FIELDS = ("n", "n_pilot", "rf_q", "freq_q", "dev_q", "pilot_q", "pilot2_q")
SHAPE_IDS = [ps.scan_id(s) for s in ps.SCAN_SHAPES]
FORMS = ["T7-D3-P5", "default", (256, 64, 255)]                 # two cases of tests/scan_cases.py and an LDS-limited shape


def _handle(pkg, shape, b, ctaps, rot, pilot_min, nbytes, generic=True, shared=False):
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=b, ctaps=ctaps, rot=rot, pilot_min=float(pilot_min), fir_decim=shape[1], shared_input=shared,
                                        max_bytes_per_call=nbytes, force_generic=generic))


def _records_equal(got, want, where):
    """two METER_DTYPE arrays as integers, field by field; reserved is 0"""
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.shape, want.shape)
    for s in range(got.size):
        for f in FIELDS:
            assert int(got[f][s]) == int(want[f][s]), (where, "stream %d" % s, f, int(got[f][s]), int(want[f][s]))
    assert (got["reserved"] == 0).all(), (where, got["reserved"])


def _in_calls(pkg, scn, iq, cuts):
    """the calls one after the other, their records summed with sdrfm_scan_meter_add"""
    acc, pos = np.zeros(scn.n_streams, pkg.METER_DTYPE), 0
    for c in cuts:
        m = scn.process_batch(iq[:, pos:pos + c])
        assert (m["reserved"] == 0).all() and (m["n"] == m["n"][0]).all(), (c, m)
        if c == 0:
            assert not m.tobytes().strip(b"\0")
        pkg.meter_add(acc, m)
        pos += c
    assert pos == iq.shape[1]
    return acc


def _exact_on_d(ds, b, pilot_min, first=0):
    """the record of the d's [first, ...) of a stream from the device's own d: freq_q and dev_q are numpy fp32 on it, pilot_q, pilot2_q and
    n_pilot come from tests/rds_ref.py's fp32-faithful pw on it"""
    f32, q24, q20 = np.float32, np.float32(2.0 ** 24), np.float32(2.0 ** 20)
    fix = lambda term, scale: int(np.rint((term * scale).astype(f32)).astype(np.int64).sum())
    ref = rds_ref(ds, b, np.ones(1, f32), pilot_min, 1.0, Dr=1)
    pw, ds = ref["pw"].astype(f32)[first:], ds.astype(f32)[first:]
    return dict(n=ds.size, n_pilot=int(ref["on"][first:].sum()), freq_q=fix(ds, q24), dev_q=fix((ds * ds).astype(f32), q24), pilot_q=fix(pw, q24),
                pilot2_q=fix((pw * pw).astype(f32), q20))


# ---- 1. against the reference from bytes, at the tuned offsets -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.SCAN_SHAPES, ids=SHAPE_IDS)
def test_tuned_offsets_against_the_reference(pkg, shape):
    """the form and the bounds of tests/test_scan_gpu.py::test_tuned_offsets_against_the_reference: n and rf_q equal, n_pilot within the count
    of d's at the gate, the means of d, e, pw and g within what TOL_D on d allows"""
    case = ps.scan_case(pkg, shape)
    b = np.asarray(case["b"], np.complex128)
    sum_b = float(np.abs(b).sum())
    with _handle(pkg, shape, case["b"], case["ctaps"], case["rot"], case["pilot_min"], case["iq"].shape[1]) as scn:
        name = scn.kernel_name
        assert name == ps.scan_name(shape, True) == "scan-generic T%d D%d P%d" % shape, name
        got = scn.process_batch(case["iq"])
    for s, r in enumerate(case["refs"]):
        have, want, n = sr.rec_of(got[s]), r["rec"], r["d"].size
        amb = sr.ambiguous(r["pw"], r["pmin2"])
        lo = int(((r["pw"] >= r["pmin2"]) & ~amb).sum())
        qmax = float(np.sqrt(r["pw"].astype(np.float64).max()))
        tol_pw = 2.0 * qmax * sum_b * TOL_D
        tol_g = 2.0 * qmax * qmax * tol_pw + 2.0 ** -20
        err = {k: abs(have[k] - want[k]) / n / 2.0 ** sh for k, sh in (("freq_q", 24), ("dev_q", 24), ("pilot_q", 24), ("pilot2_q", 20))}
        print("%s stream %d (%s at %+.4f): rf_q %s, n_pilot %d in [%d, %d], mean errors d %.3g (%.3g) e %.3g (%.3g) pw %.3g (%.3g) g %.3g (%.3g), "
              "%.3f %% of the d's at the gate" % (
                  name, s, case["names"][s], case["cycles"][s], "equal" if have["rf_q"] == want["rf_q"] else "%d != %d" % (have["rf_q"], want["rf_q"]),
                  have["n_pilot"], lo, lo + int(amb.sum()), err["freq_q"], TOL_D, err["dev_q"], 2 * np.pi * TOL_D, err["pilot_q"], tol_pw,
                  err["pilot2_q"], tol_g, 100 * amb.mean()))
        assert amb.mean() <= sc.EXCLUDED_CAP
        assert have["n"] == want["n"] == n and have["reserved"] == 0
        assert have["rf_q"] == want["rf_q"], (name, s, have["rf_q"], want["rf_q"])
        assert lo <= have["n_pilot"] <= lo + int(amb.sum()), (name, s, have["n_pilot"], lo, int(amb.sum()))
        assert err["freq_q"] <= TOL_D and err["dev_q"] <= 2 * np.pi * TOL_D, (name, s, err)
        assert err["pilot_q"] <= tol_pw and err["pilot2_q"] <= tol_g, (name, s, err, tol_pw, tol_g)


def test_the_fast_kernel_is_claimed_at_one_shape_only(pkg):
    for shape in ps.SCAN_SHAPES + [(64, 10, 101)]:
        hz = pairs(pkg.lowpass_taps(shape[0], 0.05))[None, :]
        with _handle(pkg, shape, ps.pilot_taps(pkg, shape), hz, np.zeros(1, np.float32), 0.05, 1 << 16, generic=False) as scn:
            assert scn.kernel_name == ps.scan_name(shape, False), (shape, scn.kernel_name)
            assert scn.kernel_name.startswith("scan-fast") == (shape == (64, 10, 101))


# ---- 2. exact against the device's own d at offset 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.SCAN_SHAPES, ids=SHAPE_IDS)
def test_offset_zero_record_is_exact_on_the_devices_own_d(pkg, shape):
    """taps (h, 0) and rot 0 give the untuned d bit for bit; the bit-exact mono handle with a one-tap unit audio filter hands that d back.
    Every field but rf_q follows from it exactly (rf_q is tests/scan_ref.py's), and n_pilot is the untuned broadcast handle's pilot_count
    as well.  The threshold lies in the middle of the rows' pilot powers at offset 0."""
    case = ps.scan_case(pkg, shape)
    T, D, P = shape
    ns, iq, h, b, nbytes = case["ns"], case["iq"], case["h"], case["b"], case["iq"].shape[1]
    pilot_min = ps.offset_zero_gate(case, b)
    one = np.ones(1, np.float32)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True, max_bytes_per_call=nbytes)) as mono:
        d = mono.process_batch(iq)
    with pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=one, rds_coeffs=one, pilot_coeffs=b, pilot_min=pilot_min, fir_decim=D,
                                                audio_decim=1, rds_decim=1, n_streams=ns, max_bytes_per_call=nbytes, force_generic=True)) as bc:
        pc = bc.process_batch(iq)[3]
    hz = np.tile(pairs(h), (ns, 1))
    with _handle(pkg, shape, b, hz, np.zeros(ns, np.float32), pilot_min, nbytes) as scn:
        got = scn.process_batch(iq)
    for s in range(ns):
        want = _exact_on_d(d[s], b, pilot_min)
        want["rf_q"] = sr.scan_ref(iq[s], hz[s], 0.0, D, b, pilot_min)["rec"]["rf_q"]
        have = sr.rec_of(got[s])
        for k, v in want.items():
            assert have[k] == v, (shape, s, case["names"][s], k, have[k], v)
        assert have["n_pilot"] == int(pc[s]) and have["reserved"] == 0, (s, have["n_pilot"], int(pc[s]))
    assert any(0 < int(v) < d.shape[1] for v in got["n_pilot"]), (got["n_pilot"], d.shape[1])
    print("scan-generic T%d D%d P%d at offset 0: pilot_min %.4g, n %d, n_pilot %s: every field exact on the device's own d" % (
        shape + (pilot_min, d.shape[1], [int(v) for v in got["n_pilot"]])))


# ---- 3. a ragged sequence of calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.SCAN_SHAPES, ids=SHAPE_IDS)
def test_ragged_calls_add_up_to_the_one_call(pkg, shape):
    """the case's cuts — 0 and 2 bytes, a call whose M is below H, a call that leaves the input phase off 0, the long call of three
    workgroups a stream and two full steps a workgroup, random ones — summed with sdrfm_scan_meter_add are the one call's record"""
    import torch
    case = ps.scan_case(pkg, shape)
    T, D, P = shape
    st, ns, cuts = case["step"], case["ns"], case["cuts"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M_long = case["long"] // 2 // D
    for per_cu in ps.PER_CU:
        bps, span = _split(M_long, st["NDT"], st["H"], ns, per_cu * cus)
        assert bps >= 3 and span >= 2 * st["NDT"], (per_cu, cus, bps, span, st)
    if st["H"] >= 4:
        assert any(0 < c // 2 // D < st["H"] for c in cuts)
    pilot_min = ps.mid_gate(case["names"], [r["pw"] for r in case["refs"]])
    with _handle(pkg, shape, case["b"], case["ctaps"], case["rot"], pilot_min, case["iq"].shape[1]) as scn:
        one = scn.process_batch(case["iq"])
        scn.reset()
        seq = _in_calls(pkg, scn, case["iq"], cuts)
        scn.reset()
        again = scn.process_batch(case["iq"])
    _records_equal(seq, one, "the cuts summed")
    _records_equal(again, one, "after a reset")
    assert (one["n"] == case["iq"].shape[1] // 2 // D).all()
    assert [int(v) for v in one["rf_q"]] == [r["rec"]["rf_q"] for r in case["refs"]]
    assert any(0 < int(v) < int(one["n"][0]) for v in one["n_pilot"]), one["n_pilot"]
    print("scan-generic T%d D%d P%d: %d streams, %d calls (the long one %d d's: %d steps of %d) add up to the one call, n_pilot %s of %d" % (
        shape + (ns, len(cuts), M_long, M_long // st["NDT"], st["NDT"], [int(v) for v in one["n_pilot"]], int(one["n"][0]))))


# ---- 4. the stream count -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.SCAN_SHAPES, ids=SHAPE_IDS)
def test_one_stream_and_seven_on_one_row_give_the_same_record(pkg, shape):
    """seven tunings (the five offsets in turn) on the case's first row, shared; then every distinct tuning alone on that row"""
    case = ps.scan_case(pkg, shape)
    T, D, P = shape
    fs, row = case["fs"], case["iq"][0:1]
    cyc = [sc.OFFSETS[(s + case["idx"]) % len(sc.OFFSETS)] for s in range(7)]
    ctaps = np.stack([pkg.tuned_channel_taps(case["h"], c * fs, fs) for c in cyc])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cyc], np.float32)
    pilot_min = ps.mid_gate(case["names"], [r["pw"] for r in case["refs"]])
    with _handle(pkg, shape, case["b"], ctaps, rot, pilot_min, row.shape[1], shared=True) as scn:
        seven = scn.process_batch(row)
    for s in range(5):
        with _handle(pkg, shape, case["b"], ctaps[s:s + 1], rot[s:s + 1], pilot_min, row.shape[1], shared=True) as scn:
            alone = scn.process_batch(row)
        _records_equal(alone, seven[s:s + 1], "tuning %d alone" % s)
        if s + 5 < 7:
            _records_equal(seven[s + 5:s + 6], seven[s:s + 1], "tuning %d twice" % s)
    assert T == 1 or len({m.tobytes() for m in seven[:5]}) == 5     # (the tunings do see different things; with one tap rot alone differs)


# ---- 5. the call forms ---------------------------------------------------------------------------------------------------------------
def _form_case(pkg, form):
    """(shape, b, ctaps, rot, pilot_min, iq) of a case of tests/scan_cases.py or of an LDS-limited shape"""
    if isinstance(form, str):
        su = sc.case_setup(pkg, next(c for c in sc.CASES if c[0] == form and c[1] > 1))
        return su["shape"], su["b"], su["ctaps"], su["rot"], su["pilot_min"], su["iq"]
    case = ps.scan_case(pkg, form)
    return form, case["b"], case["ctaps"], case["rot"], ps.mid_gate(case["names"], [r["pw"] for r in case["refs"]]), case["iq"]


@pytest.mark.parametrize("form", FORMS, ids=[f if isinstance(f, str) else ps.scan_id(f) for f in FORMS])
def test_call_forms_give_the_host_calls_records(pkg, form):
    import torch
    shape, b, ctaps, rot, pilot_min, iq = _form_case(pkg, form)
    ns, nbytes = iq.shape
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    assert ns > 1 and nbytes % 2 == 0
    with _handle(pkg, shape, b, ctaps, rot, pilot_min, nbytes, generic=shape != (64, 10, 101)) as scn:
        want = scn.process_batch(iq)
        assert any(0 < int(v) < int(want["n"][0]) for v in want["n_pilot"]) and len({m.tobytes() for m in want}) > 1
        # device rows cut from a larger allocation at byte offsets 2 / 6 / 14 with strides that are no multiple of 16; the records 8 bytes
        # into their allocation, canary records before and after them
        for off, pad in ((2, 2), (6, 6), (14, 10)):
            stride = nbytes + pad + (4 if (nbytes + pad) % 16 == 0 else 0)
            assert stride % 16 != 0 and (off % 16, stride % 2) == (off, 0)
            buf = torch.full((ns * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            for s in range(ns):
                buf[off + s * stride:off + s * stride + nbytes] = torch.from_numpy(iq[s].copy()).cuda()
            words = torch.full((8 * (ns + 2) + 1,), -7, dtype=torch.int64, device="cuda")
            assert words.data_ptr() % 64 == 0
            torch.cuda.synchronize()
            scn.reset()
            rc = lib.sdrfm_scan_process_batch(scn._h, C.c_void_p(buf.data_ptr() + off), stride, nbytes, C.c_void_p(words.data_ptr() + 64 + 8), DEV)
            assert rc == pkg.lib.OK, rc
            scn.synchronize()
            host = words.cpu().numpy()
            assert (host[:9] == -7).all() and (host[9 + 8 * ns:] == -7).all(), (off, host[:9], host[9 + 8 * ns:])
            _records_equal(np.ascontiguousarray(host[9:9 + 8 * ns]).view(pkg.METER_DTYPE).reshape(ns), want, "device rows at byte %d, stride %d" % (off, stride))
            hb = buf.cpu().numpy()
            assert (hb[:off] == 0xA5).all() and (hb[off + (ns - 1) * stride + nbytes:] == 0xA5).all()
            assert all((hb[off + s * stride + nbytes:off + (s + 1) * stride] == 0xA5).all() for s in range(ns - 1))
        # the caller's stream
        rows = torch.from_numpy(iq.copy()).cuda()
        d_m = torch.full((ns, 8), -7, dtype=torch.int64, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        scn.reset()
        scn.set_stream(stream.cuda_stream)
        scn.process_batch_device(rows, d_m)
        scn.synchronize()
        stream.synchronize()
        _records_equal(d_m.cpu().numpy().view(pkg.METER_DTYPE).reshape(ns), want, "the caller's stream")
        scn.reset()                                                  # (on the caller's stream as well)
        _records_equal(scn.process_batch(iq), want, "a host call on the caller's stream")
        scn.set_stream(None)
        scn.reset()
        _records_equal(scn.process_batch(iq), want, "back on the handle's own stream")
    # one stream: iq_stride is not read and may be anything, on host and on device buffers
    with _handle(pkg, shape, b, ctaps[1:2], rot[1:2], pilot_min, nbytes, generic=shape != (64, 10, 101)) as scn:
        row = np.ascontiguousarray(iq[1])
        d_row = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        d_row[6:6 + nbytes] = torch.from_numpy(row).cuda()
        torch.cuda.synchronize()
        for stride in (0, 2, nbytes - 2):
            m = np.zeros(1, pkg.METER_DTYPE)
            scn.reset()
            assert lib.sdrfm_scan_process_batch(scn._h, row.ctypes.data, stride, nbytes, m.ctypes.data, 0) == pkg.lib.OK
            _records_equal(m, want[1:2], "one stream, host, iq_stride %d" % stride)
            d_m = torch.full((3, 8), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            scn.reset()
            assert lib.sdrfm_scan_process_batch(scn._h, C.c_void_p(d_row.data_ptr() + 6), stride, nbytes, C.c_void_p(d_m.data_ptr() + 64), DEV) == pkg.lib.OK
            scn.synchronize()
            host = d_m.cpu().numpy()
            assert (host[0] == -7).all() and (host[2] == -7).all()
            _records_equal(np.ascontiguousarray(host[1]).view(pkg.METER_DTYPE).reshape(1), want[1:2], "one stream, device, iq_stride %d" % stride)


# ---- 6. the record at the top of its range -------------------------------------------------------------------------------------------
def test_record_at_the_top_of_its_range_is_exact(pkg):
    """tests/pilot_shape_cases.py's magnitude case on the generic scan kernel: a first call fills the pilot filter's history, then 4 MiB a
    stream, n = 2^21.  Every field is exact against the device's own d (rf_q against tests/scan_ref.py): pw 2^24 reaches 2^33.2, g 2^20
    reaches 2^38.5, pilot2_q 2^59.5, and stream 1's freq_q is below -2^46.  With the gate at 1e-18 every d passes, at 1e3 none does."""
    m = ps.magnitude_case(pkg)
    iq, first, one = m["iq"], ps.MAG_WARM // 2, np.ones(1, np.float32)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=m["h"], audio_coeffs=one, fir_decim=1, audio_decim=1, n_streams=2, bit_exact=True,
                                  max_bytes_per_call=ps.MAG_BYTES)) as mono:
        d = np.concatenate([mono.process_batch(iq[:, :ps.MAG_WARM]), mono.process_batch(iq[:, ps.MAG_WARM:])], 1)
    assert d.shape == (2, first + (1 << 21))
    for gate in ps.MAG_GATES:
        with _handle(pkg, ps.MAG_SHAPE, m["b"], m["ctaps"], m["rot"], gate, ps.MAG_BYTES) as scn:
            assert scn.kernel_name == "scan-generic T1 D1 P5"
            warm = scn.process_batch(iq[:, :ps.MAG_WARM])
            got = scn.process_batch(iq[:, ps.MAG_WARM:])
        assert (warm["n"] == first).all()
        for s in range(2):
            want = _exact_on_d(d[s], m["b"], gate, first)
            want["rf_q"] = m["refs"][s]["rec"]["rf_q"]
            have = sr.rec_of(got[s])
            print("scan-generic T1 D1 P5, gate %g, stream %d: n %d, n_pilot %d, rf_q 2^%.2f, freq_q %d, pilot_q 2^%.2f, pilot2_q 2^%.2f" % (
                gate, s, have["n"], have["n_pilot"], np.log2(have["rf_q"]), have["freq_q"], np.log2(max(have["pilot_q"], 1)), np.log2(max(have["pilot2_q"], 1))))
            for k, v in want.items():
                assert have[k] == v, (gate, s, k, have[k], v)
            assert have["n"] == 1 << 21 and have["n_pilot"] == (have["n"] if gate == ps.MAG_GATES[0] else 0) and have["reserved"] == 0
        # the magnitudes the case is there for, on the device's record
        assert int(got["pilot_q"][0]) >= 2 ** 54 and int(got["pilot2_q"][0]) >= 2 ** 59 and int(got["freq_q"][1]) <= -2 ** 46
