"""GPU sweep of the tuned and the metered broadcast kernels (sdrfm_bcast_tune, sdrfm_bcast_process_batch_metered)
over the configuration space tests/test_bcast_shapes_gpu.py sweeps the untuned kernels over, and one shape more: every shape of
tests/pilot_shape_cases.py on the generic kernels, and on the fast ones where the handle claims them.  Offset 0 is the untuned handle bit
for bit — at T256 D64 P255 Ta256 Tr256 the two walk in steps of 205 and 201 d's —, the tuned fast kernel is the tuned generic one, the
offsets that differ are held to tests/tuned_ref.py at the bound of tests/test_bcast_tuned_gpu.py, a ragged sequence of plain, metered and
alternating calls is the one call, a metered call's records are the scan handle's and its outputs a plain call's, on host buffers and on
unaligned device rows; and the metered record at the top of its range (tests/test_scan_shapes_gpu.py's method)."""
import ctypes as C

import numpy as np
import pytest

import pilot_shape_cases as ps
import tuned_ref as tr
from test_bcast_shapes_gpu import _split
from test_bcast_tuned_gpu import TOL, _bits, _check_case, _same
from test_scan_shapes_gpu import _exact_on_d, _records_equal

pytestmark = pytest.mark.gpu

SHAPE_IDS = [ps.bcast_id(s) for s in ps.BCAST_SHAPES]
FORMS = [(7, 3, 3, 5, 4, 9, 2), (64, 10, 101, 32, 5, 255, 25), ps.BCAST_D64]    # a small shape, the default on the fast kernels, the LDS-limited one


def _forms(shape):
    """generic: True always, False as well where the fast kernels are claimed"""
    return (False, True) if shape[:3] == (64, 10, 101) else (True,)


def _bcast(pkg, case, pilot_min, generic, nbytes=None, taps=None):
    T, D, P, Ta, Da, Tr, Dr = case["shape"]
    h, ga, gr, b, dg, rg = case["taps"] if taps is None else taps
    return pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b, pilot_min=float(pilot_min), diff_gain=dg,
                                                  rds_gain=rg, fir_decim=D, audio_decim=Da, rds_decim=Dr, n_streams=case["ns"],
                                                  max_bytes_per_call=case["iq"].shape[1] if nbytes is None else nbytes, force_generic=generic))


def _scan(pkg, case, pilot_min, generic):
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=case["taps"][3], ctaps=case["ctaps"], rot=case["rot"], pilot_min=float(pilot_min),
                                        fir_decim=case["shape"][1], max_bytes_per_call=case["iq"].shape[1], force_generic=generic))


def _mid(case):
    return ps.mid_gate(case["names"], [r["rds"]["pw"] for r in case["refs"]])


def _outputs_equal(got, want, where):
    for g, w, what in zip(got[:3], want[:3], ("L", "R", "bb")):
        assert _same(g, w), (where, what)
    assert np.array_equal(np.asarray(got[3]).astype(np.int64), np.asarray(want[3]).astype(np.int64)), (where, got[3], want[3])


# ---- 1. offset 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_zero_offset_is_the_untuned_handle_bitwise(pkg, shape):
    """taps (h, 0) and rot 0 on the case's rows: L, R, bb and pilot_count of the untuned handle, whatever steps the two forms walk in; the
    threshold lies in the middle of the rows' pilot powers at offset 0"""
    case = ps.bcast_case(pkg, shape)
    ns, iq = case["ns"], case["iq"]
    pilot_min = ps.offset_zero_gate(case, case["taps"][3])
    if shape == ps.BCAST_D64:
        assert (case["steps"][True]["NDT"], case["steps"][False]["NDT"]) == (201, 205)
    for generic in _forms(shape):
        with _bcast(pkg, case, pilot_min, generic) as bc:
            assert bc.kernel_name == ps.bcast_name(shape, False, generic), bc.kernel_name
            untuned = bc.process_batch(iq)
            bc.tune(ctaps=np.tile(tr.pairs(case["h"]), (ns, 1)), rot=np.zeros(ns, np.float32))
            assert bc.kernel_name == ps.bcast_name(shape, True, generic), bc.kernel_name
            tuned = bc.process_batch(iq)
            name = bc.kernel_name
        _outputs_equal(tuned, untuned, name)
        M = iq.shape[1] // 2 // shape[1]
        assert any(0 < int(c) < M for c in untuned[3]), ("the gate is not both on and off in any stream", list(untuned[3]), M)
        print("%s at offset 0: pilot_min %.4g, pilot counts %s of %d; L, R, bb bitwise the untuned handle's over %d + %d outputs a stream" % (
            name, pilot_min, [int(v) for v in tuned[3]], M, tuned[0].shape[1], tuned[2].shape[1]))


# ---- 2. the offsets that differ, against the reference; the tuned fast kernel against the tuned generic one -------------------------
@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_offsets_that_differ_against_the_reference(pkg, shape):
    case = ps.bcast_case(pkg, shape)
    outs = []
    for generic in _forms(shape):
        with _bcast(pkg, case, case["pilot_min"], generic) as bc:
            bc.tune(ctaps=case["ctaps"], rot=case["rot"])
            name = bc.kernel_name
            assert name == ps.bcast_name(shape, True, generic), name
            outs.append(bc.process_batch(case["iq"]))
        worst, frac = _check_case(case, case["refs"], outs[-1], name)
        assert worst <= TOL
        print("%s: %s at %s cycles / sample, pilot_min %.4g, pilot counts %s: worst |error| %.3g, %.3f %% of the outputs excluded" % (
            name, "/".join(case["names"]), case["cycles"], case["pilot_min"], [int(v) for v in outs[-1][3]], worst, 100 * frac))
    if len(outs) == 2:
        _outputs_equal(outs[0], outs[1], "tuned fast against tuned generic")


# ---- 3. metered, plain and alternating calls through the ragged sequence ------------------------------------------------------------
def _sequence(bc, iq, cuts, metered):
    """the calls one after the other, counts() before each; metered(k) says which are metered calls.  Returns (L, R, bb, summed pilot
    counts, the metered calls' records by call index)"""
    parts, pct, pos, recs = ([], [], []), 0, 0, {}
    for k, c in enumerate(cuts):
        want = bc.counts(c)
        out = bc.process_batch_metered(iq[:, pos:pos + c]) if metered(k) else bc.process_batch(iq[:, pos:pos + c])
        assert (out[0].shape[1], out[1].shape[1], out[2].shape[1]) == (want[0], want[0], want[1]), (c, out[0].shape, out[2].shape, want)
        if metered(k):
            m = out[4]
            assert (m["reserved"] == 0).all() and (m["n"] == m["n"][0]).all() and np.array_equal(m["n_pilot"], out[3].astype(np.uint64)), (c, m, out[3])
            if c == 0:
                assert not m.tobytes().strip(b"\0")
            recs[k] = m
        for acc, v in zip(parts, out[:3]):
            acc.append(v)
        pct = pct + out[3].astype(np.int64)
        pos += c
    assert pos == iq.shape[1]
    return tuple(np.concatenate(p, 1) for p in parts) + (pct, recs)


@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_metered_records_and_ragged_calls(pkg, shape):
    """At the case's tuning, the threshold in the middle of the rows' pilot powers.  One metered call: the records are a ScanDemod's with the
    same ctaps, rot, pilot taps and pilot_min in all seven fields, n = M, n_pilot = pilot_count, and L, R, bb and pilot_count are a second
    handle's plain call.  The case's cuts — 0 and 2 bytes, calls below one audio and below one RDS output, a call whose M is below H, one
    that leaves the input phase off 0, the long call of three workgroups a stream and two full steps a workgroup — as plain calls, as
    metered calls and in turn: the one call's bits each time, and the metered calls' records add up to the one call's."""
    import torch
    case = ps.bcast_case(pkg, shape)
    T, D, P, Ta, Da, Tr, Dr = shape
    ns, iq, cuts, pm = case["ns"], case["iq"], case["cuts"], _mid(case)
    M, M_long = iq.shape[1] // 2 // D, case["long"] // 2 // D
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for st in case["steps"].values():
        for per_cu in ps.PER_CU:
            bps, span = _split(M_long, st["NDT"], st["H"], ns, per_cu * cus)
            assert bps >= 3 and span >= 2 * st["NDT"], (per_cu, cus, bps, span, st)
    for generic in _forms(shape):
        with _bcast(pkg, case, pm, generic) as bc, _bcast(pkg, case, pm, generic) as other, _scan(pkg, case, pm, generic) as scn:
            bc.tune(ctaps=case["ctaps"], rot=case["rot"])
            other.tune(ctaps=case["ctaps"], rot=case["rot"])
            name = bc.kernel_name
            assert name == ps.bcast_name(shape, True, generic), name
            one = bc.process_batch_metered(iq)
            assert bc.kernel_name == name
            _records_equal(one[4], scn.process_batch(iq), name + " against the scan handle")
            assert (one[4]["n"] == M).all() and np.array_equal(one[4]["n_pilot"], one[3].astype(np.uint64)), (name, one[4], one[3])
            _outputs_equal(one, other.process_batch(iq), name + " against a plain call")
            seqs = {}
            for what, metered in (("plain", lambda k: False), ("metered", lambda k: True), ("in turn", lambda k: k % 2 == 0)):
                bc.reset()
                seqs[what] = _sequence(bc, iq, cuts, metered)
                _outputs_equal(seqs[what], one, "%s, %s calls" % (name, what))
            acc = np.zeros(ns, pkg.METER_DTYPE)
            for m in seqs["metered"][4].values():
                pkg.meter_add(acc, m)
            _records_equal(acc, one[4], name + ", the cuts summed")
            for k, m in seqs["in turn"][4].items():
                _records_equal(m, seqs["metered"][4][k], "%s, call %d of the calls in turn" % (name, k))
        assert any(0 < int(c) < M for c in one[3]), ("the gate is not both on and off in any stream", list(one[3]), M)
        print("%s metered: pilot_min %.4g, n %d, n_pilot %s, the seven fields the scan handle's; %d calls (the long one %d d's) plain, metered "
              "and in turn bitwise the one call" % (name, pm, M, [int(v) for v in one[4]["n_pilot"]], len(cuts), M_long))


# ---- 4. the metered call on unaligned device rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORMS, ids=[ps.bcast_id(s) for s in FORMS])
def test_metered_device_call_forms_give_the_host_calls(pkg, shape):
    """device rows cut from a larger allocation at byte offsets 2 / 6 / 14 with strides that are no multiple of 16, output rows with odd
    strides between canaries, the records 8 bytes into their allocation between canary records; on the caller's stream at the last"""
    import torch
    case = ps.bcast_case(pkg, shape)
    ns, iq, pm = case["ns"], case["iq"], _mid(case)
    nbytes = iq.shape[1]
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    generic = shape[:3] != (64, 10, 101)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert ns > 1
    with _bcast(pkg, case, pm, generic) as bc:
        bc.tune(ctaps=case["ctaps"], rot=case["rot"])
        want = bc.process_batch_metered(iq)
        na, nr = want[0].shape[1], want[2].shape[1]
        stream = torch.cuda.Stream()
        for k, (off, pad) in enumerate(((2, 2), (6, 6), (14, 10))):
            stride = nbytes + pad + (4 if (nbytes + pad) % 16 == 0 else 0)
            assert stride % 16 != 0
            buf = torch.full((ns * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            for s in range(ns):
                buf[off + s * stride:off + s * stride + nbytes] = torch.from_numpy(iq[s].copy()).cuda()
            d_l = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
            d_r = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
            d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
            d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
            words = torch.full((8 * (ns + 2) + 1,), -7, dtype=torch.int64, device="cuda")
            assert buf.data_ptr() % 16 == 0 and words.data_ptr() % 64 == 0
            torch.cuda.synchronize()
            bc.reset()
            if k == 2:
                bc.set_stream(stream.cuda_stream)
            n1, n2 = C.c_uint32(), C.c_uint32()
            rc = lib.sdrfm_bcast_process_batch_metered(bc._h, None, ptr(buf, off), stride, nbytes, ptr(d_l), ptr(d_r), d_l.stride(0), None, 0, ptr(d_w),
                                                       d_w.stride(0), ptr(d_pc), ptr(words, 64 + 8), C.byref(n1), C.byref(n2), DEV)
            assert rc == pkg.lib.OK and (n1.value, n2.value) == (na, nr), (rc, n1.value, n2.value, na, nr)
            bc.synchronize()
            stream.synchronize()
            where = "device rows at byte %d, stride %d" % (off, stride)
            host = words.cpu().numpy()
            assert (host[:9] == -7).all() and (host[9 + 8 * ns:] == -7).all(), (where, host[:9], host[9 + 8 * ns:])
            _records_equal(np.ascontiguousarray(host[9:9 + 8 * ns]).view(pkg.METER_DTYPE).reshape(ns), want[4], where)
            got = (d_l[:, :na].cpu().numpy(), d_r[:, :na].cpu().numpy(), np.ascontiguousarray(d_w[:, :2 * nr].cpu().numpy()).view(np.complex64),
                   d_pc.cpu().numpy())
            _outputs_equal(got, want, where)
            assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all(), where
        bc.reset()
        bc.set_stream(None)


# ---- 5. the metered record at the top of its range -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "tuned"])
def test_metered_record_at_the_top_of_its_range_is_exact(pkg, tuned):
    """tests/pilot_shape_cases.py's magnitude case on the metered generic broadcast kernels at Ta = Tr = 1, Da = Dr = 1, untuned with h = 16
    and tuned to taps (16, 0) and rot 0: a first call fills the pilot filter's history, then 4 MiB a stream.  Every field is exact
    against the device's own d (rf_q against tests/scan_ref.py), n_pilot is pilot_count, and with the gate at 1e-18 every d passes, at 1e3
    none; L, R, bb and pilot_count are a second handle's plain call."""
    m = ps.magnitude_case(pkg)
    iq, first, one = m["iq"], ps.MAG_WARM // 2, np.ones(1, np.float32)
    case = dict(shape=ps.MAG_BCAST_SHAPE, ns=2, iq=iq, taps=(m["h"], one, one, m["b"], 1.0, 1.0))
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=m["h"], audio_coeffs=one, fir_decim=1, audio_decim=1, n_streams=2, bit_exact=True,
                                  max_bytes_per_call=ps.MAG_BYTES)) as mono:
        d = np.concatenate([mono.process_batch(iq[:, :ps.MAG_WARM]), mono.process_batch(iq[:, ps.MAG_WARM:])], 1)
    for gate in ps.MAG_GATES:
        with _bcast(pkg, case, gate, True, nbytes=ps.MAG_BYTES) as bc, _bcast(pkg, case, gate, True, nbytes=ps.MAG_BYTES) as other:
            for h_ in (bc, other):
                if tuned:
                    h_.tune(ctaps=m["ctaps"], rot=m["rot"])
                assert h_.kernel_name == ps.bcast_name(ps.MAG_BCAST_SHAPE, tuned, True), h_.kernel_name
            warm = bc.process_batch_metered(iq[:, :ps.MAG_WARM])
            got = bc.process_batch_metered(iq[:, ps.MAG_WARM:])
            other.process_batch(iq[:, :ps.MAG_WARM])
            plain = other.process_batch(iq[:, ps.MAG_WARM:])
            name = bc.kernel_name
        assert (warm[4]["n"] == first).all()
        _outputs_equal(got, plain, "%s, gate %g" % (name, gate))
        assert got[0].shape == (2, 1 << 21) and got[2].shape == (2, 1 << 21)
        if gate == ps.MAG_GATES[1]:                                  # the gate shut, one unit audio tap at Da = 1: L is d, (P - 1) / 2 d's late
            dl = (ps.MAG_SHAPE[2] - 1) // 2
            assert np.array_equal(_bits(got[0]), _bits(d[:, first - dl:d.shape[1] - dl]))
        for s in range(2):
            want = _exact_on_d(d[s], m["b"], gate, first)
            want["rf_q"] = m["refs"][s]["rec"]["rf_q"]
            have = {f: int(got[4][f][s]) for f in got[4].dtype.names}
            print("%s metered, gate %g, stream %d: n %d, n_pilot %d, rf_q 2^%.2f, freq_q %d, pilot_q 2^%.2f, pilot2_q 2^%.2f" % (
                name, gate, s, have["n"], have["n_pilot"], np.log2(have["rf_q"]), have["freq_q"], np.log2(max(have["pilot_q"], 1)),
                np.log2(max(have["pilot2_q"], 1))))
            for k, v in want.items():
                assert have[k] == v, (name, gate, s, k, have[k], v)
            assert have["n"] == 1 << 21 and have["n_pilot"] == int(got[3][s]) == (have["n"] if gate == ps.MAG_GATES[0] else 0) and have["reserved"] == 0
        assert int(got[4]["pilot_q"][0]) >= 2 ** 54 and int(got[4]["pilot2_q"][0]) >= 2 ** 59 and int(got[4]["freq_q"][1]) <= -2 ** 46
