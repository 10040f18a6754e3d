"""GPU sweep of the broadcast handle's hist kernels (sdrfm_bcast_process_batch_metered_hist) over every shape of
tests/pilot_shape_cases.py, tuned and untuned, on the generic kernels and on the fast ones where the handle claims them.  At the LDS-limited
shapes the hist step is shorter than the plain one — 197 against 205 d's at T256 D64 P255 Ta256 Tr256 — and every comparison here runs the
one against the other: the rows are a ScanDemod's hist rows, integer for integer; L, R, bb, pilot_count and all eight words of the records
are a second handle's metered call; through the case's ragged sequence, hist calls with plain calls in between, every hist call gives the
scan handle's rows of that call and the outputs are the one call's bits.  Then the top of a bin's range at 4 MiB, and the device form on
unaligned rows with the histogram 4 bytes into its allocation."""
import ctypes as C

import numpy as np
import pytest

import bcast_hist_cases as bh
import pilot_shape_cases as ps
import tuned_ref as tr
from test_bcast_tuned_shapes_gpu import FORMS, SHAPE_IDS, _bcast, _forms, _outputs_equal

pytestmark = pytest.mark.gpu

BINS = bh.BINS


def _words(m):
    return np.ascontiguousarray(m).view(np.uint64)


def _scan(pkg, case, ctaps, rot, pilot_min, generic):
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=case["taps"][3], ctaps=ctaps, rot=rot, pilot_min=float(pilot_min), fir_decim=case["shape"][1],
                                        max_bytes_per_call=case["iq"].shape[1], force_generic=generic))


# ---- 1. every shape, tuned and untuned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "tuned"])
@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_rows_records_and_ragged_calls(pkg, shape, tuned):
    case = ps.bcast_case(pkg, shape)
    ns, iq, cuts, pm = case["ns"], case["iq"], case["cuts"], case["pilot_min"]
    M, long_at = iq.shape[1] // 2 // shape[1], case["cuts"].index(case["long"])
    ctaps, rot = (case["ctaps"], case["rot"]) if tuned else (np.tile(tr.pairs(case["h"]), (ns, 1)), np.zeros(ns, np.float32))
    if shape in bh.STEPS:
        assert (case["steps"][tuned]["NDT"], bh.hist_step(shape, tuned)["NDT"]) == bh.STEPS[shape][tuned]
    for generic in _forms(shape):
        with _bcast(pkg, case, pm, generic) as bc, _bcast(pkg, case, pm, generic) as other, _scan(pkg, case, ctaps, rot, pm, generic) as scn:
            if tuned:
                bc.tune(ctaps=ctaps, rot=rot)
                other.tune(ctaps=ctaps, rot=rot)
            name = bc.hist_kernel_name()
            assert bc.kernel_name == ps.bcast_name(shape, tuned, generic) and name == bh.hist_name(shape, tuned, generic), (bc.kernel_name, name)
            one = bc.process_batch_metered_hist(iq)
            met = other.process_batch_metered(iq)
            _outputs_equal(one, met, name + " against a metered call")
            assert np.array_equal(_words(one[4]), _words(met[4])), (name, one[4], met[4])
            bh.check_rows(one[4], one[5], name)
            assert (one[4]["n"] == M).all()
            want = scn.process_batch_hist(iq)[1]
            assert np.array_equal(one[5], want), (name, np.argwhere(one[5] != want)[:8])
            # the ragged sequence: hist calls with plain calls in between, the long call a hist call; the scan handle makes the same calls
            bc.reset()
            scn.reset()
            parts, pct, pos, acc = ([], [], []), 0, 0, np.zeros((ns, BINS), np.uint64)
            for k, c in enumerate(cuts):
                part = iq[:, pos:pos + c]
                rows = scn.process_batch_hist(part)[1]
                if k % 2 == long_at % 2:
                    out = bc.process_batch_metered_hist(part)
                    bh.check_rows(out[4], out[5], (name, k))
                    assert np.array_equal(out[5], rows), (name, k, c)
                    if c == 0:
                        assert not out[5].any()
                else:
                    out = bc.process_batch(part)
                pkg.hist_add(acc, rows)
                for a, v in zip(parts, out[:3]):
                    a.append(v)
                pct = pct + out[3].astype(np.int64)
                pos += c
            assert pos == iq.shape[1]
            _outputs_equal(tuple(np.concatenate(p, 1) for p in parts) + (pct,), one, name + ", hist and plain calls in turn")
            assert np.array_equal(acc, one[5].astype(np.uint64)), name
        print("%s: %d streams, n %d, %d bins in use; rows the scan handle's, the rest a metered call's; %d calls (the long one %d d's) in turn" % (
            name, ns, M, int(np.count_nonzero(one[5].sum(0))), len(cuts), case["long"] // 2 // shape[1]))


# ---- 2. the top of the range ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "tuned"])
def test_top_of_the_range(pkg, tuned):
    """T = D = 1, one stream of 4 MiB, n = 2^21.  Constant bytes put every count into bin 256: the largest count a bin can hold, all of it
    added to one LDS word of every workgroup.  The byte pairs (255, 254), (1, 2) in turn give d = +-(pi - 3.1e-5): the two extreme bins;
    d[0] is 0 (no sample before it)"""
    const, extreme = bh.top_rows()
    h, one, n = np.array([1.0], np.float32), np.ones(1, np.float32), 1 << 21
    case = dict(shape=bh.TOP_SHAPE, ns=1, iq=const, taps=(h, one, one, np.array([2, -2, 2, -1, 1], np.complex64), 1.0, 1.0))
    want = {256: n}, {457: 1048576, 54: 1048575, 256: 1}
    with _bcast(pkg, case, 0.05, True, nbytes=bh.TOP_BYTES) as bc:
        if tuned:
            bc.tune(ctaps=tr.pairs(h)[None, :], rot=np.zeros(1, np.float32))
        assert bc.hist_kernel_name() == "bcast-generic%s T1 D1 P5 Ta1 Da1 Tr1 Dr1 + hist" % ("-tuned" if tuned else ""), bc.hist_kernel_name()
        for iq, bins in zip((const, extreme), want):
            bc.reset()
            out = bc.process_batch_metered_hist(iq)
            bh.check_rows(out[4], out[5], bins)
            got = {int(b): int(out[5][0, b]) for b in np.flatnonzero(out[5][0])}
            print("%s: %s" % (bc.hist_kernel_name(), got))
            assert got == bins and int(out[4]["n"][0]) == n, (got, bins)


# ---- 3. the device form on unaligned rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORMS, ids=[ps.bcast_id(s) for s in FORMS])
def test_device_call_on_unaligned_rows(pkg, shape):
    """device rows cut from a larger allocation at byte offset 6 with a stride that is no multiple of 16, the records 8 bytes and the
    histogram 4 bytes into their allocations, rows of 515 words between canaries"""
    import torch
    case = ps.bcast_case(pkg, shape)
    ns, iq, pm = case["ns"], case["iq"], case["pilot_min"]
    nbytes, generic, stride_h = iq.shape[1], shape[:3] != (64, 10, 101), 515
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    with _bcast(pkg, case, pm, generic) as bc:
        bc.tune(ctaps=case["ctaps"], rot=case["rot"])
        want = bc.process_batch_metered_hist(iq)
        na, nr = want[0].shape[1], want[2].shape[1]
        off, stride = 6, nbytes + 6 + (4 if (nbytes + 6) % 16 == 0 else 0)
        assert stride % 16 != 0
        buf = torch.full((ns * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        for s in range(ns):
            buf[off + s * stride:off + s * stride + nbytes] = torch.from_numpy(iq[s].copy()).cuda()
        d_l = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
        words = torch.full((8 * (ns + 2) + 1,), -7, dtype=torch.int64, device="cuda")
        d_h = torch.full((1 + (ns + 2) * stride_h,), -7, dtype=torch.int32, device="cuda")
        assert d_h.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        bc.reset()
        n1, n2 = C.c_uint32(), C.c_uint32()
        rc = lib.sdrfm_bcast_process_batch_metered_hist(bc._h, None, ptr(buf, off), stride, nbytes, ptr(d_l), ptr(d_r), d_l.stride(0), None, 0, ptr(d_w),
                                                        d_w.stride(0), ptr(d_pc), ptr(words, 64 + 8), ptr(d_h, 4 + 4 * stride_h), stride_h,
                                                        C.byref(n1), C.byref(n2), DEV)
        assert rc == pkg.lib.OK and (n1.value, n2.value) == (na, nr), (rc, n1.value, n2.value, na, nr)
        bc.synchronize()
        host, gh = words.cpu().numpy(), d_h.cpu().numpy()
        assert (host[:9] == -7).all() and (host[9 + 8 * ns:] == -7).all()
        assert np.array_equal(host[9:9 + 8 * ns].view(np.uint64), _words(want[4]))
        rows = gh[1:].reshape(ns + 2, stride_h)
        assert gh[0] == -7 and (rows[0] == -7).all() and (rows[ns + 1] == -7).all() and (rows[:, BINS:] == -7).all()
        assert np.array_equal(np.ascontiguousarray(rows[1:ns + 1, :BINS]).view(np.uint32), want[5])
        got = (d_l[:, :na].cpu().numpy(), d_r[:, :na].cpu().numpy(), np.ascontiguousarray(d_w[:, :2 * nr].cpu().numpy()).view(np.complex64),
               d_pc.cpu().numpy())
        _outputs_equal(got, want, "device rows at byte %d, stride %d" % (off, stride))
        assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all()
