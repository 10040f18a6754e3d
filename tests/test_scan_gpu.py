"""GPU tests of the scan handle (sdrfm_scan_*).  Exact on the device alone, whole records as integers: the fast kernel
against the generic one, one call against a ragged sequence of calls summed with sdrfm_scan_meter_add, the same row under different
workgroup splits, one shared row against replicated rows on host and on device buffers, reset and tune, the offset-fs/2 identity.  Exact
against the device's own d at offset 0 (the bit-exact mono handle hands d back).  Against tests/scan_ref.py from bytes at the tuned
offsets of tests/scan_cases.py.  End to end: two scan scenarios through scan_capture, and a second scan tuned to what it returned."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as sc
import scan_ref as sr
from rds_ref import rds_ref
from tuned_ref import pairs

pytestmark = pytest.mark.gpu

TOL_D = 1e-5                                                    # the project's tolerance on d (radians): the device's arctangent
LDS_BUDGET = 64 << 10                                           # the host geometry of csrc/sdrfm_scan.hip
KERNELS = [(name, generic) for name in sc.SHAPES for generic in ((False, True) if name == "default" else (True,))]
KERNEL_IDS = ["%s-%s" % (n, "generic" if g else "fast") for n, g in KERNELS]
EVEN_D = [k for k in KERNELS if sc.SHAPES[k[0]][1] % 2 == 0]


def _handle(pkg, shape, ctaps, rot, pilot_min=0.05, nbytes=sc.NBYTES, generic=False, shared=False, b=None):
    T, D, P = shape
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=sc.shape_taps(pkg, shape)[1] if b is None else b, ctaps=ctaps, rot=rot, pilot_min=float(pilot_min),
                                        fir_decim=D, shared_input=shared, max_bytes_per_call=nbytes, force_generic=generic))


def _want_name(shape, generic):
    return "scan-generic T%d D%d P%d" % shape if generic or shape != (64, 10, 101) else "scan-fast T64 D10 P101"


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ndt(T, D, P):
    """new d's per step of the generic kernel (the fast one's is the same 1023 where it runs): the largest the LDS budget allows"""
    H = P - 1

    def lds(ny):
        rw = (max((ny - 1) * D + T + 4, H + ny - 1 + 4) + 3) & ~3
        return 4 * rw + 8 * ny + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 8 * T

    ny = 1024
    while ny > 2 and lds(ny) > LDS_BUDGET:
        ny -= 2
    return ny - 1


def _split(M, ndt, H, ns, slots):
    """workgroups per stream of a call, as the handle chooses them (front_split)"""
    bps, best = 1, None
    for k in range(1, min((M + ndt - 1) // ndt, 64) + 1):
        cost = ((ns * k + slots - 1) // slots) * ((M + k - 1) // k + H // 2 + 64)
        if best is None or cost < best:
            best, bps = cost, k
    return bps


def _rows(pkg, ns, nsamp, fs, first_id):
    """ns rows of bytes: the FM generator, random bytes and constant bytes in turn"""
    return np.stack([pkg.make_iq(1, nsamp, mode=("fm", "random", "const")[s % 3], fs=fs, first_id=first_id + s)[0] for s in range(ns)])


def _in_calls(pkg, scn, iq, cuts):
    """the calls one after the other, their records summed with sdrfm_scan_meter_add"""
    acc, pos = np.zeros(scn.n_streams, pkg.METER_DTYPE), 0
    for c in cuts:
        m = scn.process_batch(iq[:, pos:pos + c])
        assert m.shape == acc.shape and (m["reserved"] == 0).all()
        pkg.meter_add(acc, m)
        pos += c
    assert pos == iq.shape[1]
    return acc


# ---- 1. the two kernel forms ---------------------------------------------------------------------------------------------------------
def test_fast_is_generic_record_for_record(pkg):
    su = sc.case_setup(pkg, sc.CASES[2])                            # default shape, 7 streams, the five offsets
    got = []
    for generic in (False, True):
        with _handle(pkg, su["shape"], su["ctaps"], su["rot"], generic=generic) as scn:
            assert scn.kernel_name == _want_name(su["shape"], generic)
            got.append(scn.process_batch(su["iq"]))
    assert _same(got[0], got[1]), (got[0], got[1])
    assert (got[0]["n"] == sc.NBYTES // 2 // 10).all() and (got[0]["reserved"] == 0).all()
    assert 0 < int(got[0]["n_pilot"][0]) and int(got[0]["rf_q"][0]) > 0


# ---- 2. one call against a ragged sequence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_ragged_calls_add_up_to_the_one_call(pkg, name, generic):
    """0 and 2 bytes, a call whose M is below H, a second 0, one call of more than 64 steps (the split gives a stream 64 workgroups at the
    most, so each walks two steps at the least), then random ones; the records summed with sdrfm_scan_meter_add are the one call's"""
    import torch
    shape = sc.SHAPES[name]
    T, D, P = shape
    H, ndt, fs = P - 1, _ndt(T, D, P), sc.tc.fs_of(D)
    idx = KERNELS.index((name, generic))
    ns = (3, 7, 1)[idx % 3]
    cuts = [0, 2] + ([2 * D * (H // 2) - 2] if H >= 4 else []) + [0]
    long_ = 2 * D * (64 * ndt + ndt // 2) + 6
    cuts.append(long_)
    rng = np.random.default_rng(300 + idx)
    cuts += [int(v) for v in 2 * rng.integers(1, D * ndt, 5)]
    nbytes = sum(cuts)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (1, 2, 3):
        bps = _split(long_ // 2 // D, ndt, H, ns, per_cu * cus)
        assert bps >= 3 and (long_ // 2 // D + bps - 1) // bps > ndt, (bps, ndt)
    iq = _rows(pkg, ns, nbytes // 2, fs, 8000 + 10 * idx)
    h = sc.shape_taps(pkg, shape)[0]
    cyc = [sc.OFFSETS[(s + idx) % len(sc.OFFSETS)] for s in range(ns)]
    ctaps = np.stack([pkg.tuned_channel_taps(h, c * fs, fs) for c in cyc])
    rot = np.array([pkg.tuned_rotation(c * fs, fs, D) for c in cyc], np.float32)
    with _handle(pkg, shape, ctaps, rot, nbytes=nbytes, generic=generic) as scn:
        assert scn.kernel_name == _want_name(shape, generic)
        one = scn.process_batch(iq)
        scn.reset()
        seq = _in_calls(pkg, scn, iq, cuts)
        zero = scn.process_batch(iq[:, :0])
    assert _same(one, seq), (one, seq)
    assert (one["n"] == nbytes // 2 // D).all() and not zero.tobytes().strip(b"\0")


# ---- 3. the same row under different splits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_stream_count_and_split_do_not_change_a_record(pkg, generic):
    """1, 3, 7 and 256 streams with stream 0's tuning on one shared row: 256 streams x 7 workgroups are more than the device runs at a
    time, so the handle gives a stream fewer workgroups than it gives one stream alone"""
    import torch
    su = sc.case_setup(pkg, sc.CASES[0])
    shape = su["shape"]
    M, cus = sc.NBYTES // 2 // shape[1], torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (1, 2, 3):
        assert _split(M, 1023, shape[2] - 1, 1, per_cu * cus) != _split(M, 1023, shape[2] - 1, 256, per_cu * cus)
    recs = []
    for ns in (1, 3, 7, 256):
        with _handle(pkg, shape, np.tile(su["ctaps"][0], (ns, 1)), np.tile(su["rot"][0], ns), generic=generic, shared=True) as scn:
            recs.append(scn.process_batch(su["iq"][0:1]))
    for r in recs:
        assert r.tobytes() == recs[0].tobytes() * r.size, r


# ---- 4. one shared row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_shared_input_is_replicated_rows(pkg, generic):
    import torch
    shape, ns, nbytes = sc.SHAPES["default"], 3, sc.NBYTES
    row = sc.tc.three_stations(pkg)[0][:, :nbytes]
    h = sc.shape_taps(pkg, shape)[0]
    offs = [st["offset_hz"] for st in sc.tc.STATIONS]
    ctaps = np.stack([pkg.tuned_channel_taps(h, f, 2.4e6) for f in offs])
    rot = np.array([pkg.tuned_rotation(f, 2.4e6, 10) for f in offs], np.float32)
    cuts = [2 * 20001, 0, 2 * 7, nbytes - 2 * 20008]
    lib = pkg.load_library()
    with _handle(pkg, shape, ctaps, rot, generic=generic) as rep, _handle(pkg, shape, ctaps, rot, generic=generic, shared=True) as sh:
        want = _in_calls(pkg, rep, np.repeat(row, ns, 0), cuts)
        got = _in_calls(pkg, sh, row, cuts)
        assert _same(want, got), ("host buffers", want, got)
        assert len({m.tobytes() for m in got}) == ns                # (the streams do see different stations)
        # device buffers: one row between canaries and an iq_stride that would run off it if it were used; the records between canary records
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[32:32 + nbytes] = torch.from_numpy(row[0].copy()).cuda()
        rows3 = torch.from_numpy(np.repeat(row, ns, 0).copy()).cuda()
        torch.cuda.synchronize()
        for scn, shared in ((sh, True), (rep, False)):
            d_m = torch.full((ns + 2, 8), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            scn.reset()
            acc, pos = np.zeros(ns, pkg.METER_DTYPE), 0
            for c in cuts:
                src, stride = (buf.data_ptr() + 32 + pos, 1 << 40) if shared else (rows3.data_ptr() + pos, rows3.stride(0))
                rc = lib.sdrfm_scan_process_batch(scn._h, C.c_void_p(src), stride, c, C.c_void_p(d_m.data_ptr() + 64), pkg.lib.F_DEVICE_PTRS)
                assert rc == pkg.lib.OK, rc
                scn.synchronize()
                host = d_m.cpu().numpy()
                assert (host[0] == -7).all() and (host[ns + 1] == -7).all(), host
                pkg.meter_add(acc, np.ascontiguousarray(host[1:ns + 1]).view(pkg.METER_DTYPE).reshape(ns))
                pos += c
            assert _same(acc, want), ("device buffers", shared, acc, want)
        assert (buf[:32] == 0xA5).all() and (buf[32 + nbytes:] == 0xA5).all()
    # process_batch_device: the Python form of the same call
    with _handle(pkg, shape, ctaps, rot, generic=generic, shared=True) as scn:
        d_m = torch.zeros((ns, 8), dtype=torch.int64, device="cuda")
        scn.process_batch_device(buf[32:32 + nbytes], d_m)
        scn.synchronize()
        with _handle(pkg, shape, ctaps, rot, generic=generic, shared=True) as one:
            assert _same(d_m.cpu().numpy().view(pkg.METER_DTYPE).reshape(ns), one.process_batch(row))


# ---- 5. reset and tune ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_reset_and_tune_restart_the_streams(pkg, generic):
    su = sc.case_setup(pkg, sc.CASES[1])
    iq, half = su["iq"], 2 * 30001
    other = np.roll(su["ctaps"], 1, axis=0), np.roll(su["rot"], 1)
    lib = pkg.load_library()
    with _handle(pkg, su["shape"], su["ctaps"], su["rot"], generic=generic) as scn:
        first = scn.process_batch(iq[:, :half])
        second = scn.process_batch(iq[:, half:])
        scn.reset()                                                  # keeps the tuning
        again = scn.process_batch(iq[:, :half])
        scn.process_batch(iq[:, half:half + 2 * 777])                # (state to be dropped)
        scn.tune(ctaps=other[0], rot=other[1])
        moved = scn.process_batch(iq[:, :half])
        scn.process_batch(iq[:, half:half + 2 * 333])
        scn.tune(ctaps=su["ctaps"], rot=su["rot"])                   # a re-tune is a restart
        third = scn.process_batch(iq[:, :half])
        # a refused tune or call changes nothing: the second half continues the stream
        bad = su["rot"].copy()
        bad[0] = np.nan
        assert lib.sdrfm_scan_tune(scn._h, su["ctaps"].ctypes.data, bad.ctypes.data) == pkg.lib.EINVAL
        assert lib.sdrfm_scan_tune(scn._h, None, su["rot"].ctypes.data) == pkg.lib.EINVAL
        assert lib.sdrfm_scan_tune(scn._h, su["ctaps"].ctypes.data, None) == pkg.lib.EINVAL
        m = np.zeros(su["ns"], pkg.METER_DTYPE)
        assert lib.sdrfm_scan_process_batch(scn._h, iq.ctypes.data, iq.shape[1], 101, m.ctypes.data, 0) == pkg.lib.EODD
        assert lib.sdrfm_scan_process_batch(scn._h, iq.ctypes.data, iq.shape[1], sc.NBYTES + 2, m.ctypes.data, 0) == pkg.lib.ECAPACITY
        assert lib.sdrfm_scan_process_batch(scn._h, iq.ctypes.data, 98, 100, m.ctypes.data, 0) == pkg.lib.ECAPACITY
        assert lib.sdrfm_scan_process_batch(scn._h, iq.ctypes.data, iq.shape[1], 100, m.ctypes.data, pkg.lib.F_OVERLAP) == pkg.lib.EINVAL
        assert lib.sdrfm_scan_process_batch(scn._h, iq.ctypes.data, iq.shape[1], 100, None, 0) == pkg.lib.EINVAL
        assert lib.sdrfm_scan_process_batch(scn._h, None, iq.shape[1], 100, m.ctypes.data, 0) == pkg.lib.EINVAL
        rest = scn.process_batch(iq[:, half:])
    assert _same(first, again) and _same(first, third) and not _same(first, moved)
    assert _same(second, rest)


# ---- 6. offset fs / 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", EVEN_D, ids=["%s-%s" % (n, "generic" if g else "fast") for n, g in EVEN_D])
def test_half_rate_is_the_offset_zero_record(pkg, name, generic):
    """taps (-1)^k h[k], rot 0, an even D, on bytes with every odd-indexed sample replaced by 255 - byte: the record of taps (h, 0) on
    the original bytes, all seven fields"""
    shape = sc.SHAPES[name]
    T, D, P = shape
    ns = 3
    iq = _rows(pkg, ns, sc.NBYTES // 2, sc.tc.fs_of(D), 8200)
    flipped = iq.copy().reshape(ns, -1, 2)
    flipped[:, 1::2] = 255 - flipped[:, 1::2]
    flipped = flipped.reshape(ns, -1)
    h = sc.shape_taps(pkg, shape)[0]
    sign = np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    zero = np.zeros(ns, np.float32)
    with _handle(pkg, shape, np.tile(pairs(h), (ns, 1)), zero, generic=generic) as scn:
        want = scn.process_batch(iq)
        scn.tune(ctaps=np.tile(pairs(h * sign), (ns, 1)), rot=zero)
        got = scn.process_batch(flipped)
    assert _same(want, got), (want, got)
    assert int(want["n_pilot"].max()) > 0 and int(want["rf_q"][0]) > 0


# ---- 7. exact against the device's own d at offset 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_offset_zero_record_is_exact_on_the_devices_own_d(pkg, name, generic):
    """taps (h, 0) and rot 0 give the untuned d bit for bit; the bit-exact mono handle with a one-tap unit audio filter hands that d back.
    freq_q and dev_q are numpy fp32 on it, pilot_q, pilot2_q and n_pilot come from tests/rds_ref.py's fp32-faithful pw on it, and n_pilot
    is the untuned broadcast handle's pilot_count as well"""
    shape = sc.SHAPES[name]
    T, D, P = shape
    ns, fs, pilot_min = 3, sc.tc.fs_of(D), 0.05
    iq = np.stack([pkg.make_iq_rds(1, sc.NBYTES // 2, sc.tc.GROUPS, fs=fs, first_id=8300)[0], pkg.make_iq(1, sc.NBYTES // 2, mode="fm", fs=fs, first_id=8301)[0],
                   pkg.make_iq(1, sc.NBYTES // 2, mode="random", fs=fs, first_id=8302)[0]])
    h, b = sc.shape_taps(pkg, shape)
    one = np.ones(1, np.float32)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True,
                                  max_bytes_per_call=sc.NBYTES)) as mono:
        d = mono.process_batch(iq)
    with pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=one, rds_coeffs=one, pilot_coeffs=b, pilot_min=pilot_min, fir_decim=D,
                                                audio_decim=1, rds_decim=1, n_streams=ns, max_bytes_per_call=sc.NBYTES, force_generic=generic)) as bc:
        pc = bc.process_batch(iq)[3]
    with _handle(pkg, shape, np.tile(pairs(h), (ns, 1)), np.zeros(ns, np.float32), pilot_min=pilot_min, generic=generic) as scn:
        got = scn.process_batch(iq)
    f32, q24, q20 = np.float32, np.float32(2.0 ** 24), np.float32(2.0 ** 20)
    fix = lambda term, scale: int(np.rint((term * scale).astype(f32)).astype(np.int64).sum())
    for s in range(ns):
        ds = d[s].astype(f32)
        ref = rds_ref(ds, b, one, pilot_min, 1.0, Dr=1)
        pw = ref["pw"].astype(f32)
        want = dict(n=ds.size, n_pilot=int(ref["on"].sum()), freq_q=fix(ds, q24), dev_q=fix((ds * ds).astype(f32), q24), pilot_q=fix(pw, q24),
                    pilot2_q=fix((pw * pw).astype(f32), q20))
        have = sr.rec_of(got[s])
        for k, v in want.items():
            assert have[k] == v, (name, s, k, have[k], v)
        assert have["n_pilot"] == int(pc[s]), (s, have["n_pilot"], int(pc[s]))
    assert 0 < int(got["n_pilot"][0]) < d.shape[1]


# ---- 8. against the reference from bytes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=[sc.case_id(c) for c in sc.CASES])
def test_tuned_offsets_against_the_reference(pkg, case):
    """n and rf_q are equal: K2 holds no transcendental and is the same fmaf order.  The rest differs by the device's arctangent: |d| by
    TOL_D at the most, so e = d^2 by 2 pi TOL_D (|d| <= pi), q = b * d by TOL_D sum|b|, pw = |q|^2 by 2 max|q| times that, and g = pw^2 by
    2 max pw times pw's bound; the means of the records' integers differ by that much and, for g, whose bound can be smaller than the
    fixed-point step, by one step of 2^-20 more (|rint(a) - rint(b)| <= |a - b| + 1)."""
    su, refs = sc.case_reference(pkg, case)
    b = np.asarray(su["b"], np.complex128)
    sum_b = float(np.abs(b).sum())
    for generic in ((False, True) if case[0] == "default" else (True,)):
        with _handle(pkg, su["shape"], su["ctaps"], su["rot"], su["pilot_min"], generic=generic) as scn:
            name = scn.kernel_name
            assert name == _want_name(su["shape"], generic), name
            got = scn.process_batch(su["iq"])
        for s, r in enumerate(refs):
            have, want, n = sr.rec_of(got[s]), r["rec"], r["d"].size
            amb = sr.ambiguous(r["pw"], r["pmin2"])
            lo = int(((r["pw"] >= r["pmin2"]) & ~amb).sum())
            qmax = float(np.sqrt(r["pw"].astype(np.float64).max()))
            tol_pw = 2.0 * qmax * sum_b * TOL_D
            tol_g = 2.0 * qmax * qmax * tol_pw + 2.0 ** -20
            err = {k: abs(have[k] - want[k]) / n / 2.0 ** sh for k, sh in (("freq_q", 24), ("dev_q", 24), ("pilot_q", 24), ("pilot2_q", 20))}
            print("%s stream %d (%s at %+.4f): rf_q %s, n_pilot %d in [%d, %d], mean errors d %.3g (%.3g) e %.3g (%.3g) pw %.3g (%.3g) g %.3g (%.3g)" % (
                name, s, su["names"][s], su["cycles"][s], "equal" if have["rf_q"] == want["rf_q"] else "%d != %d" % (have["rf_q"], want["rf_q"]),
                have["n_pilot"], lo, lo + int(amb.sum()), err["freq_q"], TOL_D, err["dev_q"], 2 * np.pi * TOL_D, err["pilot_q"], tol_pw,
                err["pilot2_q"], tol_g))
            assert amb.mean() <= sc.EXCLUDED_CAP
            assert have["n"] == want["n"] == n and have["reserved"] == 0
            assert have["rf_q"] == want["rf_q"], (name, s, have["rf_q"], want["rf_q"])
            assert lo <= have["n_pilot"] <= lo + int(amb.sum()), (name, s, have["n_pilot"], lo, int(amb.sum()))
            assert err["freq_q"] <= TOL_D and err["dev_q"] <= 2 * np.pi * TOL_D, (name, s, err)
            assert err["pilot_q"] <= tol_pw and err["pilot2_q"] <= tol_g, (name, s, err, tol_pw, tol_g)


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["three-on-the-grid", "crystal+7kHz-and-mono"])
def test_scan_capture_finds_the_stations_and_a_second_scan_is_on_tune(pkg, scenario):
    row, truth = sc.scenario_capture(pkg, scenario)
    h, b = sc.scenario_taps(pkg)
    offsets, _, ref = sc.scenario_reference(pkg, scenario)
    found, report, grid, _ = pkg.scan_capture(row, sc.FS, h, grid_hz=sc.GRID_HZ, details=True)
    assert np.array_equal(grid, offsets)
    prs = sc.check_found(found, truth)
    for f, t in prs:
        c = f["candidate"]
        print("%s: %+.1f Hz (true %+.1f), level %.1f dBFS, stereo %s, freq_err %.2f Hz (reference %.2f)" % (
            scenario, f["offset_hz"], t["offset_hz"], f["level_dbfs"], f["stereo"], report["freq_err_hz"][c], ref["freq_err_hz"][c]))
        assert abs(report["freq_err_hz"][c] - ref["freq_err_hz"][c]) <= 1.0, (c, report["freq_err_hz"][c], ref["freq_err_hz"][c])
    tuned = [f["offset_hz"] for f in found]
    with pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=b, offsets_hz=tuned, h=h, fs=sc.FS, shared_input=True, max_bytes_per_call=row.size)) as scn:
        assert scn.kernel_name.startswith("scan-fast")
        rep2 = pkg.meter_report(scn.process_batch(row), sc.FS, 10)
    assert np.abs(rep2["freq_err_hz"]).max() < 100.0, rep2["freq_err_hz"]
    # ... and the offsets go into the broadcast handle as they are
    g = pkg.default_config(64)[1]
    with pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3), pilot_coeffs=b,
                                                diff_gain=pkg.stereo_diff_gain(10, sc.FS), rds_gain=pkg.rds_gain(10, sc.FS), n_streams=len(found),
                                                max_bytes_per_call=row.size)) as bc:
        bc.tune(offsets_hz=tuned, fs=sc.FS, shared_input=True)
        L, R, bb, pc = bc.process_batch(row)
    for f, count in zip(found, pc):
        assert (int(count) > 0.9 * L.shape[1] * 5) == f["stereo"], (f, int(count))
