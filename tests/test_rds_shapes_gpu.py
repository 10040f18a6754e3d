"""GPU sweep of the RDS handle (sdrfm_rds_*) over its configuration space: every (T, D, P, Tr, Dr) below against tests/rds_ref.py (fed
the device's own d, which is held to the oracle's d), ragged chunked calls bitwise one call, the kernel each shape claims, the fast
kernel bitwise the generic one, the first call's bits again after a reset; and the call forms (host buffers against device pointers,
unaligned device rows, a wide bb_stride, no pilot count, the caller's stream, SDRFM_F_OVERLAP refused).

The helpers that build a case (`case_inputs`, `case_reference`, `excluded_fraction`) take d from a callable, so the reference side of the
sweep can be run without a GPU on the oracle's d (to see that it alone stays inside the 2 % cap on excluded outputs)."""
import ctypes as C

import numpy as np
import pytest

from conftest import scaled_err
from rds_ref import oracle_d, rds_ref

TOL = 1e-5
EXCLUDED_CAP = 0.02                                             # of a case's outputs: a cap, asserted on the reference before comparing
RATE = {8: 2.048e6, 4: 1.024e6, 16: 3.2e6}                      # D -> fs of the dongle rates; 2.4 MS/s otherwise
LDS_BUDGET, FAST_NY = 64 << 10, 1024                            # the host geometry of csrc/sdrfm_rds.hip

GENERIC = [(1, 1, 1, 1, 1), (7, 3, 3, 5, 4), (16, 4, 65, 32, 8), (16, 8, 65, 64, 16), (64, 16, 51, 96, 20), (128, 10, 101, 256, 1),
           (256, 64, 255, 256, 64), (64, 10, 255, 33, 25), (23, 10, 101, 255, 25)]
FAST = [(64, 10, 101, tr, dr) for tr, dr in ((1, 1), (1, 64), (2, 7), (255, 25), (256, 64), (255, 1))]
CLASSES = ("station", "random", "counter", "const")
SHAPES = [("generic", s) for s in GENERIC] + [("fast", s) for s in FAST]
GROUPS = [(0x1234, 0x0408, 0xE0CD, 0x4142), (0x1234, 0x2400, 0x5244, 0x5320), (0x1234, 0x0409, 0xE0CD, 0x4344)]


def _fs(D):
    return RATE.get(D, 2.4e6)


def _lds(T, D, P, Tr, H, NY, NDT):
    zp = (Tr - 1 + NDT) | 1
    nx, nds = (NY - 1) * D + T + 4, H + NDT + 2 * zp
    rw = (max(nx, nds) + 3) & ~3
    return 4 * rw + 8 * NY + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 4 * ((Tr + 3) & ~3) + 4 * T + 8 * (Tr - 1)


def _ndt(T, D, P, Tr, fast):
    """new d's per step: the fast kernel's fixed NY - 1, or the largest the LDS budget allows"""
    if fast:
        return FAST_NY - 1
    H, ny = P - 1 + Tr - 1, 1024
    while ny > 2 and _lds(T, D, P, Tr, H, ny, ny - 1) > LDS_BUDGET:
        ny -= 2
    return ny - 1


def _taps(pkg, T, D, P, Tr):
    fs = _fs(D)
    h = pkg.lowpass_taps(T, min(120e3 / fs, 0.45))              # (a length of 1 gives the unit tap)
    g = pkg.lowpass_taps(Tr, min(3e3 / (fs / D), 0.45))
    b = pkg.stereo_pilot_taps(P, fs / D) if P > 1 else np.ones(1, np.complex64)
    return h, g, b


def _inputs(pkg, ns, nsamp, D, first_id, first_class=0):
    """ns streams of the input classes in turn; the station only where fs / D >= 120 kS/s carries its 57 kHz, no lone const stream (it
    has no pilot power to place a threshold in)"""
    fs = _fs(D)
    classes = [c for c in CLASSES if c != "station" or fs / D >= 120e3]
    rows, names = [], []
    for s in range(ns):
        c = classes[(first_class + s) % len(classes)]
        if ns == 1 and c == "const":
            c = "random"
        if c == "station":
            rows.append(pkg.make_iq_rds(1, nsamp, GROUPS, fs=fs, rds_phase=0.4 * s, first_id=first_id + s)[0])
        else:
            rows.append(pkg.make_iq(1, nsamp, mode=c, fs=fs, first_id=first_id + s)[0])
        names.append(c)
    return np.stack(rows), names


def _pick_pilot_min(pws):
    """a threshold inside the widest relative gap of the pooled pilot powers between their 30 % and 70 % quantiles: the gate is on
    and off within a stream, and as few d's as possible sit at it (the rule of tests/test_stereo_shapes_gpu.py)"""
    u = np.unique(np.concatenate([p[p > 0] for p in pws]).astype(np.float64))
    assert u.size >= 4, "no pilot power to place a threshold in"
    lo, hi = int(0.3 * u.size), max(int(0.7 * u.size), int(0.3 * u.size) + 1)
    i = lo + int(np.argmax(u[lo + 1:hi + 1] / u[lo:hi]))
    return np.float32(np.sqrt(np.sqrt(u[i] * u[i + 1])))


def _ambiguous(ref):
    """d's whose pilot power lies within 1e-3 relative of the threshold (the device's d may fall on either side)"""
    return np.abs(ref["pw"].astype(np.float64) - float(ref["pmin2"])) <= 1e-3 * float(ref["pmin2"])


def _clean_outputs(flag, A, Tr, Dr):
    """outputs j whose z-window [(j+1)Dr - Tr, (j+1)Dr - 1] holds no flagged d"""
    c = np.concatenate([[0], np.cumsum(flag.astype(np.int64))])
    nj = (np.arange(A) + 1) * Dr - 1
    lo = np.maximum(nj - Tr + 1, 0)
    return (c[nj + 1] - c[lo]) == 0


def _chunks(T, D, P, Tr, Dr, fast, seed):
    """ragged even byte counts: 0, 2, one shorter than one output (2 D Dr bytes), one whose M is below H, one long enough for >= 3
    workgroups per stream, then random ones"""
    H, ndt = P - 1 + Tr - 1, _ndt(T, D, P, Tr, fast)
    cuts = [0, 2]
    if D * Dr > 2:
        cuts.append(2 * D * Dr - 4)
    if H >= 4:
        cuts.append(2 * D * (H // 2) - 2)                          # M <= H / 2
    cuts += [0, 2 * D * (2 * 8 * ndt + ndt // 2) + 6]             # M > 2 workgroups' spans: 3 workgroups at least
    rng = np.random.default_rng(seed)
    cuts += [int(v) for v in 2 * rng.integers(1, D * ndt, 6)]
    return cuts


def case_inputs(pkg, kind, shape):
    """everything of a case that does not need a device: (ns, taps, rds_gain, cuts, iq, class names)"""
    T, D, P, Tr, Dr = shape
    idx = SHAPES.index((kind, shape))
    ns = (3, 7, 1)[idx % 3]
    first_class = idx
    if Tr >= 255:
        # a long window spreads every d at the gate over Tr / Dr outputs, so the threshold needs a wide gap to sit in: a station (its pilot
        # powers cluster) beside noise and the counter leaves one between them, which a lone stream does not
        ns, first_class = 3, 0
    h, g, b = _taps(pkg, T, D, P, Tr)
    gain = pkg.rds_gain(D, _fs(D)) if _fs(D) / D >= 120e3 else 2.0
    cuts = _chunks(T, D, P, Tr, Dr, kind == "fast", 100 + idx)
    iq, names = _inputs(pkg, ns, sum(cuts) // 2, D, 1000 + 10 * idx, first_class)
    return ns, (h, g, b), gain, cuts, iq, names


def case_reference(ds, names, b, g, gain, Dr):
    """pilot_min by _pick_pilot_min's rule on the streams that have pilot power, and the reference of every stream at it"""
    pws = [rds_ref(d, b, g, 1.0, gain, Dr)["pw"] for d, c in zip(ds, names) if c != "const"] or [rds_ref(d, b, g, 1.0, gain, Dr)["pw"] for d in ds]
    pm = _pick_pilot_min(pws)
    return pm, [rds_ref(d, b, g, pm, gain, Dr) for d in ds]


def excluded_fraction(refs, Tr, Dr):
    """(fraction of the case's outputs whose window holds a d within 1e-3 of the gate, the per-stream keep masks)"""
    keeps = [_clean_outputs(_ambiguous(r), r["wr"].size, Tr, Dr) for r in refs]
    total = sum(k.size for k in keeps)
    return (sum(int((~k).sum()) for k in keeps) / total if total else 0.0), keeps


def _device_d(pkg, oracle_mod, h, D, iq):
    """d of every stream as the device computes it (a bit-exact mono handle with a one-tap unit audio filter at Da = 1 hands it back),
    held to the oracle's d at TOL"""
    ns = iq.shape[0]
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=np.ones(1, np.float32), fir_decim=D, audio_decim=1, n_streams=ns,
                                  bit_exact=True, max_bytes_per_call=iq.shape[1])) as mono:
        d = mono.process_batch(iq)
    for s in range(ns):
        want = oracle_d(oracle_mod, h, iq[s], D)
        assert d[s].shape == want.shape and scaled_err(d[s], want) <= TOL, s
    return list(d)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rds(pkg, h, g, b, D, Dr, ns, nbytes, pm, gain, **kw):
    return pkg.RdsDemod(pkg.RdsConfig(fir_coeffs=h, rds_coeffs=g, pilot_coeffs=b, pilot_min=float(pm), rds_gain=float(gain), fir_decim=D,
                                      rds_decim=Dr, n_streams=ns, max_bytes_per_call=max(nbytes, 2), **kw))


def _check_ref(bb, pc, refs, keeps, where):
    """(a) w of every stream against the reference (on the device's d) outside the threshold's neighbourhood; (b) the pilot count
    within its bounds.  Returns (worst scaled error, outputs compared)."""
    worst, n = 0.0, 0
    for s, (ref, keep) in enumerate(zip(refs, keeps)):
        assert bb[s].shape == ref["wr"].shape, (where, s, bb[s].shape, ref["wr"].shape)
        amb = _ambiguous(ref)
        lo = int((ref["on"] & ~amb).sum())
        assert lo <= int(pc[s]) <= lo + int(amb.sum()), (where, s, int(pc[s]), lo, lo + int(amb.sum()))
        n += int(keep.sum())
        for got, ch in ((bb[s].real, "wr"), (bb[s].imag, "wi")):
            want = ref[ch][keep].astype(np.float64)
            err = np.abs(got[keep].astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
            if err.size:
                e = float(err.max())
                assert e <= TOL, (where, s, ch, e, int(np.flatnonzero(keep)[np.argmax(err)]))
                worst = max(worst, e)
    return worst, n


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", SHAPES, ids=["%s-T%d-D%d-P%d-Tr%d-Dr%d" % ((k,) + s) for k, s in SHAPES])
def test_shape_against_reference_chunks_and_kernels(pkg, oracle_mod, kind, shape):
    T, D, P, Tr, Dr = shape
    ns, (h, g, b), gain, cuts, iq, names = case_inputs(pkg, kind, shape)
    nbytes = sum(cuts)
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    pm, refs = case_reference(ds, names, b, g, gain, Dr)
    assert any(0 < r["count"] < r["pw"].size for r in refs), "the gate is not both on and off in any stream"
    frac, keeps = excluded_fraction(refs, Tr, Dr)
    print("pilot_min %.4g: %.3f %% of the outputs excluded" % (pm, 100 * frac))
    assert frac <= EXCLUDED_CAP, frac

    with _rds(pkg, h, g, b, D, Dr, ns, nbytes, pm, gain) as rd:
        name = rd.kernel_name
        bb1, pc1 = rd.process_batch(iq)
        assert rd.kernel_name == name
        # the kernel the shape claims
        assert name.startswith("rds-" + kind), (name, shape)
        # against the reference
        worst, n = _check_ref(bb1, pc1, refs, keeps, name)
        # the ragged sequence == one call, bitwise
        rd.reset()
        parts, pcs, pos, first = [], np.zeros(ns, np.int64), 0, None
        for c in cuts:
            want_n = rd.count(c)
            w, pc = rd.process_batch(iq[:, pos:pos + c])
            assert w.shape[1] == want_n, (c, w.shape, want_n)
            parts.append(w)
            pcs += pc
            pos += c
        assert pos == nbytes
        assert np.array_equal(_bits(np.concatenate(parts, 1)), _bits(bb1)), name
        assert np.array_equal(pcs, pc1.astype(np.int64)), (pcs, pc1)
        # after a reset the first call's bits again
        rd.reset()
        big = max(cuts)
        w_a, pc_a = rd.process_batch(iq[:, :big])
        rd.reset()
        w_b, pc_b = rd.process_batch(iq[:, :big])
        assert np.array_equal(_bits(w_a), _bits(w_b)) and np.array_equal(pc_a, pc_b)
        assert np.array_equal(_bits(w_a), _bits(bb1[:, :w_a.shape[1]]))
    # the fast kernel == the generic one, bitwise
    if kind == "fast":
        with _rds(pkg, h, g, b, D, Dr, ns, nbytes, pm, gain, force_generic=True) as gen:
            assert gen.kernel_name.startswith("rds-generic"), gen.kernel_name
            bb2, pc2 = gen.process_batch(iq)
        assert np.array_equal(_bits(bb2), _bits(bb1)) and np.array_equal(pc2, pc1)
    print("%s: %d streams (%s), pilot_min %.4g, %d chunks bitwise one call, worst scaled error %.3g over %d outputs (%.3f %% excluded)" % (
        name, ns, "/".join(names), pm, len(cuts), worst, n, 100 * frac))


def _call_device(pkg, rd, iq_ptr, iq_stride, nbytes, bb_ptr, bb_stride, pc_ptr, flags=None):
    """sdrfm_rds_process_batch on raw device addresses (strides the tensor wrapper cannot express)"""
    n = C.c_uint32()
    rc = pkg.load_library().sdrfm_rds_process_batch(rd._h, C.c_void_p(iq_ptr), int(iq_stride), int(nbytes), C.c_void_p(bb_ptr), int(bb_stride),
                                                    C.c_void_p(pc_ptr) if pc_ptr else None, C.byref(n),
                                                    pkg.lib.F_DEVICE_PTRS if flags is None else flags)
    return rc, n.value


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(23, 10, 101, 64, 25), (64, 10, 101, 255, 25)], ids=["generic", "fast"])
def test_call_forms_bitwise_host_buffers(pkg, shape):
    import torch
    T, D, P, Tr, Dr = shape
    ns, nsamp = 3, 60011
    h, g, b = _taps(pkg, T, D, P, Tr)
    gain = pkg.rds_gain(D, _fs(D))
    iq, _ = _inputs(pkg, ns, nsamp, D, 3000)
    nbytes = 2 * nsamp
    cuts = [2 * 5003, 2 * 7, 0, 2 * 29001, 2]
    cuts.append(nbytes - sum(cuts))
    with _rds(pkg, h, g, b, D, Dr, ns, nbytes, 0.05, gain) as rd:
        name = rd.kernel_name
        bb1, pc1 = rd.process_batch(iq)
        A = bb1.shape[1]
        ref_f = np.ascontiguousarray(bb1).view(np.float32)          # [ns, 2A]
        # device rows at byte offsets 2, 6, 14, row strides that are not multiples of 16 (the kernel stages x element-wise), ragged calls
        for off, pad in ((2, 2), (6, 4), (14, 6)):
            stride = nbytes + pad
            assert stride % 16 and off % 16
            buf = torch.zeros(ns * stride + 64, dtype=torch.uint8, device="cuda")
            rows = buf[off:off + ns * stride].view(ns, stride)
            rows[:, :nbytes] = torch.from_numpy(iq).cuda()
            d_bb = torch.full((ns, 2 * A + 6), -7.0, dtype=torch.float32, device="cuda")
            d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rd.reset()
            parts, pcs, pos = [], np.zeros(ns, np.int64), 0
            for c in cuts:
                n = rd.process_batch_device(rows[:, pos:], d_bb, d_pc, nbytes=c)
                rd.synchronize()
                parts.append(d_bb[:, :2 * n].cpu().numpy().copy())
                pcs += d_pc.cpu().numpy().astype(np.int64)
                pos += c
            assert np.array_equal(_bits(np.concatenate(parts, 1)), _bits(ref_f)), (off, pad)
            assert np.array_equal(pcs, pc1.astype(np.int64)), (off, pad)
        # bb_stride > 2 A: the rows' tails stay untouched; pilot_count = NULL on the device path; the caller's stream
        rd.reset()
        d_iq = torch.from_numpy(iq).cuda()
        wide = 2 * A + 77
        d_bb = torch.full((ns, wide), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mine = torch.cuda.Stream()
        rd.set_stream(mine.cuda_stream)
        n = rd.process_batch_device(d_iq, d_bb, None)
        mine.synchronize()
        rd.set_stream(None)
        assert n == A and d_bb.stride(0) == wide
        assert np.array_equal(_bits(d_bb[:, :2 * n].cpu().numpy()), _bits(ref_f))
        assert (d_bb[:, 2 * n:] == -7.0).all()
        # SDRFM_F_OVERLAP is not for this handle; a bb_stride below 2 A is refused
        rc, _ = _call_device(pkg, rd, d_iq.data_ptr(), d_iq.stride(0), nbytes, d_bb.data_ptr(), wide, 0, flags=pkg.lib.F_DEVICE_PTRS | pkg.lib.F_OVERLAP)
        assert rc == pkg.lib.EINVAL
        rc, _ = _call_device(pkg, rd, d_iq.data_ptr(), d_iq.stride(0), nbytes, d_bb.data_ptr(), 2 * A - 1, 0)
        assert rc == pkg.lib.ECAPACITY
        rd.reset()
        again, _ = rd.process_batch(iq)                              # (the refused calls left the state alone)
        assert np.array_equal(_bits(again), _bits(bb1))
    # one stream, iq_stride < nbytes (a single row needs no stride), at an unaligned address
    with _rds(pkg, h, g, b, D, Dr, 1, nbytes, 0.05, gain) as one:
        bb0, pc0 = one.process_batch(iq[1:2])
        assert np.array_equal(_bits(bb0), _bits(bb1[1:2])) and pc0[0] == pc1[1]
        one.reset()
        buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        buf[6:6 + nbytes] = torch.from_numpy(iq[1]).cuda()
        d_bb = torch.full((1, 2 * A + 3), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc, n = _call_device(pkg, one, buf.data_ptr() + 6, 2, nbytes, d_bb.data_ptr(), 0, d_pc.data_ptr())
        one.synchronize()
        assert rc == pkg.lib.OK and n == A
        assert np.array_equal(_bits(d_bb[:, :2 * n].cpu().numpy()), _bits(np.ascontiguousarray(bb0).view(np.float32)))
        assert int(d_pc[0]) == int(pc0[0]) and (d_bb[:, 2 * n:] == -7.0).all()
    print("%s: unaligned rows at offsets 2 / 6 / 14, wide bb rows, no pilot count, the caller's stream, one short-stride stream: bitwise the "
          "host-buffer calls; SDRFM_F_OVERLAP refused" % name)
