"""GPU sweep of the stereo handle (sdrfm_stereo_*) over its configuration space: every (T, D, P, Ta, Da) below against
tests/stereo_ref.py (fed the device's own d, which is held to the oracle's d), ragged chunked calls bitwise one call, the kernel each
shape claims, the fast kernel bitwise the generic one;
the call forms (unaligned device rows, wide audio rows, no pilot count, a short single-stream stride); and the value edges of the
carrier gate (pmin2 = +inf, exact ties, denormal pilot power) and of diff_gain (0, negated)."""
import ctypes as C

import numpy as np
import pytest

from conftest import scaled_err
from stereo_ref import oracle_d, stereo_ref

pytestmark = pytest.mark.gpu

TOL = 1e-5
RATE = {8: 2.048e6, 4: 1.024e6, 16: 3.2e6}                      # D -> fs of the dongle rates; 2.4 MS/s otherwise
LDS_BUDGET, FAST_NY = 64 << 10, 1024                            # the host geometry of csrc/sdrfm_stereo.hip

GENERIC = [(1, 1, 1, 1, 1), (7, 3, 3, 5, 4), (23, 10, 101, 32, 5), (16, 8, 65, 32, 8), (64, 4, 101, 64, 8), (64, 16, 51, 32, 5),
           (128, 10, 101, 256, 5), (64, 10, 255, 1, 1), (256, 1, 255, 256, 1), (256, 64, 255, 256, 64)]
FAST = [(64, 10, 101, ta, da) for ta, da in ((1, 1), (1, 64), (2, 2), (2, 7), (255, 7), (255, 1), (256, 64), (256, 2))]
CLASSES = ("stereo", "random", "counter", "const")


def _fs(D):
    return RATE.get(D, 2.4e6)


def _lds(T, D, P, Ta, H, NY, NDT):
    nx, nds = (NY - 1) * D + T + 4, H + NDT + Ta - 1 + NDT
    rw = (max(nx, nds) + 3) & ~3
    return 4 * rw + 8 * NY + 4 * ((H + 1) & ~1) + 8 * P + 4 * Ta + 4 * T


def _ndt(T, D, P, Ta, fast):
    """new d's per step: the fast kernel's fixed NY, or the largest NY the LDS budget allows"""
    if fast:
        return FAST_NY - max(Ta - 1, 1)
    H, ny = P - 1 + Ta - 1, 1024
    while ny > 2 and _lds(T, D, P, Ta, H, ny, ny - 1) > LDS_BUDGET:
        ny -= 2
    return ny - 1


def _taps(pkg, T, D, P, Ta):
    fs = _fs(D)
    h = pkg.lowpass_taps(T, min(120e3 / fs, 0.45))              # (a length of 1 gives the unit tap)
    g = pkg.lowpass_taps(Ta, min(15e3 / (fs / D), 0.45))
    b = pkg.stereo_pilot_taps(P, fs / D) if P > 1 else np.ones(1, np.complex64)
    return h, g, b


def _inputs(pkg, ns, nsamp, D, first_id, first_class=0):
    """ns streams of the input classes in turn; the stereo multiplex only where fs / D carries its 53 kHz, no lone const stream (it has
    no pilot power to place a threshold in)"""
    fs = _fs(D)
    classes = [c for c in CLASSES if c != "stereo" or fs / D >= 106e3]
    rows, names = [], []
    for s in range(ns):
        c = classes[(first_class + s) % len(classes)]
        if ns == 1 and c == "const":
            c = "random"
        if c == "stereo":
            rows.append(pkg.make_iq_stereo(1, nsamp, 1e3 + 70 * s, 3.1e3, 50e3, fs=fs, first_id=first_id + s)[0])
        else:
            rows.append(pkg.make_iq(1, nsamp, mode=c, fs=fs, first_id=first_id + s)[0])
        names.append(c)
    return np.stack(rows), names


def _stereo(pkg, h, g, b, D, Da, ns, nbytes, pm, dg, **kw):
    return pkg.StereoDemod(pkg.StereoConfig(fir_coeffs=h, audio_coeffs=g, pilot_coeffs=b, pilot_min=float(pm), diff_gain=float(dg),
                                            fir_decim=D, audio_decim=Da, n_streams=ns, max_bytes_per_call=nbytes, **kw))


def _pick_pilot_min(pws):
    """a threshold inside the widest relative gap of the pooled pilot powers between their 30 % and 70 % quantiles: the gate is on
    and off within a stream, and as few d's as possible sit at it"""
    u = np.unique(np.concatenate([p[p > 0] for p in pws]).astype(np.float64))
    assert u.size >= 4, "no pilot power to place a threshold in"
    lo, hi = int(0.3 * u.size), max(int(0.7 * u.size), int(0.3 * u.size) + 1)
    i = lo + int(np.argmax(u[lo + 1:hi + 1] / u[lo:hi]))
    return np.float32(np.sqrt(np.sqrt(u[i] * u[i + 1])))


def _ambiguous(ref):
    """d's whose pilot power lies within 1e-3 relative of the threshold (the device's d may fall on either side)"""
    return np.abs(ref["pw"].astype(np.float64) - float(ref["pmin2"])) <= 1e-3 * float(ref["pmin2"])


def _clean_outputs(flag, A, Ta, Da):
    """outputs j whose s-window [(j+1)Da - Ta, (j+1)Da - 1] holds no flagged d"""
    c = np.concatenate([[0], np.cumsum(flag.astype(np.int64))])
    nj = (np.arange(A) + 1) * Da - 1
    lo = np.maximum(nj - Ta + 1, 0)
    return (c[nj + 1] - c[lo]) == 0


def _check_ref(L, R, pc, refs, Ta, Da, where):
    """(a) L, R of every stream against the reference (on the device's d) outside the threshold's neighbourhood; (b) the pilot count within its bounds.
    Returns (worst scaled error, outputs compared, outputs excluded)."""
    worst, n, excl = 0.0, 0, 0
    for s, ref in enumerate(refs):
        assert L[s].shape == ref["L"].shape, (where, s, L[s].shape, ref["L"].shape)
        amb = _ambiguous(ref)
        lo = int((ref["on"] & ~amb).sum())
        assert lo <= int(pc[s]) <= lo + int(amb.sum()), (where, s, int(pc[s]), lo, lo + int(amb.sum()))
        keep = _clean_outputs(amb, ref["L"].size, Ta, Da)
        n, excl = n + int(keep.sum()), excl + int((~keep).sum())
        for got, ch in ((L[s], "L"), (R[s], "R")):
            want = ref[ch][keep].astype(np.float64)
            err = np.abs(got[keep].astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
            if err.size:
                e = float(err.max())
                assert e <= TOL, (where, s, ch, e, int(np.flatnonzero(keep)[np.argmax(err)]))
                worst = max(worst, e)
    return worst, n, excl


def _device_d(pkg, oracle_mod, h, D, iq):
    """d of every stream as the device computes it (a bit-exact mono handle with a one-tap unit audio filter at Da = 1 hands it back),
    held to the oracle's d at TOL.  The stereo stages are compared with the reference on this d: the device's atan2f and libm's differ
    in the last bits, and 255- and 256-tap chains over white-noise d carry that past 1e-5 without any error behind d."""
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


def _chunks(T, D, P, Ta, Da, fast, seed):
    """ragged even byte counts: 0, 2, one shorter than 2 D Da, one whose M is below H, one long enough for >= 3 workgroups per stream,
    then random ones"""
    H, ndt = P - 1 + Ta - 1, _ndt(T, D, P, Ta, fast)
    cuts = [0, 2]
    if D * Da > 2:
        cuts.append(2 * D * Da - 4)
    if H >= 4:
        cuts.append(2 * D * (H // 2) - 2)                          # M <= H / 2
    cuts += [0, 2 * D * (2 * 8 * ndt + ndt // 2) + 6]             # M > 2 workgroups' spans: 3 workgroups at least
    rng = np.random.default_rng(seed)
    cuts += [int(v) for v in 2 * rng.integers(1, D * ndt, 6)]
    return cuts


SHAPES = [("generic", s) for s in GENERIC] + [("fast", s) for s in FAST]


@pytest.mark.parametrize("kind,shape", SHAPES, ids=["%s-T%d-D%d-P%d-Ta%d-Da%d" % ((k,) + s) for k, s in SHAPES])
def test_shape_against_reference_chunks_and_kernels(pkg, oracle_mod, kind, shape):
    T, D, P, Ta, Da = shape
    idx = SHAPES.index((kind, shape))
    ns = (3, 7, 1)[idx % 3]
    h, g, b = _taps(pkg, T, D, P, Ta)
    dg = pkg.stereo_diff_gain(D, _fs(D))
    cuts = _chunks(T, D, P, Ta, Da, kind == "fast", 100 + idx)
    nbytes = sum(cuts)
    iq, names = _inputs(pkg, ns, nbytes // 2, D, 1000 + 10 * idx, idx)
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    pm = _pick_pilot_min([stereo_ref(d, b, g, 1.0, dg, Da)["pw"] for d, c in zip(ds, names) if c != "const"] or
                         [stereo_ref(d, b, g, 1.0, dg, Da)["pw"] for d in ds])
    refs = [stereo_ref(d, b, g, pm, dg, Da) for d in ds]
    assert any(0 < r["count"] < r["pw"].size for r in refs), "the gate is not both on and off in any stream"

    with _stereo(pkg, h, g, b, D, Da, ns, nbytes, pm, dg) as st:
        name = st.kernel_name
        L1, R1, pc1 = st.process_batch(iq)
        assert st.kernel_name == name
        # (d) the kernel the shape claims
        assert name.startswith("stereo-" + kind), (name, shape)
        # (a), (b) against the reference
        worst, n, excl = _check_ref(L1, R1, pc1, refs, Ta, Da, name)
        # (c) the ragged sequence == one call, bitwise
        st.reset()
        Ls, Rs, pcs, pos = [], [], np.zeros(ns, np.int64), 0
        for c in cuts:
            want_n = st.audio_count(c)
            l, r, pc = st.process_batch(iq[:, pos:pos + c])
            assert l.shape[1] == r.shape[1] == want_n, (c, l.shape, want_n)
            Ls.append(l), Rs.append(r)
            pcs += pc
            pos += c
        assert pos == nbytes
        assert np.array_equal(_bits(np.concatenate(Ls, 1)), _bits(L1)) and np.array_equal(_bits(np.concatenate(Rs, 1)), _bits(R1)), name
        assert np.array_equal(pcs, pc1.astype(np.int64)), (pcs, pc1)
    # (e) the fast kernel == the generic one, bitwise
    if kind == "fast":
        with _stereo(pkg, h, g, b, D, Da, ns, nbytes, pm, dg, force_generic=True) as gen:
            assert gen.kernel_name.startswith("stereo-generic"), gen.kernel_name
            L2, R2, pc2 = gen.process_batch(iq)
        assert np.array_equal(_bits(L2), _bits(L1)) and np.array_equal(_bits(R2), _bits(R1)) and np.array_equal(pc2, pc1)
    print("%s: %d streams (%s), pilot_min %.4g, %d chunks bitwise one call, worst scaled error %.3g over %d outputs (%d excluded)" % (
        name, ns, "/".join(names), pm, len(cuts), worst, n, excl))


def _call_device(pkg, st, iq_ptr, iq_stride, nbytes, l_ptr, r_ptr, audio_stride, pc_ptr):
    """sdrfm_stereo_process_batch on raw device addresses (strides the tensor wrapper cannot express)"""
    n = C.c_uint32()
    rc = pkg.load_library().sdrfm_stereo_process_batch(st._h, C.c_void_p(iq_ptr), int(iq_stride), int(nbytes), C.c_void_p(l_ptr),
                                                       C.c_void_p(r_ptr), int(audio_stride), C.c_void_p(pc_ptr) if pc_ptr else None,
                                                       C.byref(n), pkg.lib.F_DEVICE_PTRS)
    assert rc == pkg.lib.OK, rc
    return n.value


@pytest.mark.parametrize("shape", [(23, 10, 101, 32, 5), (64, 10, 101, 32, 5)], ids=["generic", "fast"])
def test_call_forms_bitwise_host_buffers(pkg, shape):
    import torch
    T, D, P, Ta, Da = shape
    ns, nsamp = 3, 30011
    h, g, b = _taps(pkg, T, D, P, Ta)
    dg = pkg.stereo_diff_gain(D, _fs(D))
    iq, _ = _inputs(pkg, ns, nsamp, D, 3000)
    nbytes = 2 * nsamp
    cuts = [2 * 5003, 2 * 7, 0, 2 * 9001, 2]
    cuts.append(nbytes - sum(cuts))
    with _stereo(pkg, h, g, b, D, Da, ns, nbytes, 0.05, dg) as st:
        name = st.kernel_name
        L1, R1, pc1 = st.process_batch(iq)
        A = L1.shape[1]
        # device rows at byte offsets 2, 6, 14, row strides that are not multiples of 16 (the kernel stages x element-wise), ragged calls
        for off, pad in ((2, 2), (6, 4), (14, 6)):
            stride = nbytes + pad
            assert stride % 16 and off % 16
            buf = torch.zeros(ns * stride + 64, dtype=torch.uint8, device="cuda")
            rows = buf[off:off + ns * stride].view(ns, stride)
            rows[:, :nbytes] = torch.from_numpy(iq).cuda()
            d_l = torch.full((ns, A + 5), -7.0, dtype=torch.float32, device="cuda")
            d_r = torch.full((ns, A + 5), -7.0, dtype=torch.float32, device="cuda")
            d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            st.reset()
            Ls, Rs, pcs, pos = [], [], np.zeros(ns, np.int64), 0
            for c in cuts:
                n = st.process_batch_device(rows[:, pos:], d_l, d_r, d_pc, nbytes=c)
                st.synchronize()
                Ls.append(d_l[:, :n].cpu().numpy().copy()), Rs.append(d_r[:, :n].cpu().numpy().copy())
                pcs += d_pc.cpu().numpy().astype(np.int64)
                pos += c
            assert np.array_equal(_bits(np.concatenate(Ls, 1)), _bits(L1)) and np.array_equal(_bits(np.concatenate(Rs, 1)), _bits(R1)), (off, pad)
            assert np.array_equal(pcs, pc1.astype(np.int64)), (off, pad)
        # audio_stride > A: the rows' tails stay untouched; pilot_count = NULL on the device path
        st.reset()
        d_iq = torch.from_numpy(iq).cuda()
        wide = A + 77
        d_l = torch.full((ns, wide), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, wide), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        n = st.process_batch_device(d_iq, d_l, d_r, None)
        st.synchronize()
        assert n == A and d_l.stride(0) == wide
        assert np.array_equal(_bits(d_l[:, :n].cpu().numpy()), _bits(L1)) and np.array_equal(_bits(d_r[:, :n].cpu().numpy()), _bits(R1))
        assert (d_l[:, n:] == -7.0).all() and (d_r[:, n:] == -7.0).all()
    # one stream, iq_stride < nbytes (a single row needs no stride), at an unaligned address
    with _stereo(pkg, h, g, b, D, Da, 1, nbytes, 0.05, dg) as one:
        L0, R0, pc0 = one.process_batch(iq[1:2])
        assert np.array_equal(_bits(L0), _bits(L1[1:2])) and np.array_equal(_bits(R0), _bits(R1[1:2])) and pc0[0] == pc1[1]
        one.reset()
        buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        buf[6:6 + nbytes] = torch.from_numpy(iq[1]).cuda()
        d_l = torch.full((1, A + 3), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((1, A + 3), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        n = _call_device(pkg, one, buf.data_ptr() + 6, 2, nbytes, d_l.data_ptr(), d_r.data_ptr(), 0, d_pc.data_ptr())
        one.synchronize()
        assert n == A
        assert np.array_equal(_bits(d_l[:, :n].cpu().numpy()), _bits(L0)) and np.array_equal(_bits(d_r[:, :n].cpu().numpy()), _bits(R0))
        assert int(d_pc[0]) == int(pc0[0]) and (d_l[:, n:] == -7.0).all()
    print("%s: unaligned rows at offsets 2 / 6 / 14, wide audio rows, no pilot count, one short-stride stream: bitwise the host-buffer "
          "calls (scaled error 0)" % name)


# shapes with P - 1 = 2 K Da: the mono identity L == R == a[j - K] holds where c = 0
MONO_ID = [((1, 1, 1, 1, 1), False), ((16, 8, 65, 32, 8), False), ((64, 16, 51, 32, 5), False), ((64, 10, 255, 1, 1), False),
           ((64, 10, 101, 32, 5), False), ((64, 10, 101, 32, 5), True), ((64, 10, 101, 1, 1), True), ((64, 10, 101, 256, 2), True)]


@pytest.mark.parametrize("shape,generic", MONO_ID, ids=["T%d-D%d-P%d-Ta%d-Da%d" % s + ("-generic" if f else "") for s, f in MONO_ID])
def test_pmin2_inf_is_the_mono_path_shifted(pkg, shape, generic):
    """pilot_min = 1e20: pmin2 = +inf (the header allows it), the gate never opens, pilot_count = 0 and L == R == the bit-exact
    mono audio delayed by K = (P - 1) / (2 Da), bit for bit."""
    T, D, P, Ta, Da = shape
    K = (P - 1) // (2 * Da)
    assert P - 1 == 2 * K * Da
    ns, nsamp = 3, 24000 + 1000 * D
    h, g, b = _taps(pkg, T, D, P, Ta)
    iq, _ = _inputs(pkg, ns, nsamp, D, 5000)
    assert np.float32(1e20) * np.float32(1e20) == np.inf
    with _stereo(pkg, h, g, b, D, Da, ns, 2 * nsamp, 1e20, pkg.stereo_diff_gain(D, _fs(D)), force_generic=generic) as st, \
            pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=ns, bit_exact=True,
                                     max_bytes_per_call=2 * nsamp)) as mono:
        name = st.kernel_name
        assert name.startswith("stereo-generic" if (generic or (T, D, P) != (64, 10, 101)) else "stereo-fast"), name
        L, R, pc = st.process_batch(iq)
        a = mono.process_batch(iq)
    assert L.shape == a.shape and a.shape[1] > K
    shifted = np.concatenate([np.zeros((ns, K), np.float32), a[:, :a.shape[1] - K]], 1)
    assert (pc == 0).all(), pc
    assert np.array_equal(_bits(L), _bits(R)), name
    assert np.array_equal(_bits(L), _bits(shifted)), name
    print("%s: pilot_min 1e20 -> pilot_count 0, L == R == mono audio shifted by %d, %d x %d outputs bitwise" % (name, K, ns, a.shape[1]))


@pytest.mark.parametrize("mode", ["random", "fm"])
def test_gate_ties_count_exactly(pkg, mode):
    """P = 1 with b = (1, 0) and Ta = Da = 1: q = (d, 0), pw = d*d rounded once; a bit-exact mono handle with a one-tap unit audio
    filter hands back the device's own d.  pilot_min = |d_k| makes pmin2 == pw_k exactly, so pilot_count decides >= against >."""
    T, D, ns, nsamp = 64, 10, 2, 40000
    h = pkg.lowpass_taps(T, 120e3 / 2.4e6)
    one = np.ones(1, np.float32)
    b = np.ones(1, np.complex64)
    iq = pkg.make_iq(ns, nsamp, mode=mode, first_id=6000)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=one, fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True,
                                  max_bytes_per_call=2 * nsamp)) as mono:
        d = mono.process_batch(iq)
    ad = np.abs(d[d != 0])
    picks = [np.float32(np.quantile(ad, q, method="nearest")) for q in (0.1, 0.5, 0.9)] + [np.float32(ad.min()), np.float32(ad.max())]
    pw = d * d                                                    # float32 products, rounded once like fmaf(qr, qr, +0)
    ties = 0
    for pm in picks:
        pmin2 = np.float32(pm) * np.float32(pm)
        want = (pw >= pmin2).sum(axis=1)
        ties += int((pw == pmin2).sum())
        with _stereo(pkg, h, one, b, D, 1, ns, 2 * nsamp, pm, 2.0) as st:
            name = st.kernel_name
            assert name.startswith("stereo-generic"), name
            L, R, pc = st.process_batch(iq)
        assert L.shape == d.shape
        assert np.array_equal(pc.astype(np.int64), want.astype(np.int64)), (float(pm), pc, want)
        off = pw < pmin2                                          # c = 0 there: L = R = d
        assert np.array_equal(_bits(L[off]), _bits(d[off])) and np.array_equal(_bits(R[off]), _bits(d[off]))
    assert ties >= len(picks)
    print("%s, gate ties (%s): %d thresholds at |d_k|, %d exact ties, pilot_count == count(d*d >= pmin2) exactly, L == R == d bitwise "
          "where the gate is shut" % (name, mode, len(picks), ties))


@pytest.mark.parametrize("shape", [(23, 10, 101, 32, 5), (64, 10, 101, 32, 5)], ids=["generic", "fast"])
def test_denormal_pilot_power(pkg, oracle_mod, shape):
    """pilot taps and pilot_min scaled by 2^-66: q scales exactly, pw and pmin2 land in fp32's denormal range; the device's gate and
    pilot_count agree with the reference (a kernel that flushed denormals would count nothing)."""
    T, D, P, Ta, Da = shape
    ns, nsamp = 3, 40000
    h, g, b = _taps(pkg, T, D, P, Ta)
    dg = pkg.stereo_diff_gain(D, _fs(D))
    iq = pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 50e3, first_id=7000)
    iq[1] = pkg.make_iq(1, nsamp, mode="random", first_id=7001)[0]
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    pm = _pick_pilot_min([stereo_ref(d, b, g, 1.0, dg, Da)["pw"] for d in ds])
    scale = np.float32(2.0 ** -66)
    bs = (b * scale).astype(np.complex64)
    assert np.array_equal(bs.real, b.real * scale) and np.array_equal(bs.imag, b.imag * scale)
    pms = np.float32(pm * scale)
    refs = [stereo_ref(d, bs, g, pms, dg, Da) for d in ds]
    pmin2 = refs[0]["pmin2"]
    tiny = np.finfo(np.float32).tiny
    assert 0 < pmin2 < tiny, pmin2
    on = sum(r["count"] for r in refs)
    den = sum(int(((r["pw"] > 0) & (r["pw"] < tiny) & r["on"]).sum()) for r in refs)
    assert on > 0 and den > 0, (on, den)
    with _stereo(pkg, h, g, bs, D, Da, ns, 2 * nsamp, pms, dg) as st:
        name = st.kernel_name
        L, R, pc = st.process_batch(iq)
    worst, n, excl = _check_ref(L, R, pc, refs, Ta, Da, name)
    print("%s: denormal gate (pmin2 %.3g), %d d's on (%d of them with a denormal pw), pilot counts %s, worst scaled error %.3g (%d excluded)" % (
        name, float(pmin2), on, den, list(pc), worst, excl))


@pytest.mark.parametrize("shape", [(7, 3, 3, 5, 4), (64, 10, 101, 32, 5), (64, 10, 101, 255, 7)], ids=["generic", "fast", "fast-Ta255"])
def test_diff_gain_zero_and_negated(pkg, oracle_mod, shape):
    """diff_gain = 0: L == R bitwise.  diff_gain negated: s and as change sign exactly, so L(g) == R(-g) and R(g) == L(-g) bitwise."""
    T, D, P, Ta, Da = shape
    ns, nsamp = 3, 40000
    h, g, b = _taps(pkg, T, D, P, Ta)
    dg = pkg.stereo_diff_gain(D, _fs(D))
    iq = pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 50e3, first_id=8000)
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    pm = _pick_pilot_min([stereo_ref(d, b, g, 1.0, dg, Da)["pw"] for d in ds])
    out = {}
    for gain in (dg, -dg, 0.0):
        with _stereo(pkg, h, g, b, D, Da, ns, 2 * nsamp, pm, gain) as st:
            name = st.kernel_name
            out[gain] = st.process_batch(iq)
    (Lp, Rp, pcp), (Ln, Rn, pcn), (L0, R0, pc0) = out[dg], out[-dg], out[0.0]
    assert np.array_equal(_bits(L0), _bits(R0)), name
    assert not np.array_equal(_bits(Lp), _bits(Rp)), "no difference signal: the case does not test the sign"
    assert np.array_equal(_bits(Lp), _bits(Rn)) and np.array_equal(_bits(Rp), _bits(Ln)), name
    assert np.array_equal(pcp, pcn) and np.array_equal(pcp, pc0)
    refs = [stereo_ref(d, b, g, pm, dg, Da) for d in ds]
    worst, _, _ = _check_ref(Lp, Rp, pcp, refs, Ta, Da, name)
    print("%s: diff_gain 0 -> L == R, diff_gain negated -> L and R swap, bitwise; worst scaled error %.3g" % (name, worst))
