"""GPU checks of the stereo handle (sdrfm_stereo_*): bit-identical to the mono bit-exact path where there is no pilot, within the
tolerance of tests/stereo_ref.py everywhere, channel separation on the device's own output, streaming and call modes bit-identical,
the fast kernel serving the BASELINE configs[2] shape."""
import ctypes as C

import numpy as np
import pytest

from stereo_ref import oracle_d, separation_db, stereo_ref

pytestmark = pytest.mark.gpu

FS, D, DA, P = 2.4e6, 10, 5, 101
K = (P - 1) // 2 // DA        # Δ = K Da


def _taps(pkg, T=64):
    h = pkg.lowpass_taps(T, 120e3 / FS)                          # the channel filter of the separation figures
    g = pkg.default_config()[1]
    return h, g, pkg.stereo_pilot_taps(P, FS / D)


def _stereo(pkg, h, g, b, ns, nbytes, dg=2.0, **kw):
    return pkg.StereoDemod(pkg.StereoConfig(fir_coeffs=h, audio_coeffs=g, pilot_coeffs=b, pilot_min=0.05, diff_gain=dg, n_streams=ns,
                                            max_bytes_per_call=nbytes, **kw))


def _ambiguous(ref):
    """d's whose pilot power lies within 1e-3 relative of the threshold (the device's d may fall on either side)"""
    return np.abs(ref["pw"].astype(np.float64) - float(ref["pmin2"])) <= 1e-3 * float(ref["pmin2"])


def _clean_outputs(on_or_amb, A, Ta):
    """outputs j whose s-window [(j+1)Da - Ta, (j+1)Da - 1] holds no flagged d"""
    c = np.concatenate([[0], np.cumsum(on_or_amb.astype(np.int64))])
    nj = (np.arange(A) + 1) * DA - 1
    lo = np.maximum(nj - Ta + 1, 0)
    return (c[nj + 1] - c[lo]) == 0


@pytest.mark.parametrize("urb", [False, True], ids=["one_call", "urb_512"])
def test_mono_identity_bitwise(pkg, oracle_mod, urb):
    ns, nsamp = 64, 240000
    h, g, b = _taps(pkg)
    iq = pkg.make_iq(ns, nsamp, mode="fm", first_id=40)
    chunks = [(0, 2 * nsamp)] if not urb else [(o, min(o + 512, 2 * nsamp)) for o in range(0, 2 * nsamp, 512)]
    with _stereo(pkg, h, g, b, ns, 2 * nsamp if not urb else 512) as st, \
            pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, bit_exact=True, max_bytes_per_call=2 * nsamp)) as mono:
        L, R, A, pcs = [], [], [], np.zeros(ns, np.int64)
        for lo, hi in chunks:
            l, r, pc = st.process_batch(iq[:, lo:hi])
            a = mono.process_batch(iq[:, lo:hi])
            assert l.shape == a.shape
            L.append(l), R.append(r), A.append(a)
            pcs += pc
        L, R, A = np.concatenate(L, 1), np.concatenate(R, 1), np.concatenate(A, 1)
    na = A.shape[1]
    shifted = np.concatenate([np.zeros((ns, K), np.float32), A[:, : na - K]], 1)
    ramp_streams = 0
    for s in range(ns):
        ref = stereo_ref(oracle_d(oracle_mod, h, iq[s], D), b, g, 0.05, 2.0, DA)
        amb = _ambiguous(ref)
        assert not ref["on"][2 * P:].any(), s                    # a mono input: nothing after the pilot filter's ramp-up
        if ref["count"]:
            ramp_streams += 1
        if not amb.any():
            assert pcs[s] == ref["count"], (s, pcs[s], ref["count"])
        clean = _clean_outputs(ref["on"] | amb, na, g.size)
        assert np.array_equal(L[s][clean], R[s][clean]), s
        assert np.array_equal(L[s][clean], shifted[s][clean]), s
        if not ref["on"].any() and not amb.any():
            assert pcs[s] == 0 and np.array_equal(L[s], R[s]) and np.array_equal(L[s], shifted[s]), s
    print("mono identity (%s): %d streams x %d outputs bitwise, %d streams cross pilot_min in the ramp-up" % (
        "URB calls" if urb else "one call", ns, na, ramp_streams))


@pytest.fixture(scope="module")
def big_run(pkg, oracle_mod):
    ns, nsamp = 256, 240000
    h, g, b = _taps(pkg)
    lhz = 1000.0 + 50.0 * (np.arange(ns) % 7)
    rhz = 3100.0 + 70.0 * (np.arange(ns) % 5)
    iq = pkg.make_iq_stereo(ns, nsamp, lhz, rhz, 50e3, first_id=100)
    dg = pkg.stereo_diff_gain(D, FS)
    with _stereo(pkg, h, g, b, ns, 2 * nsamp, dg=dg) as st:
        name = st.kernel_name
        L, R, pc = st.process_batch(iq)
        name_after = st.kernel_name
    return dict(ns=ns, h=h, g=g, b=b, iq=iq, dg=dg, L=L, R=R, pc=pc, name=name, name_after=name_after, lhz=lhz, rhz=rhz)


def test_against_the_reference(pkg, oracle_mod, big_run):
    r = big_run
    worst, excluded, nout = 0.0, 0, 0
    for s in range(r["ns"]):
        ref = stereo_ref(oracle_d(oracle_mod, r["h"], r["iq"][s], D), r["b"], r["g"], 0.05, r["dg"], DA)
        assert r["L"][s].shape == ref["L"].shape
        amb = _ambiguous(ref)
        on_new = ref["on"] & ~amb
        lo, hi = int(on_new.sum()), int(on_new.sum() + amb.sum())
        assert lo <= r["pc"][s] <= hi, (s, r["pc"][s], lo, hi)
        keep = _clean_outputs(amb, ref["L"].size, r["g"].size)
        excluded += int((~keep).sum())
        nout += keep.size
        for ch in ("L", "R"):
            want = ref[ch][keep].astype(np.float64)
            err = np.abs(r[ch][s][keep] - want) / np.maximum(np.abs(want), 1.0)
            worst = max(worst, float(err.max()))
    print("stereo vs reference: %d streams, worst scaled error %.3g, %d of %d outputs excluded (pilot power at the threshold)" % (
        r["ns"], worst, excluded, nout))
    assert worst <= 1e-5


def test_separation_on_the_device_output(pkg, big_run):
    r = big_run
    worst = (1e9, 1e9)
    for s in range(0, r["ns"], 17):
        # this stream's composite carries both tones: L = lhz, R = rhz
        sep_l, sep_r, (l_l, l_r, r_l, r_r) = separation_db(r["L"][s], r["R"][s], r["lhz"][s], r["rhz"][s])
        assert l_l > 10 * r_l and r_r > 10 * l_r, s             # channel order
        worst = (min(worst[0], sep_l), min(worst[1], sep_r))
    print("device separation (diff_gain %.4f): worst L %.1f dB, worst R %.1f dB" % (r["dg"], worst[0], worst[1]))
    assert worst[0] >= 40.0 and worst[1] >= 40.0


def test_configs2_shape_runs_the_fast_kernel(pkg, big_run):
    assert big_run["name"].startswith("stereo-fast") and big_run["name_after"].startswith("stereo-fast"), big_run["name"]


def test_capacity_checks(pkg):
    import torch
    h, g, b = _taps(pkg)
    lib = pkg.load_library()
    with _stereo(pkg, h, g, b, 4, 4096) as st:
        iq = torch.zeros((4, 8192), dtype=torch.uint8, device="cuda")
        out = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
        n = C.c_uint32()
        rc = lib.sdrfm_stereo_process_batch(st._h, C.c_void_p(iq.data_ptr()), 8192, 4098, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(out.data_ptr()), 64, None, C.byref(n), pkg.lib.F_DEVICE_PTRS)
        assert rc == pkg.lib.ECAPACITY
        A = st.audio_count(4000)
        rc = lib.sdrfm_stereo_process_batch(st._h, C.c_void_p(iq.data_ptr()), 8192, 4000, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(out.data_ptr()), A - 1, None, C.byref(n), pkg.lib.F_DEVICE_PTRS)
        assert rc == pkg.lib.ECAPACITY
        rc = lib.sdrfm_stereo_process_batch(st._h, C.c_void_p(iq.data_ptr()), 8192, 4000, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(out.data_ptr()), 64, None, C.byref(n), pkg.lib.F_DEVICE_PTRS | pkg.lib.F_OVERLAP)
        assert rc == pkg.lib.EINVAL
        st.synchronize()


@pytest.mark.parametrize("T,generic", [(64, False), (64, True), (23, True)], ids=["fast", "forced_generic", "generic_T23"])
def test_streaming_and_call_modes_are_bitwise_one_call(pkg, T, generic):
    import torch
    ns, nsamp = 8, 60000
    h, g, b = _taps(pkg, T)
    iq = pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 50e3, first_id=7)
    dg = pkg.stereo_diff_gain(D, FS)
    with _stereo(pkg, h, g, b, ns, 2 * nsamp, dg=dg, force_generic=generic) as st:
        L1, R1, pc1 = st.process_batch(iq)
        name = st.kernel_name
        assert name.startswith("stereo-generic" if (generic or T != 64) else "stereo-fast"), name
        # random even chunks: odd decimator phases, one shorter than an audio period (2 D Da = 100 bytes)
        rng = np.random.default_rng(11)
        cuts = sorted(set([0, 2 * nsamp, 38, 38 + 64, 1000 + 6] + list(2 * rng.integers(1, nsamp, 12))))
        st.reset()
        mono = pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, bit_exact=True, max_bytes_per_call=2 * nsamp))
        Ls, Rs, pcs = [], [], np.zeros(ns, np.int64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            want_n = mono.audio_count(hi - lo)
            l, r, pc = st.process_batch(iq[:, lo:hi])
            assert l.shape[1] == want_n, (lo, hi)
            mono.process_batch(iq[:, lo:hi])
            Ls.append(l), Rs.append(r)
            pcs += pc
        mono.close()
        assert np.array_equal(np.concatenate(Ls, 1), L1) and np.array_equal(np.concatenate(Rs, 1), R1)
        assert np.array_equal(pcs, pc1)
        # reset + the same input == a fresh handle
        st.reset()
        L2, R2, pc2 = st.process_batch(iq)
        assert np.array_equal(L2, L1) and np.array_equal(R2, R1) and np.array_equal(pc2, pc1)
        # device pointers == host buffers
        st.reset()
        d_iq = torch.from_numpy(iq).cuda()
        cap = L1.shape[1] + 3
        d_l = torch.full((ns, cap), 7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, cap), 7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.full((ns,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        n = st.process_batch_device(d_iq, d_l, d_r, d_pc)
        st.synchronize()
        assert n == L1.shape[1]
        assert np.array_equal(d_l[:, :n].cpu().numpy(), L1) and np.array_equal(d_r[:, :n].cpu().numpy(), R1)
        assert np.array_equal(d_pc.cpu().numpy().astype(np.int64), pc1.astype(np.int64))
        assert (d_l[:, n:] == 7.0).all() and (d_r[:, n:] == 7.0).all()
    if T == 64:
        # the fast and the generic kernel give the same bits
        with _stereo(pkg, h, g, b, ns, 2 * nsamp, dg=dg, force_generic=not generic) as other:
            L3, R3, pc3 = other.process_batch(iq)
        assert np.array_equal(L3, L1) and np.array_equal(R3, R1) and np.array_equal(pc3, pc1)
    print("%s: %d chunks bitwise one call; host == device; reset == fresh" % (name, len(cuts) - 1))
