"""GPU sweep of the broadcast receiver handle (sdrfm_bcast_*) over its configuration space.  The reference is the pair of handles it
stands for, on the same box: for every (T, D, P, Ta, Da, Tr, Dr) below L and R are the StereoDemod's and bb is the RdsDemod's, bit against
bit (the existing sweeps hold those two to tests/stereo_ref.py and tests/rds_ref.py), so no output is excluded.  Then: a ragged sequence
of calls bitwise the one call with counts() right before every call, the kernel each shape claims, the fast kernel bitwise the generic
one, the first call's bits again after a reset."""
import numpy as np
import pytest

from test_rds_shapes_gpu import GROUPS, _bits, _fs, _pick_pilot_min

pytestmark = pytest.mark.gpu

LDS_BUDGET, FAST_NY = 64 << 10, 1024                            # the host geometry of csrc/sdrfm_bcast.hip

GENERIC = [(1, 1, 1, 1, 1, 1, 1), (7, 3, 3, 5, 4, 9, 2), (16, 8, 65, 64, 16, 32, 5), (23, 10, 101, 32, 5, 255, 25), (128, 10, 101, 256, 5, 1, 1),
           (256, 64, 255, 256, 64, 256, 64)]
FAST = [(64, 10, 101, ta, da, tr, dr) for ta, da, tr, dr in ((32, 5, 255, 25), (1, 1, 1, 1), (256, 64, 2, 7), (2, 7, 256, 64), (255, 1, 255, 1))]
SHAPES = [("generic", s) for s in GENERIC] + [("fast", s) for s in FAST]


def _lds(T, D, P, Ta, Tr, H, NY, NDT):
    zp = (Tr - 1 + NDT) | 1
    nx, nds = (NY - 1) * D + T + 4, H + NDT + (Ta - 1 + NDT) + 2 * zp
    rw = (max(nx, nds) + 3) & ~3
    return 4 * rw + 8 * NY + 4 * ((H + 3) & ~3) + 8 * ((P + 1) & ~1) + 4 * ((Tr + 3) & ~3) + 4 * Ta + 4 * T + 8 * (Tr - 1) + 4 * (Ta - 1)


def _ndt(T, D, P, Ta, Tr, fast):
    """new d's per step: the fast kernel's fixed NY - 1, or the largest the LDS budget allows"""
    H = P - 1 + max(Ta, Tr) - 1
    if fast:
        assert _lds(64, 10, 101, Ta, Tr, H, FAST_NY, FAST_NY - 1) <= LDS_BUDGET
        return FAST_NY - 1
    ny = 1024
    while ny > 2 and _lds(T, D, P, Ta, Tr, H, ny, ny - 1) > LDS_BUDGET:
        ny -= 2
    return ny - 1


def _split(M, ndt, H, ns, slots):
    """(workgroups per stream, new d's per workgroup) of a call, as bcast_enqueue chooses them"""
    bps, best = 1, None
    for k in range(1, min((M + ndt - 1) // ndt, 64) + 1):
        cost = ((ns * k + slots - 1) // slots) * ((M + k - 1) // k + H // 2 + 64)
        if best is None or cost < best:
            best, bps = cost, k
    return bps, (M + bps - 1) // bps


def _taps(pkg, T, D, P, Ta, Tr):
    fs = _fs(D)
    h = pkg.lowpass_taps(T, min(120e3 / fs, 0.45))              # (a length of 1 gives the unit tap)
    ga = pkg.lowpass_taps(Ta, min(15e3 / (fs / D), 0.45))
    gr = pkg.lowpass_taps(Tr, min(3e3 / (fs / D), 0.45))
    b = pkg.stereo_pilot_taps(P, fs / D) if P > 1 else np.ones(1, np.complex64)
    return h, ga, gr, b


_stations = {}


def _station(pkg, fs, k, nsamp):
    """station k at fs (pilot, stereo multiplex, RDS), made once at the longest length asked for so far"""
    have = _stations.get((fs, k))
    if have is None or have.size < 2 * nsamp:
        have = pkg.make_iq_rds(1, max(nsamp, 740000), GROUPS, fs=fs, rds_phase=0.4 * k, first_id=4000 + k)[0]
        have.setflags(write=False)
        _stations[(fs, k)] = have
    return have[:2 * nsamp]


def _inputs(pkg, ns, nsamp, D, first_id):
    """ns streams: a station (where fs / D >= 120 kS/s carries its 57 kHz), then random / counter / const in turn; no lone const stream"""
    fs = _fs(D)
    classes = (["station"] if fs / D >= 120e3 else []) + ["random", "counter", "const"]
    rows, names = [], []
    for s in range(ns):
        c = classes[s % len(classes)]
        rows.append(_station(pkg, fs, s, nsamp) if c == "station" else pkg.make_iq(1, nsamp, mode=c, fs=fs, first_id=first_id + s)[0])
        names.append(c)
    return np.stack(rows), names


def _pilot_powers(pkg, h, b, D, iq, names):
    """|q|^2 of every stream that has any, q = b * d on the device's own d (a bit-exact mono handle with a one-tap unit audio filter at
    Da = 1 hands d back); in float64: it only places the threshold"""
    ns = iq.shape[0]
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=np.ones(1, np.float32), fir_decim=D, audio_decim=1, n_streams=ns, bit_exact=True,
                                  max_bytes_per_call=iq.shape[1])) as mono:
        d = mono.process_batch(iq)
    pws = [(np.abs(np.convolve(d[s].astype(np.float64), np.asarray(b, np.complex128))[:d.shape[1]]) ** 2).astype(np.float32) for s in range(ns)]
    return [p for p, c in zip(pws, names) if c != "const"] or pws


def _chunks(T, D, P, Ta, Da, Tr, Dr, fast, seed):
    """ragged even byte counts: 0, 2, one shorter than one audio output (2 D Da bytes), one shorter than one RDS output, one whose M is
    below H / 2, a second 0, one of more than 64 steps (the split gives a stream 64 workgroups at the most, so each walks two steps at
    least), then six random ones"""
    H, ndt = P - 1 + max(Ta, Tr) - 1, _ndt(T, D, P, Ta, Tr, fast)
    cuts = [0, 2]
    if D * Da > 2:
        cuts.append(2 * D * Da - 4)
    if D * Dr > 2:
        cuts.append(2 * D * Dr - 4)
    if H >= 4:
        cuts.append(2 * D * (H // 2) - 2)                          # M <= H / 2
    long_ = 2 * D * (64 * ndt + ndt // 2) + 6
    cuts += [0, long_]
    rng = np.random.default_rng(seed)
    cuts += [int(v) for v in 2 * rng.integers(1, D * ndt, 6)]
    return cuts, long_, ndt, H


@pytest.mark.parametrize("kind,shape", SHAPES, ids=["%s-T%d-D%d-P%d-Ta%d-Da%d-Tr%d-Dr%d" % ((k,) + s) for k, s in SHAPES])
def test_shape_is_the_two_handles_bitwise_chunks_and_kernels(pkg, kind, shape):
    import torch
    T, D, P, Ta, Da, Tr, Dr = shape
    idx = SHAPES.index((kind, shape))
    ns = (3, 7, 1)[idx % 3]
    fs = _fs(D)
    h, ga, gr, b = _taps(pkg, T, D, P, Ta, Tr)
    dg = pkg.stereo_diff_gain(D, fs)
    rg = pkg.rds_gain(D, fs) if fs / D >= 120e3 else 2.0
    cuts, long_, ndt, H = _chunks(T, D, P, Ta, Da, Tr, Dr, kind == "fast", 100 + idx)
    nbytes = sum(cuts)
    iq, names = _inputs(pkg, ns, nbytes // 2, D, 1000 + 10 * idx)
    pm = _pick_pilot_min(_pilot_powers(pkg, h, b, D, iq, names))
    # the long call's geometry, whichever occupancy the kernel has: >= 3 workgroups per stream, >= 2 steps per workgroup
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (1, 2):
        bps, span = _split(long_ // 2 // D, ndt, H, ns, per_cu * cus)
        assert bps >= 3 and span > ndt, (bps, span, ndt)

    common = dict(fir_coeffs=h, pilot_coeffs=b, pilot_min=float(pm), fir_decim=D, n_streams=ns, max_bytes_per_call=nbytes)
    bcfg = dict(common, audio_coeffs=ga, rds_coeffs=gr, diff_gain=float(dg), rds_gain=float(rg), audio_decim=Da, rds_decim=Dr)
    with pkg.StereoDemod(pkg.StereoConfig(audio_coeffs=ga, diff_gain=float(dg), audio_decim=Da, **common)) as st:
        Ls, Rs, pcs = st.process_batch(iq)
    with pkg.RdsDemod(pkg.RdsConfig(rds_coeffs=gr, rds_gain=float(rg), rds_decim=Dr, **common)) as rd:
        bbs, pcr = rd.process_batch(iq)
    M = nbytes // 2 // D
    assert np.array_equal(pcs, pcr)
    assert any(0 < int(c) < M for c in pcs), ("the gate is not both on and off in any stream", list(pcs), M)

    with pkg.BroadcastDemod(pkg.BroadcastConfig(**bcfg)) as bc:
        name = bc.kernel_name
        assert bc.counts(nbytes) == (Ls.shape[1], bbs.shape[1])
        L1, R1, bb1, pc1 = bc.process_batch(iq)
        assert bc.kernel_name == name
        # (c) the kernel the shape claims
        want_name = ("bcast-fast T64 D10 P101 Ta%d Da%d Tr%d Dr%d" % (Ta, Da, Tr, Dr) if kind == "fast" else
                     "bcast-generic T%d D%d P%d Ta%d Da%d Tr%d Dr%d" % shape)
        assert name == want_name, (name, want_name)
        # (a) one call: L, R the stereo handle's, bb the RDS handle's, the pilot count both's
        assert L1.shape == Ls.shape and R1.shape == Rs.shape and bb1.shape == bbs.shape
        assert np.array_equal(_bits(L1), _bits(Ls)), (name, "L")
        assert np.array_equal(_bits(R1), _bits(Rs)), (name, "R")
        assert np.array_equal(_bits(bb1), _bits(bbs)), (name, "bb")
        assert np.array_equal(pc1, pcs) and np.array_equal(pc1, pcr), (pc1, pcs, pcr)
        # (b) the ragged sequence == the one call, bitwise; counts() before every call
        bc.reset()
        parts, pct, pos = ([], [], []), np.zeros(ns, np.int64), 0
        px = pa = pr = 0
        for c in cuts:
            m = (px + c // 2) // D
            want = ((pa + m) // Da, (pr + m) // Dr)
            px, pa, pr = (px + c // 2) % D, (pa + m) % Da, (pr + m) % Dr
            assert bc.counts(c) == want, (c, bc.counts(c), want)
            l, r, w, pc = bc.process_batch(iq[:, pos:pos + c])
            assert (l.shape[1], r.shape[1], w.shape[1]) == (want[0], want[0], want[1]), (c, l.shape, r.shape, w.shape, want)
            for acc, v in zip(parts, (l, r, w)):
                acc.append(v)
            pct += pc
            pos += c
        assert pos == nbytes
        for acc, one, what in zip(parts, (L1, R1, bb1), "LRw"):
            assert np.array_equal(_bits(np.concatenate(acc, 1)), _bits(one)), (name, what)
        assert np.array_equal(pct, pc1.astype(np.int64)), (pct, pc1)
        # (e) after a reset the first call's bits again
        bc.reset()
        l, r, w, pc = bc.process_batch(iq[:, :long_])
        assert l.shape[1] > 0 and w.shape[1] > 0
        assert np.array_equal(_bits(l), _bits(L1[:, :l.shape[1]])) and np.array_equal(_bits(r), _bits(R1[:, :r.shape[1]]))
        assert np.array_equal(_bits(w), _bits(bb1[:, :w.shape[1]]))
    # (d) the fast kernel == the generic one, bitwise
    if kind == "fast":
        with pkg.BroadcastDemod(pkg.BroadcastConfig(force_generic=True, **bcfg)) as gen:
            assert gen.kernel_name == "bcast-generic T64 D10 P101 Ta%d Da%d Tr%d Dr%d" % (Ta, Da, Tr, Dr), gen.kernel_name
            L2, R2, bb2, pc2 = gen.process_batch(iq)
        assert np.array_equal(_bits(L2), _bits(L1)) and np.array_equal(_bits(R2), _bits(R1)) and np.array_equal(_bits(bb2), _bits(bb1))
        assert np.array_equal(pc2, pc1)
    print("%s: %d streams (%s), pilot_min %.4g, pilot counts %s of %d; L, R, bb bitwise the two handles' over %d + %d outputs a stream; "
          "%d chunks bitwise one call" % (name, ns, "/".join(names), pm, list(pc1), M, L1.shape[1], bb1.shape[1], len(cuts)))
