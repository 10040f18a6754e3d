"""GPU checks of the broadcast receiver handle (sdrfm_bcast_*) at the default shape: against the written definitions (tests/stereo_ref.py,
tests/rds_ref.py) on station input, the call forms bitwise the host-buffer call, the refusals, and the receiver end to end — the PS name
and the radio text through RdsSync from the handle's bb while L and R of the same calls are the stereo handle's."""
import ctypes as C

import numpy as np
import pytest

from rds_ref import rds_ref, station_samples
from stereo_ref import stereo_ref
from test_rds_shapes_gpu import _bits, _device_d
from test_stereo_shapes_gpu import _ambiguous, _clean_outputs

pytestmark = pytest.mark.gpu

FS, D, DA, DR = 2.4e6, 10, 5, 25
TOL = 1e-5
EXCLUDED_CAP = 0.02                                             # of a stream's stereo outputs: asserted on the reference before comparing


def _setup(pkg, T=64):
    return dict(fir_coeffs=pkg.lowpass_taps(T, 120e3 / FS), pilot_coeffs=pkg.stereo_pilot_taps(101, FS / D),
                audio_coeffs=pkg.lowpass_taps(32, 15e3 / (FS / D)), rds_coeffs=pkg.rds_lowpass_taps(255, FS / D),
                diff_gain=pkg.stereo_diff_gain(D, FS), rds_gain=pkg.rds_gain(D, FS), pilot_min=0.05, fir_decim=D, audio_decim=DA, rds_decim=DR)


def _bcast(pkg, ns, nbytes, T=64, **kw):
    return pkg.BroadcastDemod(pkg.BroadcastConfig(n_streams=ns, max_bytes_per_call=nbytes, **dict(_setup(pkg, T), **kw)))


def _stereo(pkg, ns, nbytes, T=64):
    c = _setup(pkg, T)
    for k in ("rds_coeffs", "rds_gain", "rds_decim"):
        del c[k]
    return pkg.StereoDemod(pkg.StereoConfig(n_streams=ns, max_bytes_per_call=nbytes, **c))


def test_default_shape_against_the_written_definitions_on_stations(pkg, oracle_mod):
    """bb is the fp32-faithful RDS reference's w on the device's own d bit for bit (every stage behind d is a written fmaf, a product or a
    correctly rounded quotient); L and R are within 1e-5 scaled of the stereo reference's outside outputs whose window holds a d within
    1e-3 of the gate; the pilot count is both references'."""
    c = _setup(pkg)
    h, b, ga, gr = c["fir_coeffs"], c["pilot_coeffs"], c["audio_coeffs"], c["rds_coeffs"]
    ns, nsamp = 4, 600000
    sent = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "RDS on the GPU..")
    iq = np.stack([pkg.make_iq_rds(1, nsamp, sent, rds_phase=0.7 * s, clock_ppm=(0, 100, -100, 0)[s], first_id=60 + s)[0] for s in range(ns)])
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    with _bcast(pkg, ns, 2 * nsamp) as bc:
        name = bc.kernel_name
        L, R, bb, pc = bc.process_batch(iq)
    assert name == "bcast-fast T64 D10 P101 Ta32 Da5 Tr255 Dr25", name
    for s in range(ns):
        rr = rds_ref(ds[s], b, gr, 0.05, c["rds_gain"], DR)
        sr = stereo_ref(ds[s], b, ga, 0.05, c["diff_gain"], DA)
        assert rr["count"] == sr["count"]
        amb = _ambiguous(sr)
        keep = _clean_outputs(amb, sr["L"].size, 32, DA)
        excl = float((~keep).sum()) / keep.size
        print("stream %d: %d d's within 1e-3 of the gate, %d of %d stereo outputs excluded, pilot count %d of %d (reference %d)" % (
            s, int(amb.sum()), int((~keep).sum()), keep.size, int(pc[s]), ds[s].size, sr["count"]))
        assert excl <= EXCLUDED_CAP, (s, excl)
        assert int(pc[s]) == rr["count"], (s, int(pc[s]), rr["count"])
        assert bb[s].shape == rr["w"].shape and np.array_equal(_bits(bb[s]), _bits(rr["w"])), (s, float(np.abs(bb[s] - rr["w"]).max()))
        for got, ch in ((L[s], "L"), (R[s], "R")):
            assert got.shape == sr[ch].shape
            want = sr[ch][keep].astype(np.float64)
            err = float((np.abs(got[keep].astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)).max())
            print("stream %d %s: worst scaled error %.3g over %d outputs" % (s, ch, err, int(keep.sum())))
            assert err <= TOL, (s, ch, err)


def _call(pkg, bc, iq_ptr, iq_stride, nbytes, l_ptr, r_ptr, audio_stride, bb_ptr, bb_stride, pc_ptr, flags=None):
    """sdrfm_bcast_process_batch on raw device addresses (strides the tensor wrapper cannot express)"""
    na, nr = C.c_uint32(), C.c_uint32()
    rc = pkg.load_library().sdrfm_bcast_process_batch(bc._h, C.c_void_p(iq_ptr), int(iq_stride), int(nbytes), C.c_void_p(l_ptr), C.c_void_p(r_ptr),
                                                      int(audio_stride), C.c_void_p(bb_ptr), int(bb_stride), C.c_void_p(pc_ptr) if pc_ptr else None,
                                                      C.byref(na), C.byref(nr), pkg.lib.F_DEVICE_PTRS if flags is None else flags)
    return rc, na.value, nr.value


def _case(pkg, ns, nsamp):
    iq = np.stack([pkg.make_iq_rds(1, nsamp, pkg.rds_encode_groups(0x3000 + s, "FORMS %02d" % s), rds_phase=0.4 * s, first_id=3000 + s)[0] if s != 1 else
                   pkg.make_iq(1, nsamp, mode="random", first_id=3001)[0] for s in range(ns)])
    return iq


@pytest.mark.parametrize("T", [23, 64], ids=["generic", "fast"])
def test_call_forms_bitwise_host_buffers(pkg, T):
    import torch
    ns, nsamp = 3, 60011
    iq = _case(pkg, ns, nsamp)
    nbytes = 2 * nsamp
    cuts = [2 * 5003, 2 * 7, 0, 2 * 29001, 2]
    cuts.append(nbytes - sum(cuts))
    with _bcast(pkg, ns, nbytes, T) as bc:
        name = bc.kernel_name
        assert name.startswith("bcast-fast" if T == 64 else "bcast-generic"), name
        L1, R1, bb1, pc1 = bc.process_batch(iq)
        Aa, Ar = L1.shape[1], bb1.shape[1]
        ref_f = np.ascontiguousarray(bb1).view(np.float32)          # [ns, 2 Ar]
        # device rows at byte offsets 2, 6, 14, row strides that are not multiples of 16 (the kernel stages x element-wise), ragged calls
        for off, pad in ((2, 2), (6, 4), (14, 6)):
            stride = nbytes + pad
            assert stride % 16 and off % 16
            buf = torch.zeros(ns * stride + 64, dtype=torch.uint8, device="cuda")
            rows = buf[off:off + ns * stride].view(ns, stride)
            rows[:, :nbytes] = torch.from_numpy(iq).cuda()
            d_l = torch.full((ns, Aa + 5), -7.0, dtype=torch.float32, device="cuda")
            d_r = torch.full((ns, Aa + 5), -7.0, dtype=torch.float32, device="cuda")
            d_bb = torch.full((ns, 2 * Ar + 6), -7.0, dtype=torch.float32, device="cuda")
            d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            bc.reset()
            Ls, Rs, ws, pcs, pos = [], [], [], np.zeros(ns, np.int64), 0
            for c in cuts:
                na, nr = bc.process_batch_device(rows[:, pos:], d_l, d_r, d_bb, d_pc, nbytes=c)
                bc.synchronize()
                Ls.append(d_l[:, :na].cpu().numpy().copy()), Rs.append(d_r[:, :na].cpu().numpy().copy())
                ws.append(d_bb[:, :2 * nr].cpu().numpy().copy())
                pcs += d_pc.cpu().numpy().astype(np.int64)
                pos += c
            assert np.array_equal(_bits(np.concatenate(Ls, 1)), _bits(L1)) and np.array_equal(_bits(np.concatenate(Rs, 1)), _bits(R1)), (off, pad)
            assert np.array_equal(_bits(np.concatenate(ws, 1)), _bits(ref_f)), (off, pad)
            assert np.array_equal(pcs, pc1.astype(np.int64)), (off, pad)
        # audio_stride > n_audio and bb_stride > 2 n_rds: the rows' tails stay untouched; pilot_count = NULL; the caller's stream
        bc.reset()
        d_iq = torch.from_numpy(iq).cuda()
        wide_a, wide_r = Aa + 77, 2 * Ar + 77
        d_l = torch.full((ns, wide_a), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, wide_a), -7.0, dtype=torch.float32, device="cuda")
        d_bb = torch.full((ns, wide_r), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mine = torch.cuda.Stream()
        bc.set_stream(mine.cuda_stream)
        na, nr = bc.process_batch_device(d_iq, d_l, d_r, d_bb, None)
        mine.synchronize()
        bc.set_stream(None)
        assert (na, nr) == (Aa, Ar) and d_l.stride(0) == wide_a and d_bb.stride(0) == wide_r
        assert np.array_equal(_bits(d_l[:, :na].cpu().numpy()), _bits(L1)) and np.array_equal(_bits(d_r[:, :na].cpu().numpy()), _bits(R1))
        assert np.array_equal(_bits(d_bb[:, :2 * nr].cpu().numpy()), _bits(ref_f))
        assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_bb[:, 2 * nr:] == -7.0).all()
        # the refusals: SDRFM_F_OVERLAP, short output rows, too many bytes, an odd count; the state is left alone
        lib = pkg.lib
        args = (d_iq.data_ptr(), d_iq.stride(0), nbytes, d_l.data_ptr(), d_r.data_ptr(), wide_a, d_bb.data_ptr(), wide_r, 0)
        assert _call(pkg, bc, *args, flags=lib.F_DEVICE_PTRS | lib.F_OVERLAP)[0] == lib.EINVAL
        assert _call(pkg, bc, *args[:5], Aa - 1, *args[6:])[0] == lib.ECAPACITY
        assert _call(pkg, bc, *args[:7], 2 * Ar - 1, 0)[0] == lib.ECAPACITY
        assert _call(pkg, bc, args[0], args[1], nbytes + 2, *args[3:])[0] == lib.ECAPACITY
        assert _call(pkg, bc, args[0], args[1], nbytes - 1, *args[3:])[0] == lib.EODD
        assert _call(pkg, bc, args[0], nbytes - 2, *args[2:])[0] == lib.ECAPACITY
        with pytest.raises(pkg.SdrfmError) as e:
            bc.counts(nbytes - 1)
        assert e.value.status == lib.EODD
        bc.reset()
        L3, R3, bb3, pc3 = bc.process_batch(iq[:, :2 * 20000])
        na, nr = bc.counts(nbytes - 2 * 20000)
        assert _call(pkg, bc, *args[:5], na - 1, *args[6:])[0] == lib.ECAPACITY      # (refused in mid-stream: the phases stay)
        L4, R4, bb4, pc4 = bc.process_batch(iq[:, 2 * 20000:])
        for a, b_, one in ((L3, L4, L1), (R3, R4, R1), (bb3, bb4, bb1)):
            assert np.array_equal(_bits(np.concatenate([a, b_], 1)), _bits(one))
        assert np.array_equal(pc3.astype(np.int64) + pc4, pc1.astype(np.int64))
    # one stream, iq_stride < nbytes (a single row needs no stride), at an unaligned address
    with _bcast(pkg, 1, nbytes, T) as one:
        L0, R0, bb0, pc0 = one.process_batch(iq[2:3])
        assert np.array_equal(_bits(L0), _bits(L1[2:3])) and np.array_equal(_bits(R0), _bits(R1[2:3])) and np.array_equal(_bits(bb0), _bits(bb1[2:3]))
        assert pc0[0] == pc1[2]
        one.reset()
        buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        buf[6:6 + nbytes] = torch.from_numpy(iq[2]).cuda()
        d_l = torch.full((1, Aa + 3), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((1, Aa + 3), -7.0, dtype=torch.float32, device="cuda")
        d_bb = torch.full((1, 2 * Ar + 3), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc, na, nr = _call(pkg, one, buf.data_ptr() + 6, 2, nbytes, d_l.data_ptr(), d_r.data_ptr(), 0, d_bb.data_ptr(), 0, d_pc.data_ptr())
        one.synchronize()
        assert rc == pkg.lib.OK and (na, nr) == (Aa, Ar)
        assert np.array_equal(_bits(d_l[:, :na].cpu().numpy()), _bits(L0)) and np.array_equal(_bits(d_r[:, :na].cpu().numpy()), _bits(R0))
        assert np.array_equal(_bits(d_bb[:, :2 * nr].cpu().numpy()), _bits(np.ascontiguousarray(bb0).view(np.float32)))
        assert int(d_pc[0]) == int(pc0[0]) and (d_l[:, na:] == -7.0).all() and (d_bb[:, 2 * nr:] == -7.0).all()
    print("%s: unaligned rows at offsets 2 / 6 / 14, wide audio and bb rows, no pilot count, the caller's stream, one short-stride stream: "
          "bitwise the host-buffer calls; SDRFM_F_OVERLAP, short rows, too many and odd bytes refused, the state left alone" % name)


def test_receiver_end_to_end_three_stations(pkg):
    """three stations (own PI, PS, radio text, subcarrier phase, crystal offset) in four calls: the PS name and the radio text come back
    through RdsSync from the handle's bb, and L and R of the same calls are the stereo handle's bit for bit"""
    ns, n_calls, call_samples = 3, 4, 380000
    nsamp = n_calls * call_samples
    sent = [pkg.rds_encode_groups(0x4000 + k, "BCAST %02d" % k, "tx%d" % k) for k in range(ns)]
    assert len(sent[0]) == 5 and station_samples(7) <= nsamp        # a cycle of five groups; seven leave two for the decoder to lock
    iq = np.stack([pkg.make_iq_rds(1, nsamp, sent[k], rds_phase=0.8 * k, clock_ppm=(0.0, 100.0, -100.0)[k], first_id=800 + k)[0] for k in range(ns)])
    syncs = [pkg.RdsSync(FS / D / DR) for _ in range(ns)]
    heard = [[] for _ in range(ns)]
    with _bcast(pkg, ns, 2 * call_samples) as bc, _stereo(pkg, ns, 2 * call_samples) as st:
        name = bc.kernel_name
        for c in range(n_calls):
            part = iq[:, 2 * c * call_samples:2 * (c + 1) * call_samples]
            L, R, bb, pc = bc.process_batch(part)
            Ls, Rs, pcs = st.process_batch(part)
            assert np.array_equal(_bits(L), _bits(Ls)) and np.array_equal(_bits(R), _bits(Rs)) and np.array_equal(pc, pcs), c
            for k in range(ns):
                heard[k] += syncs[k].push(bb[k])
    assert name.startswith("bcast-fast"), name
    for k in range(ns):
        info = pkg.rds_parse(heard[k])
        assert info["pi"] == 0x4000 + k and info["ps"] == "BCAST %02d" % k and info["text"] == "tx%d" % k, (k, info)
        syncs[k].close()
    print("%s: %d stations' PS names and radio texts read back over %d calls (%d groups each), L and R bitwise the stereo handle's" % (
        name, ns, n_calls, len(heard[0])))
