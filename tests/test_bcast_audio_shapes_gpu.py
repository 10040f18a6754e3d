"""GPU sweep of the conditioned broadcast kernels (sdrfm_bcast_set_audio) over every shape of tests/pilot_shape_cases.py, on
the generic kernels and on the fast ones where the handle claims them, with the ramps of tests/audio_shape_cases.py: every stream from a
start of its own to targets of its own, still moving deep inside the case's long call.

  1. tuned, the whole row in one call, against tests/audio_ref.py's blend of the reference's am and as_ at the bound of
     tests/test_bcast_tuned_gpu.py (|beta|, |mu| <= 1: a blended output is at most a plain one's error off, plus three roundings of values
     below 2 pi); the same outputs against the ramps one output further along and against the streams' records rotated by one must miss
     that bound in every stream that carries audio — tests/test_audio_shapes_cpu.py shows from the references alone that they can.
  2. the identities of §4.16, exact and on the device alone, tuned and untuned: blend 0 is a handle made with diff_gain = 0, blend 1/4 at
     gain 1/8 one made with diff_gain / 4 times 0.125, a gain ramp at blend 0 is mu_j am.
  3. the case's ragged cuts as plain calls, as metered calls and in turn, tuned and untuned, both ramps running: the one blended call's
     bits, the records an unconditioned handle's, audio_state() the reference's after every call.  This is where the four metered blended
     instantiations of k_bcast run with ramps that move, at their own split.  The one blended call itself is held, untuned as well, to
     mu_j (am +- beta_j as) under the reference's b and v at §4.16's derived tolerance, am a diff_gain = 0 handle's L and as = (L - R) / 2
     of the unconditioned handle: every call form's outputs so depend on the count, on the stream's record and on the output index.
  4. the metered call on unaligned device rows between canaries, the ramps running.
Audio is compared as values where a product with mu or beta = 0 is involved (the sign of a zero), bb, pilot_count and records as integers."""
import ctypes as C

import numpy as np
import pytest

import audio_ref as ar
import audio_shape_cases as asc
import pilot_shape_cases as ps
import tuned_cases as tc
from test_bcast_audio_gpu import _set
from test_bcast_tuned_gpu import TOL, _check_case, _same
from test_bcast_tuned_shapes_gpu import FORMS, SHAPE_IDS, _bcast, _forms, _mid, _outputs_equal
from test_scan_shapes_gpu import _records_equal

pytestmark = pytest.mark.gpu

ONE = ar.ONE


def _scaled(case, scale):
    """the case's taps with diff_gain times a power of two or 0 (exact in fp32)"""
    h, ga, gr, b, dg, rg = case["taps"]
    return h, ga, gr, b, float(np.float32(dg) * np.float32(scale)), rg


def _tune(bc, case, tuned):
    if tuned:
        bc.tune(ctaps=case["ctaps"], rot=case["rot"])


def _condition(bc, b0, v0, bt, vt, slew):
    """whatever the handle's conditioning was: the streams put at (b0, v0) by a jump that a reset completes (the streams start again), then
    sent to (bt, vt) at the slew, all through the C call; returns the audio_ref.AudioState that went along"""
    bc.clear_audio()
    ref = ar.AudioState(bc.cfg.n_streams)
    ref.check(bc.audio_state())
    _set(b0, v0, ONE, ref)(bc)
    bc.reset()
    ref.complete()
    ref.check(bc.audio_state())
    _set(bt, vt, slew, ref)(bc)
    return ref


def _case_ramps(bc, rm):
    return _condition(bc, rm["b0"], rm["v0"], rm["bt"], rm["vt"], rm["slew"])


def _gate(case, tuned):
    """the threshold of the comparisons that are exact on the device alone: in the middle of the rows' pilot powers"""
    return _mid(case) if tuned else ps.offset_zero_gate(case, case["taps"][3])


def _stream_errors(got, L, R, keep_a):
    """per stream: the worst |error| of L and R on the kept outputs"""
    out = []
    for s in range(L.shape[0]):
        e = np.maximum(np.abs(got[0][s].astype(np.float64) - L[s]), np.abs(got[1][s].astype(np.float64) - R[s]))[keep_a[s]]
        out.append(float(e.max()) if e.size else 0.0)
    return out


# ---- 1. against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_both_ramps_moving_against_the_reference(pkg, shape):
    ac = asc.audio_case(pkg, shape)
    case, rm = ac["case"], ac["ramps"]
    frac, keep_a, keep_r, n_amb = tc.case_keeps(case, case["refs"])
    silent = asc.silent_streams(ac, keep_a)
    for generic in _forms(shape):
        with _bcast(pkg, case, case["pilot_min"], generic) as bc:
            bc.tune(ctaps=case["ctaps"], rot=case["rot"])
            ref = _case_ramps(bc, rm)
            name = bc.kernel_name
            assert name == ps.bcast_name(shape, True, generic) + " blend", name
            got = bc.process_batch(case["iq"])
            b, v = ref.call(got[0].shape[1])
            ref.check(bc.audio_state())
        assert np.array_equal(b, rm["b"]) and np.array_equal(v, rm["v"])
        # L and R against the blended rows, bb and pilot_count as the unconditioned sweep compares them
        worst, frac = _check_case(case, asc.refs_blended(ac, ac["L"], ac["R"]), got, name)
        assert worst <= TOL
        right = _stream_errors(got, ac["L"], ac["R"], keep_a)
        print("%s: slew %d, pilot counts %s: worst |error| %.3g (L, R alone %.3g), %.3f %% of the outputs excluded" % (
            name, rm["slew"], [int(c) for c in got[3]], worst, max(right), 100 * frac))
        assert max(right) <= TOL
        for what in asc.WRONG:
            if what == asc.WRONG[1] and rm["ns"] == 1:
                continue                                             # one stream: its record rotates onto itself
            wrong = _stream_errors(got, ac["wrong"][what][0], ac["wrong"][what][1], keep_a)
            print("%s against %s: worst |error| per stream %s%s" % (name, what, ["%.3g" % e for e in wrong],
                                                                    ", silent %s" % silent if silent else ""))
            for s, e in enumerate(wrong):
                assert s in silent or e > TOL, (name, what, s, case["names"][s], e)
            with pytest.raises(AssertionError):
                _check_case(case, asc.refs_blended(ac, *ac["wrong"][what]), got, name)


# ---- 2. the identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_identities_are_exact_at_every_geometry(pkg, shape):
    case, rm = ps.bcast_case(pkg, shape), asc.case_ramps(shape)
    ns, iq = case["ns"], case["iq"]
    for generic in _forms(shape):
        for tuned in (False, True):
            pm = _gate(case, tuned)
            with _bcast(pkg, case, pm, generic) as bc, _bcast(pkg, case, pm, generic, taps=_scaled(case, 0.0)) as mono, \
                    _bcast(pkg, case, pm, generic, taps=_scaled(case, 0.25)) as quarter:
                for h_ in (bc, mono, quarter):
                    _tune(h_, case, tuned)
                plain = ps.bcast_name(shape, tuned, generic)
                want0, want4 = mono.process_batch(iq), quarter.process_batch(iq)
                assert mono.kernel_name == quarter.kernel_name == plain
                where = (plain, "tuned" if tuned else "untuned")
                # blend 0 by a jump
                _set(0, None, ONE)(bc)
                assert bc.kernel_name == plain + " blend", bc.kernel_name
                got = bc.process_batch(iq)
                for x, y, what in zip(got[:2], want0[:2], "LR"):
                    assert x.shape == y.shape and not np.isnan(x).any() and np.array_equal(x, y), (where, "blend 0", what)
                _outputs_equal((want0[0], want0[1]) + got[2:], want0, where)
                assert np.array_equal(got[0], got[1])
                # blend 2^-2 at gain 2^-3
                _condition(bc, ONE // 4, ONE // 8, ONE // 4, ONE // 8, ONE)
                got = bc.process_batch(iq)
                eighth = np.float32(0.125)
                assert np.array_equal(got[0], want4[0] * eighth) and np.array_equal(got[1], want4[1] * eighth), (where, "blend 1/4 at gain 1/8")
                _outputs_equal((want4[0], want4[1]) + got[2:], want4, where)
                # a gain ramp at blend 0: the case's own gains and slew
                ref = _condition(bc, 0, rm["v0"], 0, rm["vt"], rm["slew"])
                got = bc.process_batch(iq)
                b, v = ref.call(got[0].shape[1])
                ref.check(bc.audio_state())
                assert not b.any() and np.array_equal(v, rm["v"])
                mu = (v.astype(np.float64) / ONE).astype(np.float32)
                assert np.array_equal(got[0], mu * want0[0]) and np.array_equal(got[1], mu * want0[0]), (where, "gain ramp at blend 0")
                _outputs_equal((want0[0], want0[1]) + got[2:], want0, where)
                name = bc.kernel_name
            M = iq.shape[1] // 2 // shape[1]
            assert any(0 < int(c) < M for c in want0[3]), ("the gate is not both on and off in any stream", list(want0[3]), M)
            print("%s, %s: blend 0, blend 1/4 at gain 1/8 and the gain ramp at blend 0 exact over %d outputs a stream; pilot counts %s" % (
                name, where[1], got[0].shape[1], [int(c) for c in want0[3]]))


# ---- 3. the ragged sequence ----------------------------------------------------------------------------------------------------------
def _within_the_derived_tolerance(got, am, plain, b, v, where):
    """L and R of a blended call against mu (am +- beta as) in float64, am the diff_gain = 0 handle's L and as = (L - R) / 2 of the plain
    handle's rows.  Tolerance per output 4 * 2^-23 (|am| + |as|), as tests/test_bcast_audio_gpu.py derives it whatever the shape: as so
    estimated is within 2^-23 of that sum, and the formula's three roundings add at most 2^-24 of it each.  Returns the worst ratio."""
    am, as_ = am.astype(np.float64), (plain[0].astype(np.float64) - plain[1].astype(np.float64)) / 2
    tol = 4 * 2.0 ** -23 * (np.abs(am) + np.abs(as_))
    beta, mu = b / ONE, v / ONE
    el, er = np.abs(got[0] - mu * (am + beta * as_)), np.abs(got[1] - mu * (am - beta * as_))
    assert (el <= tol).all() and (er <= tol).all(), (where, int((el > tol).sum()), int((er > tol).sum()), np.argwhere((el > tol) | (er > tol))[:4])
    return float((np.maximum(el, er) / np.maximum(tol, 1e-30)).max())


def _sequence(bc, iq, cuts, metered, ref):
    """tests/test_bcast_tuned_shapes_gpu.py's _sequence with the reference moved along: after every call, the 0-byte and 2-byte ones
    included, audio_state() is the reference's.  Returns (L, R, bb, summed pilot counts, the metered calls' records by call index, b, v)"""
    parts, pct, pos, recs, bs, vs = ([], [], []), 0, 0, {}, [], []
    for k, c in enumerate(cuts):
        want = bc.counts(c)
        out = bc.process_batch_metered(iq[:, pos:pos + c]) if metered(k) else bc.process_batch(iq[:, pos:pos + c])
        assert (out[0].shape[1], out[1].shape[1], out[2].shape[1]) == (want[0], want[0], want[1]), (c, out[0].shape, out[2].shape, want)
        if metered(k):
            m = out[4]
            assert (m["reserved"] == 0).all() and (m["n"] == m["n"][0]).all() and np.array_equal(m["n_pilot"], out[3].astype(np.uint64)), (c, m, out[3])
            recs[k] = m
        for acc, x in zip(parts, out[:3]):
            acc.append(x)
        pct = pct + out[3].astype(np.int64)
        pos += c
        b, v = ref.call(out[0].shape[1])
        bs.append(b)
        vs.append(v)
        ref.check(bc.audio_state())
    assert pos == iq.shape[1]
    return tuple(np.concatenate(p, 1) for p in parts) + (pct, recs, np.concatenate(bs, 1), np.concatenate(vs, 1))


@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=SHAPE_IDS)
def test_ragged_plain_metered_and_alternating_calls_with_the_ramps_running(pkg, shape):
    case, rm = ps.bcast_case(pkg, shape), asc.case_ramps(shape)
    ns, iq, cuts = case["ns"], case["iq"], case["cuts"]
    assert cuts == rm["cuts"] and 0 in cuts and 2 in cuts
    for generic in _forms(shape):
        for tuned in (False, True):
            pm = _gate(case, tuned)
            with _bcast(pkg, case, pm, generic) as bc, _bcast(pkg, case, pm, generic) as plain, _bcast(pkg, case, pm, generic, taps=_scaled(case, 0.0)) as mono:
                for h_ in (bc, plain, mono):
                    _tune(h_, case, tuned)
                unconditioned = plain.process_batch_metered(iq)      # an unconditioned handle's one metered call
                records = unconditioned[4]
                name = ps.bcast_name(shape, tuned, generic) + " blend"
                ref = _case_ramps(bc, rm)
                one = bc.process_batch(iq)
                ref.call(one[0].shape[1])
                ref.check(bc.audio_state())
                assert bc.kernel_name == name and plain.kernel_name + " blend" == name
                ratio = _within_the_derived_tolerance(one, mono.process_batch(iq)[0], unconditioned, rm["b"], rm["v"], name)
                seqs = {}
                for what, metered in (("plain", lambda k: False), ("metered", lambda k: True), ("in turn", lambda k: k % 2 == 0)):
                    ref = _case_ramps(bc, rm)                        # (its reset starts the streams again)
                    seqs[what] = _sequence(bc, iq, cuts, metered, ref)
                    assert bc.kernel_name == name
                    _outputs_equal(seqs[what], one, "%s, %s calls" % (name, what))
                    assert np.array_equal(seqs[what][5], rm["b"]) and np.array_equal(seqs[what][6], rm["v"])
                acc = np.zeros(ns, pkg.METER_DTYPE)
                for m in seqs["metered"][4].values():
                    pkg.meter_add(acc, m)
                _records_equal(acc, records, name + ", the metered cuts summed against an unconditioned handle's one metered call")
                for k, m in seqs["in turn"][4].items():
                    _records_equal(m, seqs["metered"][4][k], "%s, call %d of the calls in turn" % (name, k))
            print("%s: %d calls (the long one %d audio outputs) plain, metered and in turn bitwise the one blended call, that one at %.3f of "
                  "the derived tolerance; the records an unconditioned handle's; audio_state the reference's after every call" % (
                      name, len(cuts), rm["a1"] - rm["a0"], ratio))


# ---- 4. the metered call on unaligned device rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORMS, ids=[ps.bcast_id(s) for s in FORMS])
def test_metered_device_call_forms_with_the_ramps_running(pkg, shape):
    """tests/test_bcast_tuned_shapes_gpu.py's layouts — device rows at byte offsets 2 / 6 / 14 with strides that are no multiple of 16, output
    rows with odd strides between canaries, the records 8 bytes into their allocation between canary records, the caller's stream at the
    last — on a conditioned handle: the host-buffer call's bits"""
    import torch
    case, rm = ps.bcast_case(pkg, shape), asc.case_ramps(shape)
    ns, iq, pm = case["ns"], case["iq"], _mid(case)
    nbytes = iq.shape[1]
    lib, DEV = pkg.load_library(), pkg.lib.F_DEVICE_PTRS
    generic = shape[:3] != (64, 10, 101)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert ns > 1
    with _bcast(pkg, case, pm, generic) as bc:
        bc.tune(ctaps=case["ctaps"], rot=case["rot"])
        _case_ramps(bc, rm)
        want = bc.process_batch_metered(iq)
        assert bc.kernel_name == ps.bcast_name(shape, True, generic) + " blend"
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
            ref = _case_ramps(bc, rm)
            if k == 2:
                bc.set_stream(stream.cuda_stream)
            n1, n2 = C.c_uint32(), C.c_uint32()
            rc = lib.sdrfm_bcast_process_batch_metered(bc._h, None, ptr(buf, off), stride, nbytes, ptr(d_l), ptr(d_r), d_l.stride(0), None, 0, ptr(d_w),
                                                       d_w.stride(0), ptr(d_pc), ptr(words, 64 + 8), C.byref(n1), C.byref(n2), DEV)
            assert rc == pkg.lib.OK and (n1.value, n2.value) == (na, nr), (rc, n1.value, n2.value, na, nr)
            bc.synchronize()
            stream.synchronize()
            ref.call(na)
            ref.check(bc.audio_state())
            where = "device rows at byte %d, stride %d" % (off, stride)
            host = words.cpu().numpy()
            assert (host[:9] == -7).all() and (host[9 + 8 * ns:] == -7).all(), (where, host[:9], host[9 + 8 * ns:])
            _records_equal(np.ascontiguousarray(host[9:9 + 8 * ns]).view(pkg.METER_DTYPE).reshape(ns), want[4], where)
            got = (d_l[:, :na].cpu().numpy(), d_r[:, :na].cpu().numpy(), np.ascontiguousarray(d_w[:, :2 * nr].cpu().numpy()).view(np.complex64),
                   d_pc.cpu().numpy())
            _outputs_equal(got, want, where)
            assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all(), where
            assert (buf[:off] == 0xA5).all() and (buf[off + (ns - 1) * stride + nbytes:] == 0xA5).all(), where
        bc.reset()
        bc.set_stream(None)
    assert len(np.unique(rm["b"][0])) > 100 and not _same(want[0][0:1], want[0][1:2])
