"""GPU tests of the tuned broadcast handle (sdrfm_bcast_tune): the identities that tie the tuned kernels to the untuned
ones bit for bit (offset 0; offset fs / 2 at an even D), the tuned kernels against tests/tuned_ref.py at per-stream offsets that differ
(the cases of tests/tuned_cases.py, whose outputs at the pilot gate tests/test_tuned_ref.py counts without a device), any cut of a capture
into calls, one shared input row against replicated rows, tune / reset / un-tune, the refusals, the PCM one-call form, and three stations
received from one capture by one 3-stream handle.  Every test runs the fast kernel and the generic one."""
import ctypes as C

import numpy as np
import pytest

import tuned_cases as tc
import tuned_ref as tr
from stereo_ref import separation_db

pytestmark = pytest.mark.gpu

TOL = 1e-5                                                      # absolute, on L, R (radians) and bb: the project's parity bound
KERNELS = [(name, generic) for name in tc.SHAPES for generic in ((False, True) if name == "default" else (True,))]
KERNEL_IDS = ["%s-%s" % (n, "generic" if g else "fast") for n, g in KERNELS]
CLASSES = ("station", "carrier", "random", "const")
EVEN_D = [k for k in KERNELS if tc.SHAPES[k[0]][1] % 2 == 0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _handle(pkg, shape, ns, pilot_min=0.05, nbytes=tc.NBYTES, generic=False):
    T, D, P, Ta, Da, Tr, Dr = shape
    h, ga, gr, b, dg, rg = tc.shape_taps(pkg, shape)
    return pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b, pilot_min=float(pilot_min), diff_gain=dg,
                                                  rds_gain=rg, fir_decim=D, audio_decim=Da, rds_decim=Dr, n_streams=ns, max_bytes_per_call=nbytes,
                                                  force_generic=generic))


def _want_name(shape, generic, tuned):
    T, D, P, Ta, Da, Tr, Dr = shape
    kind = "generic" if generic or (T, D, P) != (64, 10, 101) else "fast"
    dims = "T%d D%d P%d Ta%d Da%d Tr%d Dr%d" % shape
    return "bcast-%s%s %s" % (kind, "-tuned" if tuned else "", dims)


_untuned = {}


def _untuned_inputs(pkg, shape, ns):
    """ns rows at 0 Hz, the classes in turn (a carrier is the FM generator's), made once per (rate, stream)"""
    fs = tc.fs_of(shape[1])
    rows = []
    for s in range(ns):
        key = (fs, s)
        if key not in _untuned:
            cls = CLASSES[s % 4]
            if cls == "station":
                row = pkg.make_iq_rds(1, tc.NBYTES // 2, tc.GROUPS, fs=fs, rds_phase=0.4 * s, first_id=6000 + s)[0]
            else:
                row = pkg.make_iq(1, tc.NBYTES // 2, mode="fm" if cls == "carrier" else cls, fs=fs, first_id=6000 + s)[0]
            row.setflags(write=False)
            _untuned[key] = row
        rows.append(_untuned[key])
    return np.stack(rows)


def _ragged(shape, nbytes, seed):
    """even byte counts that sum to nbytes, the ragged sequence of tests/test_bcast_shapes_gpu.py: 0, 2, one short of an audio output, one
    short of an RDS output, one whose M is below H / 2, a second 0, then random ones"""
    T, D, P, Ta, Da, Tr, Dr = shape
    H = P - 1 + max(Ta, Tr) - 1
    cuts = [0, 2]
    if D * Da > 2:
        cuts.append(2 * D * Da - 4)
    if D * Dr > 2:
        cuts.append(2 * D * Dr - 4)
    if H >= 4:
        cuts.append(2 * D * (H // 2) - 2)
    cuts.append(0)
    rest = nbytes - sum(cuts)
    rng = np.random.default_rng(seed)
    marks = np.sort(2 * rng.integers(1, rest // 2, 4))
    cuts += [int(v) for v in np.diff(np.concatenate([[0], marks, [rest]]))]
    assert sum(cuts) == nbytes and all(c >= 0 and c % 2 == 0 for c in cuts)
    return cuts


def _in_calls(bc, iq, cuts):
    """the calls one after the other, counts() before each; returns (L, R, bb, summed pilot counts)"""
    parts, pct, pos = ([], [], []), 0, 0
    for c in cuts:
        want = bc.counts(c)
        l, r, w, pc = bc.process_batch(iq[:, pos:pos + c])
        assert (l.shape[1], r.shape[1], w.shape[1]) == (want[0], want[0], want[1]), (c, l.shape, w.shape, want)
        for acc, v in zip(parts, (l, r, w)):
            acc.append(v)
        pct = pct + pc.astype(np.int64)
        pos += c
    assert pos == iq.shape[1]
    return tuple(np.concatenate(p, 1) for p in parts) + (pct,)


# ---- 1. offset 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_zero_offset_is_the_untuned_handle_bitwise(pkg, name, generic):
    """taps (h, 0) and rot 0: B is a chain of +0's, y = (Ar - 0, Ai + 0) and v = atan2 - 0 never wraps; L, R, bb and pilot_count are the
    untuned handle's in one call and over the ragged sequence"""
    shape = tc.SHAPES[name]
    ns = (3, 7, 1)[list(tc.SHAPES).index(name) % 3] if generic else 7
    iq = _untuned_inputs(pkg, shape, ns)
    h = tc.shape_taps(pkg, shape)[0]
    cuts = _ragged(shape, tc.NBYTES, 11)
    with _handle(pkg, shape, ns, generic=generic) as bc:
        assert bc.kernel_name == _want_name(shape, generic, False)
        one_u = bc.process_batch(iq)
        bc.reset()
        seq_u = _in_calls(bc, iq, cuts)
        bc.tune(ctaps=np.tile(tr.pairs(h), (ns, 1)), rot=np.zeros(ns, np.float32))
        assert bc.kernel_name == _want_name(shape, generic, True), bc.kernel_name
        one_t = bc.process_batch(iq)
        bc.reset()
        seq_t = _in_calls(bc, iq, cuts)
    assert tc.NBYTES // 2 // shape[1] >= 3 * 1023 and 0 < int(one_u[3].max())   # three workgroups a stream at the least; the gate opens
    for u, t, what in zip(one_u[:3] + seq_u[:3], one_t[:3] + seq_t[:3], ("L", "R", "bb", "L seq", "R seq", "bb seq")):
        assert _same(u, t), (name, what)
    assert np.array_equal(one_u[3], one_t[3]) and np.array_equal(seq_u[3], seq_t[3]) and np.array_equal(seq_t[3], one_t[3].astype(np.int64))
    for a, b_ in zip(one_t[:3], seq_t[:3]):
        assert _same(a, b_)


def test_tuned_fast_is_tuned_generic_bitwise(pkg):
    su, _ = tc.case_reference(pkg, tc.CASES[1])                     # default shape, 7 streams, the five offsets
    outs = []
    for generic in (False, True):
        with _handle(pkg, su["shape"], su["ns"], generic=generic) as bc:
            bc.tune(ctaps=su["ctaps"], rot=su["rot"])
            assert bc.kernel_name == _want_name(su["shape"], generic, True)
            outs.append(bc.process_batch(su["iq"]))
    for f, g in zip(outs[0][:3], outs[1][:3]):
        assert _same(f, g)
    assert np.array_equal(outs[0][3], outs[1][3])


# ---- 2. offset fs / 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", EVEN_D, ids=["%s-%s" % (n, "generic" if g else "fast") for n, g in EVEN_D])
def test_half_rate_is_the_untuned_handle_bitwise(pkg, name, generic):
    """taps (-1)^k h[k], rot 0, an even D, on bytes with every odd-indexed sample replaced by 255 - byte: the untuned handle's bits on the
    original bytes, all four input classes"""
    shape = tc.SHAPES[name]
    T, ns = shape[0], 4
    iq = _untuned_inputs(pkg, shape, ns)
    flipped = iq.copy().reshape(ns, -1, 2)
    flipped[:, 1::2] = 255 - flipped[:, 1::2]
    flipped = flipped.reshape(ns, -1)
    h = tc.shape_taps(pkg, shape)[0]
    sign = np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    with _handle(pkg, shape, ns, generic=generic) as bc:
        want = bc.process_batch(iq)
        bc.tune(ctaps=np.tile(tr.pairs(h * sign), (ns, 1)), rot=np.zeros(ns, np.float32))
        got = bc.process_batch(flipped)
    for w, g, what in zip(want[:3], got[:3], "LRw"):
        assert _same(w, g), (name, what)
    assert np.array_equal(want[3], got[3])


# ---- 3. per-stream offsets against the reference ----------------------------------------------------------------------------------
def _check_case(su, refs, got, where):
    frac, keep_a, keep_r, n_amb = tc.case_keeps(su, refs)
    assert frac <= tc.EXCLUDED_CAP, frac
    L, R, bb, pc = got
    worst = 0.0
    for s, r in enumerate(refs):
        assert L[s].shape == r["L"].shape and bb[s].shape == r["bb"].shape, (where, s, L[s].shape, r["L"].shape, bb[s].shape, r["bb"].shape)
        amb = tr.ambiguous(r["rds"])
        lo = int((r["rds"]["on"] & ~amb).sum())
        assert lo <= int(pc[s]) <= lo + n_amb[s], (where, s, int(pc[s]), lo, n_amb[s])
        for g, w, keep, what in ((L[s], r["L"], keep_a[s], "L"), (R[s], r["R"], keep_a[s], "R"), (bb[s].real, r["bb"].real, keep_r[s], "wr"),
                                 (bb[s].imag, r["bb"].imag, keep_r[s], "wi")):
            err = np.abs(g[keep].astype(np.float64) - w[keep].astype(np.float64))
            if err.size:
                e = float(err.max())
                worst = max(worst, e)
                assert e <= TOL, (where, s, su["names"][s], su["cycles"][s], what, e, int(np.flatnonzero(keep)[np.argmax(err)]))
    return worst, frac


@pytest.mark.parametrize("case", tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_offsets_that_differ_against_the_reference(pkg, case):
    su, refs = tc.case_reference(pkg, case)
    for generic in ((False, True) if case[0] == "default" else (True,)):
        with _handle(pkg, su["shape"], su["ns"], su["pilot_min"], generic=generic) as bc:
            bc.tune(ctaps=su["ctaps"], rot=su["rot"])
            name = bc.kernel_name
            assert name == _want_name(su["shape"], generic, True), name
            got = bc.process_batch(su["iq"])
        worst, frac = _check_case(su, refs, got, name)
        print("%s: %s at %s cycles / sample, pilot counts %s: worst |error| %.3g, %.3f %% of the outputs excluded" % (
            name, "/".join(su["names"]), su["cycles"], list(got[3]), worst, 100 * frac))


# ---- 4. any cut into calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [tc.CASES[0], tc.CASES[3], tc.CASES[7]], ids=[tc.case_id(tc.CASES[i]) for i in (0, 3, 7)])
def test_any_cut_into_calls_gives_the_one_call_bits(pkg, case):
    su = tc.case_setup(pkg, case)
    for generic in ((False, True) if case[0] == "default" else (True,)):
        with _handle(pkg, su["shape"], su["ns"], su["pilot_min"], generic=generic) as bc:
            bc.tune(ctaps=su["ctaps"], rot=su["rot"])
            one = bc.process_batch(su["iq"])
            for seed in (21, 22):
                bc.reset()
                seq = _in_calls(bc, su["iq"], _ragged(su["shape"], tc.NBYTES, seed))
                for a, b_, what in zip(one[:3], seq[:3], "LRw"):
                    assert _same(a, b_), (bc.kernel_name, seed, what)
                assert np.array_equal(one[3].astype(np.int64), seq[3]), (one[3], seq[3])


# ---- 5. one shared row -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_shared_input_is_replicated_rows_bitwise(pkg, generic):
    import torch
    shape, ns, nbytes = tc.SHAPES["default"], 3, tc.NBYTES
    row = tc.three_stations(pkg)[0][:, :nbytes]
    h = tc.shape_taps(pkg, shape)[0]
    offs = [st["offset_hz"] for st in tc.STATIONS]
    ctaps = np.stack([pkg.tuned_channel_taps(h, f, 2.4e6) for f in offs])
    rot = np.array([pkg.tuned_rotation(f, 2.4e6, 10) for f in offs], np.float32)
    cuts = [2 * 20001, 0, 2 * 7, nbytes - 2 * 20008]
    with _handle(pkg, shape, ns, generic=generic) as bc:
        bc.tune(ctaps=ctaps, rot=rot)
        want = _in_calls(bc, np.repeat(row, ns, 0), cuts)
        bc.tune(ctaps=ctaps, rot=rot, shared_input=True)
        assert bc.kernel_name == _want_name(shape, generic, True)
        got = _in_calls(bc, row, cuts)
        for a, b_, what in zip(want[:3], got[:3], "LRw"):
            assert _same(a, b_), ("host buffers", what)
        assert np.array_equal(want[3], got[3])
        assert not _same(got[0][0:1], got[0][1:2])                  # (the streams do receive different stations)
        # device buffers: one row between canaries, an iq_stride that would run off it if it were used; output rows padded by canaries
        na, nr = want[0].shape[1], want[2].shape[1]
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[32:32 + nbytes] = torch.from_numpy(row[0].copy()).cuda()
        d_l = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bc.reset()
        n1, n2 = C.c_uint32(), C.c_uint32()
        pos, oa, ow, pct = 0, 0, 0, np.zeros(ns, np.int64)
        for c in cuts:
            ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
            rc = pkg.load_library().sdrfm_bcast_process_batch(bc._h, ptr(buf, 32 + pos), 1 << 40, c, ptr(d_l, 4 * oa), ptr(d_r, 4 * oa), d_l.stride(0),
                                                              ptr(d_w, 4 * ow), d_w.stride(0), ptr(d_pc), C.byref(n1), C.byref(n2), pkg.lib.F_DEVICE_PTRS)
            assert rc == pkg.lib.OK, rc
            bc.synchronize()
            pct += d_pc.cpu().numpy().astype(np.int64)
            pos, oa, ow = pos + c, oa + n1.value, ow + 2 * n2.value
        assert (oa, ow) == (na, 2 * nr)
        assert _same(d_l[:, :na].cpu().numpy(), want[0]) and _same(d_r[:, :na].cpu().numpy(), want[1])
        assert _same(d_w[:, :2 * nr].cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32))
        assert np.array_equal(pct, want[3])
        assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all()
        assert (buf[:32] == 0xA5).all() and (buf[32 + nbytes:] == 0xA5).all()


# ---- 6. tune, reset, un-tune -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_tune_resets_reset_keeps_the_tuning_and_null_restores(pkg, generic):
    su = tc.case_setup(pkg, tc.CASES[0])
    shape, iq, half = su["shape"], su["iq"], 2 * 30001
    with _handle(pkg, shape, su["ns"], generic=generic) as bc:
        plain = bc.process_batch(iq[:, :half])
        plain_name = bc.kernel_name
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        first = bc.process_batch(iq[:, :half])
        assert not _same(first[0], plain[0])
        bc.process_batch(iq[:, half:])
        bc.reset()                                                   # keeps the tuning
        assert bc.kernel_name == _want_name(shape, generic, True)
        again = bc.process_batch(iq[:, :half])
        bc.process_batch(iq[:, half:half + 2 * 777])                 # (state to be dropped)
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])                    # a re-tune is a restart
        assert bc.counts(half) == (first[0].shape[1], first[2].shape[1])
        third = bc.process_batch(iq[:, :half])
        for a, b_, c_ in zip(first[:3], again[:3], third[:3]):
            assert _same(a, b_) and _same(a, c_)
        bc.process_batch(iq[:, half:half + 2 * 333])
        bc.tune()                                                    # back to the untuned kernels, from a zeroed state
        assert bc.kernel_name == plain_name == _want_name(shape, generic, False)
        back = bc.process_batch(iq[:, :half])
        for a, b_ in zip(plain[:3], back[:3]):
            assert _same(a, b_)
        assert np.array_equal(plain[3], back[3])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_next_call_unchanged(pkg):
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, T = su["ns"], su["shape"][0]
    lib = pkg.load_library()
    good_t, good_r = np.ascontiguousarray(su["ctaps"], np.float32), np.ascontiguousarray(su["rot"], np.float32)

    def with_(a, idx, v):
        a = a.copy().reshape(-1)
        a[idx] = v
        return a

    over = np.nextafter(tr.PI_F, np.float32(4))
    zeros_t, zeros_r = np.zeros_like(good_t), np.zeros_like(good_r)
    bad = [(with_(good_t, ns * 2 * T - 1, np.nan), zeros_r, 0), (with_(good_t, 0, np.inf), zeros_r, 0), (zeros_t, with_(good_r, ns - 1, np.nan), 0),
           (zeros_t, with_(good_r, 0, -np.inf), 0), (zeros_t, with_(good_r, 1, over), 0), (zeros_t, with_(good_r, 1, -over), 0),
           (zeros_t, zeros_r, 2), (zeros_t, zeros_r, 0x80000001), (zeros_t, None, 0), (None, zeros_r, 0), (None, None, 1)]
    cuts = [2 * 3001] * len(bad)
    cuts.append(tc.NBYTES - sum(cuts))
    with _handle(pkg, su["shape"], ns) as bc:
        bc.tune(ctaps=good_t, rot=good_r)
        name = bc.kernel_name
        one = bc.process_batch(su["iq"])
        # |rot| == pi exactly is taken
        bc.tune(ctaps=good_t, rot=with_(good_r, 0, -tr.PI_F))
        bc.tune(ctaps=good_t, rot=good_r)
        parts, pos = ([], [], []), 0
        for k, c in enumerate(cuts):
            l, r, w, _ = bc.process_batch(su["iq"][:, pos:pos + c])
            for acc, v in zip(parts, (l, r, w)):
                acc.append(v)
            pos += c
            if k < len(bad):
                t, ro, fl = bad[k]
                rc = lib.sdrfm_bcast_tune(bc._h, t.ctypes.data if t is not None else None, ro.ctypes.data if ro is not None else None, fl)
                assert rc == pkg.lib.EINVAL, (k, rc)
                assert bc.kernel_name == name
        for acc, o, what in zip(parts, one[:3], "LRw"):
            assert _same(np.concatenate(acc, 1), o), what
        assert lib.sdrfm_bcast_tune(None, None, None, 0) == pkg.lib.EINVAL
        with pytest.raises(pkg.SdrfmError):
            bc.tune(ctaps=bad[0][0], rot=good_r)
    # an untuned handle stays untuned
    with _handle(pkg, su["shape"], ns) as bc:
        first = bc.process_batch(su["iq"][:, :2 * 9001])
        name = bc.kernel_name
        for t, ro, fl in bad:
            assert lib.sdrfm_bcast_tune(bc._h, t.ctypes.data if t is not None else None, ro.ctypes.data if ro is not None else None, fl) == pkg.lib.EINVAL
        assert bc.kernel_name == name
        rest = bc.process_batch(su["iq"][:, 2 * 9001:])
    with _handle(pkg, su["shape"], ns) as bc:
        whole = bc.process_batch(su["iq"])
    assert _same(np.concatenate([first[0], rest[0]], 1), whole[0]) and _same(np.concatenate([first[2], rest[2]], 1), whole[2])


# ---- 8. the PCM one-call form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_pcm_one_call_form_is_the_tuned_call_and_the_sink(pkg, generic):
    su = tc.case_setup(pkg, tc.CASES[0])
    ns, half = su["ns"], 2 * 30001
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    chunks = [su["iq"][:, :half], su["iq"][:, half:]]
    with _handle(pkg, su["shape"], ns, generic=generic) as bc, pkg.StereoPcmSink(ns, alpha, gain) as sink:
        bc.tune(ctaps=su["ctaps"], rot=su["rot"])
        want = []
        for c in chunks:
            l, r, w, pc = bc.process_batch(c)
            want.append((l, r, sink.process_batch(l, r), w, pc))
        bc.reset()
        sink.reset()
        for k, c in enumerate(chunks):
            l, r, pcm, w, pc = bc.process_batch_pcm(sink, c, with_audio=k == 0)
            if k == 0:
                assert _same(l, want[k][0]) and _same(r, want[k][1])
            assert np.array_equal(pcm, want[k][2]) and _same(w, want[k][3]) and np.array_equal(pc, want[k][4]), k
        assert bc.kernel_name == _want_name(su["shape"], generic, True)


# ---- 9. three stations from one capture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_three_stations_from_one_shared_capture(pkg, generic):
    iq, sts = tc.three_stations(pkg)
    with _handle(pkg, tc.SHAPES["default"], 3, nbytes=iq.shape[1], generic=generic) as bc:
        bc.tune(offsets_hz=[st["offset_hz"] for st in sts], fs=2.4e6, shared_input=True)
        L, R, bb, pc = bc.process_batch(iq)
        name = bc.kernel_name
    for k, st in enumerate(sts):
        with pkg.RdsSync(9600.0) as sync:
            info = pkg.rds_parse(sync.push(bb[k]))
        assert info["pi"] == st["pi"] and info["ps"] == st["ps"], (k, info)
        sl, sr, _ = separation_db(L[k], R[k], st["left_hz"], st["right_hz"])
        print("%s: station %d at %+.0f kHz: PS %r, separation %.2f / %.2f dB, pilot count %d" % (name, k, st["offset_hz"] / 1e3, info["ps"], sl, sr, int(pc[k])))
        assert min(sl, sr) >= tc.STATIONS_SEPARATION_DB[k] - 1.0, (k, sl, sr)
