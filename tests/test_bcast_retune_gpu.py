"""GPU tests of the re-tune of a running broadcast handle (sdrfm_bcast_retune).  Bit for bit and without a reference: the
identity re-tune, an untuned handle re-tuned to (h, 0), fast against generic, any cut into calls round the re-tune, the settled outputs
against a handle tuned that way from its first byte, one shared row against replicated rows, host against device buffers, a restart per
stream against an untouched handle, a fresh one and sdrfm_bcast_tune.  Against tests/retune_ref.py at 1e-5 (the cases of
tests/retune_cases.py, whose outputs at the pilot gate tests/test_retune_ref.py counts without a device): offsets moved by +5 kHz, -7 kHz
and across the rot wrap, with and without the carry, restarts at non-zero phases, two re-tunes with no call between them.  Then the PCM
and the metered call forms, reset, the refusals, and one drifted capture followed end to end with no tune after the first."""
import ctypes as C

import numpy as np
import pytest

import retune_cases as rc
import scan_cases as sc
import tuned_cases as tc
import tuned_ref as tr
from test_bcast_tuned_gpu import KERNELS, KERNEL_IDS, TOL, _handle, _same, _untuned_inputs, _want_name

pytestmark = pytest.mark.gpu

FIELDS = ("n", "n_pilot", "rf_q", "freq_q", "dev_q", "pilot_q", "pilot2_q")
N0 = rc.N0
FOLLOW_N0 = 120033
CASE_OF = {name: next(c for c in rc.CASES if c[0] == name and c[2] == "signal") for name in tc.SHAPES}


def _seq(bc, iq, cuts, acts=None):
    """the calls one after the other, acts[k](bc) before call k; returns (L, R, bb, summed pilot counts)"""
    parts, pct, pos = ([], [], []), 0, 0
    for k, c in enumerate(cuts):
        if acts and k in acts:
            acts[k](bc)
        want = bc.counts(c)
        l, r, w, pc = bc.process_batch(iq[:, pos:pos + c])
        assert (l.shape[1], w.shape[1]) == want, (c, l.shape, w.shape, want)
        for acc, v in zip(parts, (l, r, w)):
            acc.append(v)
        pct = pct + pc.astype(np.int64)
        pos += c
    assert pos == iq.shape[1], (pos, iq.shape)
    return tuple(np.concatenate(p, 1) for p in parts) + (pct,)


def _all_same(a, b, where):
    for x, y, what in zip(a[:3], b[:3], ("L", "R", "bb")):
        assert _same(x, y), (where, what)
    assert np.array_equal(a[3], b[3]), (where, a[3], b[3])


def _retune(su, carry=True, restart=None, **kw):
    return lambda bc: bc.retune(ctaps=su["new"][0], rot=su["new"][1], carry=su["carry"] if carry else None, restart=restart, **kw)


def _settled(shape, n, m0, audio):
    """the outputs all of whose d's have an index above m0"""
    T, D, P, Ta, Da, Tr, Dr = shape
    taps, decim = (Ta, Da) if audio else (Tr, Dr)
    return (np.arange(n) + 1) * decim - 1 - (taps - 1) - (P - 1) > m0


# ---- 1. bit for bit, no reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_identity_retune_changes_no_bit(pkg, name, generic):
    """the same taps and rotations in mid-sequence, carry NULL, carry (1, 0) and through offsets_hz (taps.retune_carry of no move is
    bitwise (1, 0)): a handle never re-tuned"""
    su = rc.case_setup(pkg, CASE_OF[name])
    shape, ns, fs = su["shape"], su["ns"], tc.fs_of(su["shape"][1])
    cuts = [2 * N0, 2 * 5001, tc.NBYTES - 2 * N0 - 2 * 5001 - 2 * 4002, 2 * 4002]
    ones = np.tile(np.array([1.0, 0.0], np.float32), (ns, 1))
    with _handle(pkg, shape, ns, generic=generic) as bc, _handle(pkg, shape, ns, generic=generic) as other:
        bc.tune(offsets_hz=su["old_hz"], fs=fs)
        other.tune(offsets_hz=su["old_hz"], fs=fs)
        want = _seq(other, su["iq"], cuts)
        got = _seq(bc, su["iq"], cuts, {1: lambda b: b.retune(offsets_hz=su["old_hz"], fs=fs),
                                        2: lambda b: b.retune(ctaps=su["old"][0], rot=su["old"][1]),
                                        3: lambda b: b.retune(ctaps=su["old"][0], rot=su["old"][1], carry=ones)})
        assert bc.kernel_name == _want_name(shape, generic, True)
    _all_same(got, want, name)


@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_untuned_handle_retuned_to_offset_zero_is_the_untuned_handle(pkg, name, generic):
    """taps (h, 0) and rot 0 on an untuned handle in mid-stream: the kernel changes, the bits do not (rot_old is 0: nothing is shifted)"""
    shape = tc.SHAPES[name]
    ns = 7 if not generic else (3, 7, 1)[list(tc.SHAPES).index(name) % 3]
    iq = _untuned_inputs(pkg, shape, ns)
    h = tc.shape_taps(pkg, shape)[0]
    cuts = [2 * N0, tc.NBYTES - 2 * N0]
    with _handle(pkg, shape, ns, generic=generic) as bc, _handle(pkg, shape, ns, generic=generic) as other:
        want = _seq(other, iq, cuts)
        names = []

        def act(b):
            names.append(b.kernel_name)
            b.retune(ctaps=np.tile(tr.pairs(h), (ns, 1)), rot=np.zeros(ns, np.float32))
            names.append(b.kernel_name)
        got = _seq(bc, iq, cuts, {1: act})
    assert names == [_want_name(shape, generic, False), _want_name(shape, generic, True)], names
    _all_same(got, want, name)
    assert int(want[3].max()) > 0


def test_fast_is_generic_across_a_real_retune(pkg):
    su = rc.case_setup(pkg, ("default", 7, "signal"))
    cuts, outs = [2 * N0, tc.NBYTES - 2 * N0], []
    for generic in (False, True):
        with _handle(pkg, su["shape"], su["ns"], generic=generic) as bc:
            bc.tune(ctaps=su["old"][0], rot=su["old"][1])
            outs.append(_seq(bc, su["iq"], cuts, {1: _retune(su)}))
            assert bc.kernel_name == _want_name(su["shape"], generic, True)
    _all_same(outs[0], outs[1], "fast against generic")


@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_any_cut_before_and_after_the_retune(pkg, name, generic):
    """the re-tune after N0 samples, where the input phase and both decimator phases are non-zero; before it and behind it 0-byte and 2-byte
    calls, calls one short of an output, and a call whose M is below H directly behind the re-tune"""
    su = rc.case_setup(pkg, CASE_OF[name])
    shape, ns = su["shape"], su["ns"]
    T, D, P, Ta, Da, Tr, Dr = shape
    H = P - 1 + max(Ta, Tr) - 1
    assert all(rc.phases(shape))
    rest = tc.NBYTES - 2 * N0
    before = [0, 2, 2 * D * Da - 4, 2 * 9001]
    before.append(2 * N0 - sum(before))
    short = 2 * D * (H // 2) - 2                                  # M < H
    afters = [[short, 0, 2, 2 * D * Dr - 4, 2 * 7003], [0, 2, short, 2 * 11001], [2, 2 * 20001]]
    with _handle(pkg, shape, ns, generic=generic) as bc:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        want = _seq(bc, su["iq"], [2 * N0, rest], {1: _retune(su)})
        for k, after in enumerate(afters):
            after = after + [rest - sum(after)]
            assert all(c >= 0 and c % 2 == 0 for c in before + after), (before, after)
            bc.tune(ctaps=su["old"][0], rot=su["old"][1])
            got = _seq(bc, su["iq"], before + after, {len(before): _retune(su)})
            _all_same(got, want, (name, k))


@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_settled_outputs_are_a_handles_tuned_that_way_from_the_first_byte(pkg, name, generic):
    su = rc.case_setup(pkg, CASE_OF[name])
    shape, ns, m0 = su["shape"], su["ns"], N0 // su["shape"][1]
    with _handle(pkg, shape, ns, generic=generic) as bc, _handle(pkg, shape, ns, generic=generic) as other:
        other.tune(ctaps=su["new"][0], rot=su["new"][1])
        want = other.process_batch(su["iq"])
        for carry in (True, False):
            bc.tune(ctaps=su["old"][0], rot=su["old"][1])
            got = _seq(bc, su["iq"], [2 * N0, tc.NBYTES - 2 * N0], {1: _retune(su, carry)})
            sa, sr_ = _settled(shape, got[0].shape[1], m0, True), _settled(shape, got[2].shape[1], m0, False)
            assert sa.sum() > 10 and sr_.sum() > 10 and not sa[:m0 // shape[4]].any()
            assert _same(got[0][:, sa], want[0][:, sa]) and _same(got[1][:, sa], want[1][:, sa]) and _same(got[2][:, sr_], want[2][:, sr_]), (name, carry)
            assert not _same(got[0][:, ~sa], want[0][:, ~sa])        # (the old tuning did receive something else)


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_shared_row_replicated_rows_and_device_buffers(pkg, generic):
    import torch
    shape, ns, nbytes = tc.SHAPES["default"], 3, tc.NBYTES
    row = tc.three_stations(pkg)[0][:, :nbytes]
    new = np.array([st["offset_hz"] for st in tc.STATIONS])
    old = new + np.array([5e3, -7e3, 2e3])
    cuts = [2 * N0, 0, 2 * 7, nbytes - 2 * N0 - 14]
    with _handle(pkg, shape, ns, generic=generic) as bc:
        bc.tune(offsets_hz=old)
        want = _seq(bc, np.repeat(row, ns, 0), cuts, {1: lambda b: b.retune(offsets_hz=new)})
        assert bc._shared_input is False
        bc.tune(offsets_hz=old, shared_input=True)
        got = _seq(bc, row, cuts, {1: lambda b: b.retune(offsets_hz=new)})     # shared_input=None keeps the setting
        assert bc._shared_input is True
        _all_same(got, want, "shared against replicated rows")
        bc.tune(offsets_hz=old)
        got = _seq(bc, np.repeat(row, ns, 0)[:, :2 * N0], [2 * N0])
        bc.retune(offsets_hz=new, shared_input=True)                 # the setting replaced by the re-tune itself
        rest = _seq(bc, row[:, 2 * N0:], cuts[1:])
        for g, r_, w in zip(got[:3], rest[:3], want[:3]):
            assert _same(np.concatenate([g, r_], 1), w)
        # device buffers, canaries round the outputs and the row
        na, nr = want[0].shape[1], want[2].shape[1]
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[32:32 + nbytes] = torch.from_numpy(row[0].copy()).cuda()
        d_l = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns, na + 5), -7.0, dtype=torch.float32, device="cuda")
        d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bc.tune(offsets_hz=old, shared_input=True)
        pos, oa, ow, pct = 0, 0, 0, 0
        for k, c in enumerate(cuts):
            if k == 1:
                bc.retune(offsets_hz=new)
            a, w_ = bc.process_batch_device(buf[32 + pos:32 + pos + c].unsqueeze(0), d_l[:, oa:], d_r[:, oa:], d_w[:, ow:], d_pc, nbytes=c)
            bc.synchronize()
            pct = pct + d_pc.cpu().numpy().astype(np.int64) if c else pct
            pos, oa, ow = pos + c, oa + a, ow + 2 * w_
        assert (oa, ow) == (na, 2 * nr)
        assert _same(d_l[:, :na].cpu().numpy(), want[0]) and _same(d_r[:, :na].cpu().numpy(), want[1])
        assert _same(d_w[:, :2 * nr].cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32))
        assert np.array_equal(pct, want[3])
        assert (d_l[:, na:] == -7.0).all() and (d_r[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all()
        assert (buf[:32] == 0xA5).all() and (buf[32 + nbytes:] == 0xA5).all()


# ---- 2. restart per stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", [("default", False), ("default", True), ("T7-D3-P5", True)], ids=["default-fast", "default-generic", "T7-D3-P5-generic"])
def test_restart_per_stream(pkg, name, generic):
    """7 streams, streams 2 and 5 restarted with new offsets after 30000 samples, where all three phases are 0: the kept streams are a
    handle's that was never touched, the restarted ones a fresh handle's fed from that byte on, and a restart of all is sdrfm_bcast_tune"""
    su = rc.case_setup(pkg, (name, 7, "signal"))
    shape, ns, n0 = su["shape"], 7, 30000
    assert not any(rc.phases(shape, n0))
    moved = [2, 5]
    kept = [s for s in range(ns) if s not in moved]
    flags = np.array([1 if s in moved else 0 for s in range(ns)], np.uint8)
    ctaps, rot = su["old"][0].copy(), su["old"][1].copy()
    ctaps[moved], rot[moved] = su["new"][0][moved], su["new"][1][moved]
    cuts = [2 * n0, tc.NBYTES - 2 * n0]
    with _handle(pkg, shape, ns, generic=generic) as bc, _handle(pkg, shape, ns, generic=generic) as other:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        got = _seq(bc, su["iq"], cuts, {1: lambda b: b.retune(ctaps=ctaps, rot=rot, restart=flags)})
        other.tune(ctaps=su["old"][0], rot=su["old"][1])
        never = _seq(other, su["iq"], cuts)
        for g, w in zip(got[:3], never[:3]):
            assert _same(g[kept], w[kept])
        assert np.array_equal(got[3][kept], never[3][kept])
        other.tune(ctaps=ctaps, rot=rot)                             # a fresh handle, fed from byte 2 n0 on
        fresh = other.process_batch(su["iq"][:, 2 * n0:])
        for g, w in zip(got[:3], fresh[:3]):
            assert _same(g[moved][:, g.shape[1] - w.shape[1]:], w[moved])
            assert not _same(g[kept][:, g.shape[1] - w.shape[1]:], w[kept])
        # a restart of every stream is sdrfm_bcast_tune
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        every = _seq(bc, su["iq"], cuts, {1: lambda b: b.retune(ctaps=su["new"][0], rot=su["new"][1], carry=su["carry"], restart=np.ones(ns, np.uint8))})
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        tuned = _seq(bc, su["iq"], cuts, {1: lambda b: b.tune(ctaps=su["new"][0], rot=su["new"][1])})
        _all_same(every, tuned, "restart of all against tune")


# ---- 3. against the reference --------------------------------------------------------------------------------------------------------
def _check(su, refs, got, where):
    frac = rc.excluded(refs)
    assert frac <= tc.EXCLUDED_CAP, frac
    L, R, bb, pc = got
    worst = 0.0
    for s, r in enumerate(refs):
        assert L[s].shape == r["L"].shape and bb[s].shape == r["bb"].shape, (where, s, L[s].shape, r["L"].shape, bb[s].shape, r["bb"].shape)
        assert r["lo"] <= int(pc[s]) <= r["lo"] + r["n_amb"], (where, s, int(pc[s]), r["lo"], r["n_amb"])
        for g, w, keep, what in ((L[s], r["L"], r["keep_a"], "L"), (R[s], r["R"], r["keep_a"], "R"), (bb[s].real, r["bb"].real, r["keep_r"], "wr"),
                                 (bb[s].imag, r["bb"].imag, r["keep_r"], "wi")):
            err = np.abs(g[keep].astype(np.float64) - w[keep].astype(np.float64))
            if err.size:
                e = float(err.max())
                worst = max(worst, e)
                assert e <= TOL, (where, s, su["names"][s], what, e, int(np.flatnonzero(keep)[np.argmax(err)]))
    return worst, frac


@pytest.mark.parametrize("case", rc.CASES, ids=[rc.case_id(c) for c in rc.CASES])
def test_retuned_streams_against_the_reference(pkg, case):
    """+5 kHz, -7 kHz and across the rot wrap in turn, with the carry and without it, and streams 2 and 5 restarted instead — at N0, where
    all three phases are non-zero: the restarted streams' x is 0 before input N0"""
    for generic in ((False, True) if case[0] == "default" else (True,)):
        for with_carry, restart in ((True, ()), (False, ()), (True, (2, 5))):
            su, refs = rc.case_reference(pkg, case, with_carry, restart)
            flags = np.array([1 if s in restart else 0 for s in range(su["ns"])], np.uint8) if restart else None
            with _handle(pkg, su["shape"], su["ns"], su["pilot_min"], generic=generic) as bc:
                bc.tune(ctaps=su["old"][0], rot=su["old"][1])
                got = _seq(bc, su["iq"], [2 * N0, tc.NBYTES - 2 * N0], {1: _retune(su, with_carry, flags)})
                name = bc.kernel_name
            assert name == _want_name(su["shape"], generic, True), name
            worst, frac = _check(su, refs, got, (name, with_carry, restart))
            print("%s, carry %s, restarted %s: %s moved by %s Hz, pilot counts %s: worst |error| %.3g, %.3f %% of the outputs excluded" % (
                name, with_carry, restart, "/".join(su["names"]), [int(round(v)) for v in su["new_hz"] - su["old_hz"]], [int(v) for v in got[3]], worst, 100 * frac))


@pytest.mark.parametrize("name,generic", [("default", False), ("T7-D3-P5", True)], ids=["default-fast", "T7-D3-P5-generic"])
def test_two_retunes_with_no_call_between_them(pkg, name, generic):
    """old -> halfway -> new with no call between: the carry applied twice, the shifts added — tests/retune_ref.py with two events at one
    m0, at the bound of every comparison of a device's d with the scalar-C definition's (its arctangent differs in the last bits, so
    this is no bitwise comparison); the wrap stream's halfway rotation is pi itself"""
    su, mid, (c1, c2), refs = rc.two_step_reference(pkg, CASE_OF[name])
    shape, ns = su["shape"], su["ns"]

    def act(b):
        b.retune(ctaps=mid[0], rot=mid[1], carry=c1)
        b.retune(ctaps=su["new"][0], rot=su["new"][1], carry=c2)
    with _handle(pkg, shape, ns, generic=generic) as bc:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        got = _seq(bc, su["iq"], [2 * N0, tc.NBYTES - 2 * N0], {1: act})
    worst, frac = _check(su, refs, got, name)
    print("%s, two re-tunes: worst |error| %.3g, %.3f %% of the outputs excluded" % (name, worst, 100 * frac))


# ---- 4. other call forms -------------------------------------------------------------------------------------------------------------
def _sinks(pkg, ns):
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    return pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_pcm_form_across_a_retune(pkg, generic):
    su = rc.case_setup(pkg, CASE_OF["default"])
    ns = su["ns"]
    chunks = [su["iq"][:, :2 * N0], su["iq"][:, 2 * N0:]]
    a, b_ = _sinks(pkg, ns)
    with _handle(pkg, su["shape"], ns, generic=generic) as bc, _handle(pkg, su["shape"], ns, generic=generic) as other, a as sink, b_ as other_sink:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        other.tune(ctaps=su["old"][0], rot=su["old"][1])
        for k, c in enumerate(chunks):
            if k == 1:
                _retune(su)(bc)
                _retune(su)(other)
            l, r, pcm, w, pc = bc.process_batch_pcm(sink, c)
            wl, wr, ww, wpc = other.process_batch(c)
            wpcm = other_sink.process_batch(wl, wr)
            assert _same(l, wl) and _same(r, wr) and _same(w, ww) and np.array_equal(pc, wpc), k
            assert np.array_equal(pcm, wpcm) and _same(sink.state(), other_sink.state()), k


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_metered_calls_behind_a_retune(pkg, generic):
    """directly behind the re-tune: n = M, n_pilot = pilot_count, the outputs a plain call's; once the new d's lie beyond m0 + P: all seven
    fields are those of a handle tuned that way from the first byte"""
    su = rc.case_setup(pkg, CASE_OF["default"])
    shape, ns, iq = su["shape"], su["ns"], su["iq"]
    T, D, P = shape[:3]
    gap = 2 * D * (P + 2)
    with _handle(pkg, shape, ns, generic=generic) as bc, _handle(pkg, shape, ns, generic=generic) as other:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        other.tune(ctaps=su["old"][0], rot=su["old"][1])
        bc.process_batch(iq[:, :2 * N0])
        other.process_batch(iq[:, :2 * N0])
        _retune(su)(bc)
        _retune(su)(other)
        M = bc.counts(gap)
        l, r, w, pc, m = bc.process_batch_metered(iq[:, 2 * N0:2 * N0 + gap])
        plain = other.process_batch(iq[:, 2 * N0:2 * N0 + gap])
        assert (l.shape[1], w.shape[1]) == M
        assert (m["n"] == (N0 % D + gap // 2) // D).all() and np.array_equal(m["n_pilot"], pc.astype(np.uint64)) and (m["reserved"] == 0).all()
        _all_same((l, r, w, pc), plain, "metered directly behind the re-tune")
        late = bc.process_batch_metered(iq[:, 2 * N0 + gap:])
        other.tune(ctaps=su["new"][0], rot=su["new"][1])             # tuned that way from the first byte
        other.process_batch(iq[:, :2 * N0 + gap])
        want = other.process_batch_metered(iq[:, 2 * N0 + gap:])
    for s in range(ns):
        for f in FIELDS:
            assert int(late[4][f][s]) == int(want[4][f][s]), (s, f, int(late[4][f][s]), int(want[4][f][s]))
    assert int(late[4]["n_pilot"].max()) > 0 and int(late[4]["rf_q"].max()) > 0


def test_reset_after_retune_keeps_the_tuning(pkg):
    su = rc.case_setup(pkg, CASE_OF["default"])
    with _handle(pkg, su["shape"], su["ns"]) as bc, _handle(pkg, su["shape"], su["ns"]) as other:
        other.tune(ctaps=su["new"][0], rot=su["new"][1])
        want = other.process_batch(su["iq"])
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        bc.process_batch(su["iq"][:, :2 * N0])
        _retune(su)(bc)
        bc.reset()
        got = bc.process_batch(su["iq"])
        assert bc.kernel_name == _want_name(su["shape"], False, True)
    _all_same(got, want, "reset behind a re-tune")


def test_every_refusal_leaves_the_next_call_unchanged(pkg):
    su = rc.case_setup(pkg, CASE_OF["default"])
    ns, lib = su["ns"], pkg.load_library()
    t, r, c = (np.ascontiguousarray(v, np.float32).copy() for v in (su["new"][0], su["new"][1], su["carry"]))
    flags = np.zeros(ns, np.uint8)

    def bad(v, at, value):
        v = v.copy()
        v.reshape(-1)[at] = value
        return v
    p = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    refusals = [(None, r, c, flags, 0), (t, None, c, flags, 0), (None, None, None, None, 0), (bad(t, 5, np.nan), r, c, flags, 0),
                (bad(t, t.size - 1, np.inf), r, None, None, 0), (t, bad(r, ns - 1, np.nan), c, flags, 0), (t, r, bad(c, 3, -np.inf), flags, 0),
                (t, bad(r, 0, np.nextafter(np.float32(np.pi), np.float32(4))), c, flags, 0), (t, bad(r, 1, -3.2), None, None, 0),
                (t, r, c, flags, 2), (t, r, c, flags, pkg.lib.TUNE_SHARED_INPUT | 4), (t, r, c, bad(flags, ns - 1, 2), 0), (t, r, None, bad(flags, 0, 255), 0)]
    cuts = [2 * 2001] * len(refusals)
    cuts.append(tc.NBYTES - sum(cuts))
    with _handle(pkg, su["shape"], ns) as bc, _handle(pkg, su["shape"], ns) as other:
        bc.tune(ctaps=su["old"][0], rot=su["old"][1])
        other.tune(ctaps=su["old"][0], rot=su["old"][1])
        want = _seq(other, su["iq"], cuts)

        def refuse(k):
            def act(b):
                a = refusals[k - 1]
                assert lib.sdrfm_bcast_retune(b._h, p(a[0]), p(a[1]), p(a[2]), p(a[3]), a[4]) == pkg.lib.EINVAL, k
            return act
        got = _seq(bc, su["iq"], cuts, {k: refuse(k) for k in range(1, len(cuts))})
        assert bc._shared_input is False
        with pytest.raises(pkg.SdrfmError) as e:
            bc.retune(ctaps=bad(t, 0, np.nan), rot=r)
        assert e.value.status == pkg.lib.EINVAL
    _all_same(got, want, "refusals")


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_a_drifted_receiver_follows_its_stations_without_a_restart(pkg):
    """scenario "crystal+7kHz-and-mono" on a 4-stream shared-input handle: metered calls, stream_status, follow, more metered calls, no tune
    after the first.  Afterwards every stream is within 100 Hz; the audio over the correction is tests/retune_ref.py's for the offsets the
    handle chose, and so is the RDS group count"""
    name = "crystal+7kHz-and-mono"
    row, truth = sc.scenario_capture(pkg, name)
    truth = sorted(truth, key=lambda t: t["offset_hz"])
    offsets, _, _ = sc.scenario_reference(pkg, name)
    tuned = offsets[[int(np.argmin(np.abs(offsets - t["offset_hz"]))) for t in truth]]
    shape = tc.SHAPES["default"]
    D = shape[1]
    n0 = FOLLOW_N0                                                  # samples before the correction: all three phases non-zero
    assert all(rc.phases(shape, n0))
    cuts = [2 * 60001, 2 * n0 - 2 * 60001, 2 * 50007, row.size - 2 * n0 - 2 * 50007]
    parts, pos = ([], [], []), 0
    with _handle(pkg, shape, 4, pilot_min=sc.PILOT_MIN, nbytes=row.size) as bc:
        bc.tune(offsets_hz=tuned, fs=sc.FS, shared_input=True)
        acc = np.zeros(4, pkg.METER_DTYPE)
        for k, c in enumerate(cuts):
            if k == 2:
                status = pkg.stream_status(pkg.meter_report(acc, sc.FS, D), tuned)
                assert bc.follow(status) == [0, 1, 2, 3]
                acc = np.zeros(4, pkg.METER_DTYPE)
            out = bc.process_batch_metered(row[None, pos:pos + c])
            for a, v in zip(parts, out[:3]):
                a.append(v)
            pkg.meter_add(acc, out[4])
            pos += c
        chosen = np.array(bc._offsets_hz)
        assert bc.kernel_name.startswith("bcast-fast-tuned") and bc._shared_input is True
    L, R, bb = (np.concatenate(p, 1) for p in parts)
    rep = pkg.meter_report(acc, sc.FS, D)
    print("moved to %s Hz (the stations lie at %s); freq_err after the correction %s Hz" % (
        [round(float(v), 1) for v in chosen], [t["offset_hz"] for t in truth], [round(float(v), 1) for v in rep["freq_err_hz"]]))
    assert np.abs(rep["freq_err_hz"]).max() < 100.0, rep["freq_err_hz"]
    assert all(abs(chosen[s] - t["offset_hz"]) < 100.0 for s, t in enumerate(truth)), chosen
    refs = rc.follow_reference(pkg, row, tuned, chosen, n0, sc.PILOT_MIN)
    frac = rc.excluded(refs)
    assert frac <= tc.EXCLUDED_CAP, frac
    for s, r in enumerate(refs):
        for g, w, what in ((L[s], r["L"], "L"), (R[s], r["R"], "R")):
            e = float(np.abs(g[r["keep_a"]].astype(np.float64) - w[r["keep_a"]]).max())
            assert e <= TOL, (s, what, e)
        with pkg.RdsSync(9600.0) as sync, pkg.RdsSync(9600.0) as ref_sync:
            assert len(sync.push(bb[s])) == len(ref_sync.push(r["bb"])), s
