"""GPU tests of the broadcast handle's audio conditioning (sdrfm_bcast_set_audio / sdrfm_bcast_get_audio) on the shapes and
rows of tests/tuned_cases.py.  Bit for bit where the definition allows it: blend = gain = 1 against a plain handle in every call form, blend
0 against a handle made with diff_gain = 0, power-of-two blends against handles made with diff_gain scaled, power-of-two gains against the
plain rows scaled, a gain ramp at blend 0 against the mono rows times the reference's mu_j, any cut of a capture into calls round a ramp and
round a set in mid-ramp.  Against tests/audio_ref.py at a derived tolerance: both ramps at once on an L-only tone.  Then reset, tune,
retune, the refusals, and the device-pointer form on the caller's stream.  Audio is compared as values (a product with mu = 0 may differ
from the reference in the sign of a zero), bb, pilot_count and the records as integers."""
import ctypes as C

import numpy as np
import pytest

import audio_ref as ar
import tuned_cases as tc
from test_bcast_tuned_gpu import _bits, _same, _untuned_inputs, _want_name

pytestmark = pytest.mark.gpu

KERNELS = [("default", False), ("default", True), ("T7-D3-P5", True), ("T16-D8", True)]
KERNEL_IDS = ["%s-%s" % (n, "generic" if g else "fast") for n, g in KERNELS]
CASE_OF = {"default": ("default", 3, "signal"), "T7-D3-P5": ("T7-D3-P5", 7, "signal"), "T16-D8": ("T16-D8", 1, "signal")}
FIELDS = ("n", "n_pilot", "rf_q", "freq_q", "dev_q", "pilot_q", "pilot2_q", "reserved")
ONE = ar.ONE


def _mk(pkg, shape, ns, generic, dg_scale=1.0, nbytes=tc.NBYTES):
    """tests/test_bcast_tuned_gpu.py's handle with diff_gain scaled (a power of two, or 0: exact in fp32)"""
    T, D, P, Ta, Da, Tr, Dr = shape
    h, ga, gr, b, dg, rg = tc.shape_taps(pkg, shape)
    return pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b, pilot_min=0.05,
                                                  diff_gain=float(np.float32(dg) * np.float32(dg_scale)), rds_gain=rg, fir_decim=D, audio_decim=Da,
                                                  rds_decim=Dr, n_streams=ns, max_bytes_per_call=nbytes, force_generic=generic))


def _station_rows(pkg, shape, ns):
    """ns station rows at 0 Hz for an untuned handle (tests/tuned_cases.py's station class), made once"""
    fs = tc.fs_of(shape[1])
    return np.stack([tc.stream_input(pkg, "station", 0.0, fs, tc.NBYTES // 2, 7900 + s) for s in range(ns)])


def _seq(bc, iq, cuts, acts=None, ref=None):
    """the calls one after the other, acts[k](bc) before call k; ref: an audio_ref.AudioState moved along, the handle's audio_state held to
    it after every call.  Returns (L, R, bb, summed pilot counts) and, with ref, the reference's (b, v) per output"""
    parts, pct, pos, bs, vs = ([], [], []), 0, 0, [], []
    for k, c in enumerate(cuts):
        if acts and k in acts:
            acts[k](bc)
        want = bc.counts(c)
        l, r, w, pc = bc.process_batch(iq[:, pos:pos + c])
        assert (l.shape[1], r.shape[1], w.shape[1]) == (want[0], want[0], want[1]), (c, l.shape, w.shape, want)
        for acc, v in zip(parts, (l, r, w)):
            acc.append(v)
        pct = pct + pc.astype(np.int64)
        pos += c
        if ref is not None:
            b, v = ref.call(l.shape[1])
            bs.append(b)
            vs.append(v)
            ref.check(bc.audio_state())
    assert pos == iq.shape[1], (pos, iq.shape)
    out = tuple(np.concatenate(p, 1) for p in parts) + (pct,)
    return out if ref is None else out + (np.concatenate(bs, 1), np.concatenate(vs, 1))


def _eq(got, want, where):
    """L and R as values, bb and the pilot counts as integers"""
    for x, y, what in zip(got[:2], want[:2], ("L", "R")):
        assert x.shape == y.shape and not np.isnan(x).any() and np.array_equal(x, y), (where, what)
    assert _same(got[2], want[2]), (where, "bb")
    assert np.array_equal(got[3], want[3]), (where, got[3], want[3])


def _set(blend=None, gain=None, slew=ONE, ref=None):
    """set_audio through the C call with an explicit slew, the reference moved with it"""
    def act(bc):
        ns = bc.cfg.n_streams
        b = None if blend is None else np.ascontiguousarray(np.broadcast_to(np.asarray(blend), (ns,)), dtype=np.uint16)
        g = None if gain is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gain), (ns,)), dtype=np.uint16)
        st = bc._lib.sdrfm_bcast_set_audio(bc._h, None if b is None else b.ctypes.data, None if g is None else g.ctypes.data, int(slew))
        assert st == 0, st
        if ref is not None:
            ref.set(b, g, slew)
            ref.check(bc.audio_state())
    return act


def _sinks(pkg, ns):
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    return pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)


def _inputs(pkg, name, tuned):
    """(shape, ns, iq, tune arguments or None) of a kernel's case: tests/tuned_cases.py's rows and tunings, or rows at 0 Hz"""
    su = tc.case_setup(pkg, CASE_OF[name])
    if tuned:
        return su["shape"], su["ns"], su["iq"], dict(ctaps=su["ctaps"], rot=su["rot"])
    return su["shape"], su["ns"], _untuned_inputs(pkg, su["shape"], su["ns"]), None


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_blend_and_gain_of_one_change_no_bit_in_any_call_form(pkg, name, generic):
    for tuned in (False, True):
        shape, ns, iq, tune = _inputs(pkg, name, tuned)
        cuts = [2 * 20001, tc.NBYTES - 2 * 20001]
        a, b_ = _sinks(pkg, ns)
        with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic) as other, a as sink, b_ as other_sink:
            if tuned:
                bc.tune(**tune)
                other.tune(**tune)
            plain = _want_name(shape, generic, tuned)
            assert bc.kernel_name == plain
            bc.set_audio(1.0, 1.0)                                   # floats, the default 50 ms
            assert bc.kernel_name == plain + " blend" and other.kernel_name == plain
            got, want = _seq(bc, iq, cuts), _seq(other, iq, cuts)
            for x, y in zip(got[:3], want[:3]):
                assert _same(x, y), (name, tuned)
            assert np.array_equal(got[3], want[3])
            assert int(want[3].max()) > 0 or name != "default"
            # the metered form: the same outputs and equal records
            bc.reset()
            other.reset()
            gm, wm = bc.process_batch_metered(iq), other.process_batch_metered(iq)
            for x, y in zip(gm[:3], wm[:3]):
                assert _same(x, y), (name, tuned, "metered")
            assert np.array_equal(gm[3], wm[3])
            for f in FIELDS:
                assert np.array_equal(gm[4][f], wm[4][f]), (name, tuned, f)
            assert bc.kernel_name == plain + " blend"
            # the PCM form: the same PCM and sink state
            bc.reset()
            other.reset()
            for k, (lo, hi) in enumerate(((0, cuts[0]), (cuts[0], tc.NBYTES))):
                l, r, pcm, w, pc = bc.process_batch_pcm(sink, iq[:, lo:hi])
                wl, wr, wpcm, ww, wpc = other.process_batch_pcm(other_sink, iq[:, lo:hi])
                assert _same(l, wl) and _same(r, wr) and _same(w, ww) and np.array_equal(pc, wpc), (name, tuned, k)
                assert np.array_equal(pcm, wpcm) and _same(sink.state(), other_sink.state()), (name, tuned, k)
            # ... and back
            bc.clear_audio()
            assert bc.kernel_name == plain
            bc.reset()
            other.reset()
            got, want = _seq(bc, iq, cuts), _seq(other, iq, cuts)
            for x, y in zip(got[:3], want[:3]):
                assert _same(x, y), (name, tuned, "cleared")


# ---- 2. blend 0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_blend_zero_is_a_handle_made_with_diff_gain_zero(pkg, name, generic):
    for tuned in (False, True):
        shape, ns, iq, tune = _inputs(pkg, name, tuned)
        if not tuned:
            iq = _station_rows(pkg, shape, ns)
        with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic, 0.0) as mono, _mk(pkg, shape, ns, generic) as plain:
            for h_ in (bc, mono, plain):
                if tuned:
                    h_.tune(**tune)
            bc.set_audio(blend=0, ramp_ms=0)                         # a jump: the first output is at its target
            got, want, full = bc.process_batch(iq), mono.process_batch(iq), plain.process_batch(iq)
            _eq(got, want, (name, tuned))
            assert np.array_equal(got[0], got[1])                    # L == R == am
            if name != "T7-D3-P5":                                   # (its 5-tap pilot filter passes everything: the gate is what it is)
                assert int(got[3].max()) > 0 and not np.array_equal(full[0], full[1])   # the plain handle did decode a difference


# ---- 3. powers of two ----------------------------------------------------------------------------------------------------------------
BETAS = (ONE, ONE // 2, ONE // 4, 1)                                # 1, 1/2, 1/4, 2^-15
MUS = (ONE // 2, ONE // 8, 0)                                       # 1/2, 2^-3, 0


@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_power_of_two_blends_and_gains_are_exact(pkg, name, generic):
    """seven streams on one station row: blends 1, 1/2, 1/4, 2^-15 at gain 1 against plain handles made with diff_gain * beta, gains 1/2,
    2^-3 and 0 at blend 1 against the plain row times mu"""
    shape = tc.SHAPES[name]
    row = _station_rows(pkg, shape, 1)
    ns = len(BETAS) + len(MUS)
    iq = np.repeat(row, ns, 0)
    blend = np.array(list(BETAS) + [ONE] * len(MUS), np.uint16)
    gain = np.array([ONE] * len(BETAS) + list(MUS), np.uint16)
    with _mk(pkg, shape, ns, generic) as bc:
        _set(blend, gain, ONE)(bc)
        got = bc.process_batch(iq)
        st = bc.audio_state()
        assert np.array_equal(st["blend"], blend) and np.array_equal(st["gain"], gain)
    rows = {}
    for beta in BETAS:
        with _mk(pkg, shape, 1, generic, beta / ONE) as ref:
            rows[beta] = ref.process_batch(row)
    for s, beta in enumerate(BETAS):
        _eq(tuple(v[s:s + 1] for v in got), rows[beta], (name, "beta", beta))
    assert not np.array_equal(rows[ONE][0], rows[ONE // 2][0]) or name == "T7-D3-P5"
    for k, mu in enumerate(MUS):
        s = len(BETAS) + k
        m = np.float32(mu / ONE)
        assert np.array_equal(got[0][s], rows[ONE][0][0] * m) and np.array_equal(got[1][s], rows[ONE][1][0] * m), (name, "mu", mu)
        assert _same(got[2][s], rows[ONE][2][0]) and got[3][s] == rows[ONE][3][0]
    assert not got[0][ns - 1].any() and not got[1][ns - 1].any()     # muted


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_sixty_four_streams_on_one_shared_row_each_with_its_own_pair(pkg, generic):
    """the three-station capture, 64 streams tuned to the stations in turn, stream s with blend BETAS5[s % 5] and gain MUS4[(s // 5) % 4]:
    the per-stream record is read far beyond one workgroup's streams"""
    shape, ns = tc.SHAPES["default"], 64
    row = tc.three_stations(pkg)[0][:, :tc.NBYTES]
    offs = np.array([st["offset_hz"] for st in tc.STATIONS])
    betas5, mus4 = (ONE, ONE // 2, ONE // 4, 1, 0), (ONE, ONE // 2, ONE // 8, 0)
    blend = np.array([betas5[s % 5] for s in range(ns)], np.uint16)
    gain = np.array([mus4[(s // 5) % 4] for s in range(ns)], np.uint16)
    with _mk(pkg, shape, ns, generic) as bc:
        bc.tune(offsets_hz=offs[np.arange(ns) % 3], shared_input=True)
        _set(blend, gain, ONE)(bc)
        got = bc.process_batch(row)
        assert bc.kernel_name == _want_name(shape, generic, True) + " blend"
    rows = {}
    for beta in betas5:
        with _mk(pkg, shape, 3, generic, beta / ONE) as ref:
            ref.tune(offsets_hz=offs, shared_input=True)
            rows[beta] = ref.process_batch(row)
    assert int(rows[ONE][3].min()) > 0
    for s in range(ns):
        w, m = rows[int(blend[s])], np.float32(int(gain[s]) / ONE)
        assert np.array_equal(got[0][s], w[0][s % 3] * m) and np.array_equal(got[1][s], w[1][s % 3] * m), s
        assert _same(got[2][s], w[2][s % 3]) and got[3][s] == w[3][s % 3], s


# ---- 4. ramps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_gain_ramp_at_blend_zero_is_the_mono_row_times_the_reference_ramp(pkg, name, generic):
    """exact on every shape: at blend 0 L = R = mu_j am with one rounding, am the diff_gain = 0 handle's L; the ramp runs over three calls"""
    shape = tc.SHAPES[name]
    ns = 2
    iq = _station_rows(pkg, shape, ns)
    third = (tc.NBYTES // 3) & ~1
    cuts = [third, third, tc.NBYTES - 2 * third]
    with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic, 0.0) as mono:
        am = mono.process_batch(iq)
        n_out = am[0].shape[1]
        slew = max(1, ONE // (3 * n_out // 4))                      # the ramp ends in the last call
        ref = ar.AudioState(ns)
        _set(0, [ONE, ONE // 2], ONE, ref)(bc)
        first = bc.process_batch(iq[:, :third])                     # every output at blend 0
        ref.call(first[0].shape[1])
        bc.reset()                                                   # (the ramps are complete; the streams start again)
        ref.complete()
        ref.check(bc.audio_state())
        got = _seq(bc, iq, cuts, {0: _set(None, [0, ONE], slew, ref)}, ref)
    assert (got[5][:, 0] != got[5][:, -1]).all() and (got[5][:, -1] == [0, ONE]).all() and (got[4] == 0).all()
    assert len(np.unique(got[5][0])) > n_out // 2                    # a ramp, not a step
    mu = (got[5].astype(np.float64) / ONE).astype(np.float32)
    assert np.array_equal(got[0], mu * am[0]) and np.array_equal(got[1], mu * am[0]), name
    assert _same(got[2], am[2]) and np.array_equal(got[3], am[3])


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
@pytest.mark.parametrize("slew", [40, 7])
def test_both_ramps_on_an_l_only_tone_against_the_reference(pkg, generic, slew):
    """blend 1 -> 0 while gain 0 -> 1, slew 40 (ramp and plateau inside the second call) and slew 7 (carried over four calls).  Expected
    mu_j (am +- beta_j as) in float64 with am the diff_gain = 0 handle's L and as = (L - R) / 2 of the plain handle.  Tolerance per output
    4 * 2^-23 (|am| + |as|), derived: as so estimated is within 2^-23 of that sum (L and R are each one rounding, 2^-24 of it, off), and the
    formula's three roundings — t, the sum, the product — add at most 2^-24 of it each.  The same comparison against the blend ramp moved
    by one unit must fail on at least half of the ramping outputs: one unit is mu 2^-15 |as|."""
    shape, ns, calls = tc.SHAPES["default"], 2, 6
    iq = pkg.make_iq_stereo(ns, calls * tc.NBYTES // 2, 1e3, 0.0, 50e3, first_id=8100)
    cuts = [tc.NBYTES] * calls
    with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic, 0.0) as mono, _mk(pkg, shape, ns, generic) as plain:
        am = _seq(mono, iq, cuts)[0].astype(np.float64)
        full = _seq(plain, iq, cuts)
        as_ = (full[0].astype(np.float64) - full[1].astype(np.float64)) / 2
        ref = ar.AudioState(ns)
        got = _seq(bc, iq, cuts, {0: _set(ONE, 0, ONE, ref), 1: _set(0, ONE, slew, ref)}, ref)
    n1 = got[0].shape[1] // calls
    assert not got[0][:, :n1].any() and not got[1][:, :n1].any()    # the first call: muted from its first output
    b, v = got[4], got[5]
    end = n1 + -(-ONE // slew)
    assert (b[:, n1] == ONE - slew).all() and (v[:, n1] == slew).all() and (b[:, end - 1] == 0).all() and (b[:, end - 2] > 0).all()
    assert (v[:, end - 1:] == ONE).all() and end < b.shape[1]        # the plateau
    assert (end < 2 * n1) == (slew == 40) and (end > 4 * n1) == (slew == 7)
    assert _same(got[2], full[2]) and np.array_equal(got[3], full[3])
    tol = 4 * 2.0 ** -23 * (np.abs(am) + np.abs(as_))
    print("median |as| %.3f, |am| %.3f" % (float(np.median(np.abs(as_))), float(np.median(np.abs(am)))))

    def errors(bb):
        beta, mu = bb / ONE, v / ONE
        return (np.abs(got[0].astype(np.float64) - mu * (am + beta * as_)), np.abs(got[1].astype(np.float64) - mu * (am - beta * as_)))
    el, er = errors(b.astype(np.float64))
    print("slew %d: worst error / tolerance L %.3f, R %.3f" % (slew, float((el / np.maximum(tol, 1e-30)).max()), float((er / np.maximum(tol, 1e-30)).max())))
    assert (el <= tol).all() and (er <= tol).all()
    ramping = np.zeros(b.shape, bool)
    ramping[:, n1:end - 1] = True
    sl, sr = errors(np.minimum(b + 1, ONE).astype(np.float64))
    frac = float(((sl > tol) | (sr > tol))[ramping].mean())
    print("slew %d: the ramp moved by one unit fails on %.3f of the %d ramping outputs" % (slew, frac, int(ramping.sum())))
    assert frac >= 0.5, frac


# ---- 5. cuts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_any_cut_with_a_ramp_in_progress_is_the_one_call(pkg, name, generic):
    """calls of 0 and 2 bytes, one below one audio output, one whose M is below H, and the long call of >= 3 workgroups x >= 2 steps, with
    both ramps running throughout: bitwise the one call, tuned"""
    shape, ns, iq, tune = _inputs(pkg, name, True)
    T, D, P, Ta, Da, Tr, Dr = shape
    H = P - 1 + max(Ta, Tr) - 1
    small = [0, 2, 2 * D * Da - 4, 2 * D * (H // 2) - 2, 0]
    orders = [small + [tc.NBYTES - sum(small)], [tc.NBYTES - sum(small) - 2 * 9001] + small + [2 * 9001]]
    with _mk(pkg, shape, ns, generic) as bc:
        n_out = bc.counts(tc.NBYTES)[0]
        slew = max(1, ONE // (3 * n_out // 4))
        targets = ((np.arange(ns) * 5000) % ONE, (ONE // 3 + np.arange(ns) * 3000) % ONE)

        def start(ref):
            def act(b):
                b.tune(**tune)
                b.clear_audio()                                      # blend = gain = 1 ...
                _set(targets[0], targets[1], slew, ref)(b)           # ... and off they go
            return act
        ref = ar.AudioState(ns)
        want = _seq(bc, iq, [tc.NBYTES], {0: start(ref)}, ref)
        assert (want[4][:, 0] != want[4][:, n_out // 2]).any()        # in progress
        for k, cuts in enumerate(orders):
            assert all(c >= 0 and c % 2 == 0 for c in cuts) and sum(cuts) == tc.NBYTES
            ref = ar.AudioState(ns)
            got = _seq(bc, iq, cuts, {0: start(ref)}, ref)
            for x, y, what in zip(got[:3], want[:3], ("L", "R", "bb")):
                assert _same(x, y), (name, k, what)
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])


@pytest.mark.parametrize("name,generic", KERNELS, ids=KERNEL_IDS)
def test_a_set_in_mid_ramp_at_one_output_index_whatever_the_cuts_round_it(pkg, name, generic):
    shape, ns, iq, tune = _inputs(pkg, name, False)
    iq = _station_rows(pkg, shape, ns)
    D, Da = shape[1], shape[4]
    mid = (tc.NBYTES // 5 * 2) & ~1
    a1 = 2 * D * Da * 7 + 6
    with _mk(pkg, shape, ns, generic) as bc:
        n_out = bc.counts(tc.NBYTES)[0]
        slew = max(1, ONE // (n_out // 2))
        outs = []
        for cuts, at in (([mid, tc.NBYTES - mid], 1), ([a1, mid - a1, 2, 2 * 8001, tc.NBYTES - mid - 2 - 2 * 8001], 2)):
            bc.reset()
            bc.clear_audio()
            ref = ar.AudioState(ns)
            outs.append(_seq(bc, iq, cuts, {0: _set(0, ONE // 4, slew, ref), at: _set(ONE // 2, ONE, 3 * slew, ref)}, ref))
    b = outs[0][4]
    assert (b.min(1) > 0).all() and (b.min(1) < ONE // 2).all() and (b[:, -1] == ONE // 2).all()   # turned round in mid-ramp, then arrived
    for x, y, what in zip(outs[0], outs[1], ("L", "R", "bb", "pc", "b", "v")):
        assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y), (name, what)


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_reset_and_tune_complete_the_ramps_and_retune_leaves_them_running(pkg, generic):
    shape, ns, iq, tune = _inputs(pkg, "default", True)
    part = 2 * 10001
    tb, tg = np.array([0, ONE // 3, ONE], np.uint16), np.array([ONE // 5, 0, ONE], np.uint16)
    with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic) as jump:
        jump.tune(**tune)
        _set(tb, tg, ONE)(jump)                                      # a jump: every output at the targets
        want = jump.process_batch(iq)
        for how in ("reset", "tune"):
            bc.tune(**tune)
            bc.clear_audio()
            ref = ar.AudioState(ns)
            _set(tb, tg, 3, ref)(bc)
            _seq(bc, iq[:, :part], [part], None, ref)
            st = bc.audio_state()
            assert (st["blend"][:2] != tb[:2]).all() and (st["gain"][:2] != tg[:2]).all()   # still on their way
            bc.reset() if how == "reset" else bc.tune(**tune)
            ref.complete()
            ref.check(bc.audio_state())
            st = bc.audio_state()
            assert np.array_equal(st["blend"], tb) and np.array_equal(st["gain"], tg)
            assert bc.kernel_name == _want_name(shape, generic, True) + " blend"    # the settings stay
            _eq(bc.process_batch(iq), want, how)
        # retune: the identity re-tune in mid-ramp changes neither the ramps nor a bit
        outs = []
        for acts in ({}, {1: lambda b: b.retune(ctaps=tune["ctaps"], rot=tune["rot"])}):
            bc.tune(**tune)
            bc.clear_audio()
            ref = ar.AudioState(ns)
            outs.append(_seq(bc, iq, [part, tc.NBYTES - part], {0: _set(tb, tg, 9, ref), **acts}, ref))
        for x, y in zip(outs[0], outs[1]):
            assert np.array_equal(x, y)
        assert (outs[0][4][0, part // 100:] < ONE).all() and len(np.unique(outs[1][4][0])) > 1000


def test_every_refusal_leaves_the_next_call_unchanged(pkg):
    shape, ns, iq, tune = _inputs(pkg, "default", True)
    lib = pkg.load_library()
    ok = np.array([ONE // 2, 0, ONE], np.uint16)

    def bad(at, value):
        v = ok.copy()
        v[at] = value
        return v
    p = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    refusals = [(bad(0, ONE + 1), ok, 5), (ok, bad(ns - 1, 65535), 5), (bad(1, 40000), None, ONE), (None, bad(0, ONE + 1), 1), (ok, ok, 0),
                (ok, None, 0), (None, ok, 0), (ok, ok, ONE + 1), (None, None, ONE + 1), (ok, ok, 0xFFFFFFFF)]
    cuts = [2 * 2001] * (len(refusals) + 1)
    cuts.append(tc.NBYTES - sum(cuts))
    with _mk(pkg, shape, ns, False) as bc, _mk(pkg, shape, ns, False) as other:
        assert lib.sdrfm_bcast_set_audio(None, p(ok), p(ok), 5) == pkg.lib.EINVAL and lib.sdrfm_bcast_get_audio(None, None, None, None, None) == pkg.lib.EINVAL
        bc.tune(**tune)
        other.tune(**tune)
        ra, rb = ar.AudioState(ns), ar.AudioState(ns)
        first = {0: _set([ONE, ONE // 2, 0], [ONE, ONE // 4, ONE // 2], 11, rb)}
        want = _seq(other, iq, cuts, first, rb)

        def refuse(k):
            def act(b):
                a = refusals[k - 1]
                assert lib.sdrfm_bcast_set_audio(b._h, p(a[0]), p(a[1]), a[2]) == pkg.lib.EINVAL, k
            return act
        acts = {0: _set([ONE, ONE // 2, 0], [ONE, ONE // 4, ONE // 2], 11, ra), **{k: refuse(k) for k in range(1, len(refusals) + 1)}}
        got = _seq(bc, iq, cuts, acts, ra)
        with pytest.raises(pkg.SdrfmError) as e:
            bc.set_audio(blend=[0, 40000, 0])
        assert e.value.status == pkg.lib.EINVAL
        with pytest.raises(pkg.SdrfmError) as e:
            bc.set_audio(gain=1.5)
        assert e.value.status == pkg.lib.EINVAL
        ra.check(bc.audio_state())
        assert bc.kernel_name.endswith(" blend")
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert len(np.unique(got[4][1])) > 100


# ---- 7. device pointers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_device_pointer_form_between_canaries_on_the_callers_stream(pkg, generic):
    """output rows that start 4 bytes past a 16-byte boundary with a row pitch that is no multiple of 16 bytes, canaries before, between
    and behind them, the input 32 bytes into its buffer; every call enqueued on a stream of the caller's"""
    import torch
    shape, ns, iq, tune = _inputs(pkg, "default", True)
    cuts = [2 * 12001, 0, tc.NBYTES - 2 * 12001]
    tb, tg = np.array([0, ONE // 2, ONE // 7], np.uint16), np.array([ONE // 3, ONE, 0], np.uint16)
    with _mk(pkg, shape, ns, generic) as bc:
        bc.tune(**tune)
        ref = ar.AudioState(ns)
        want = _seq(bc, iq, cuts, {0: _set(tb, tg, 30, ref)}, ref)
        na, nr = want[0].shape[1], want[2].shape[1]
        pitch = na + 7 + (0 if (na + 7) % 4 else 1)                 # floats: never a multiple of 16 bytes
        d_iq = torch.full((ns, tc.NBYTES + 64), 0xA5, dtype=torch.uint8, device="cuda")
        d_iq[:, 32:32 + tc.NBYTES] = torch.from_numpy(iq.copy()).cuda()
        d_l = torch.full((ns * pitch + 1,), -7.0, dtype=torch.float32, device="cuda")
        d_r = torch.full((ns * pitch + 1,), -7.0, dtype=torch.float32, device="cuda")
        d_w = torch.full((ns, 2 * nr + 6), -7.0, dtype=torch.float32, device="cuda")
        d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
        vl, vr = d_l[1:].view(ns, pitch), d_r[1:].view(ns, pitch)
        assert vl.data_ptr() % 16 == 4 and (4 * pitch) % 16 != 0
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        bc.tune(**tune)
        bc.clear_audio()
        bc.set_stream(stream.cuda_stream)
        ref = ar.AudioState(ns)
        _set(tb, tg, 30, ref)(bc)
        pos, oa, ow, pct = 0, 0, 0, 0
        for c in cuts:
            a, w_ = bc.process_batch_device(d_iq[:, 32 + pos:32 + pos + c], vl[:, oa:], vr[:, oa:], d_w[:, ow:], d_pc, nbytes=c)
            stream.synchronize()
            pct = pct + d_pc.cpu().numpy().astype(np.int64) if c else pct
            pos, oa, ow = pos + c, oa + a, ow + 2 * w_
            ref.call(a)
            ref.check(bc.audio_state())
        bc.set_stream(None)
        assert (oa, ow) == (na, 2 * nr)
        assert _same(vl[:, :na].cpu().numpy(), want[0]) and _same(vr[:, :na].cpu().numpy(), want[1])
        assert _same(d_w[:, :2 * nr].cpu().numpy(), np.ascontiguousarray(want[2]).view(np.float32))
        assert np.array_equal(pct, want[3])
        assert (vl[:, na:] == -7.0).all() and (vr[:, na:] == -7.0).all() and (d_w[:, 2 * nr:] == -7.0).all() and d_l[0] == -7.0 and d_r[0] == -7.0
        assert (d_iq[:, :32] == 0xA5).all() and (d_iq[:, 32 + tc.NBYTES:] == 0xA5).all()
