"""The long run behind a set: the outputs-since-the-set count J through its saturation at 65536 and n * slew through
2^32 on the device, which no other test reaches — audio_ctl_ramp clamps n at 65536 because n * slew leaves 32 bits at n = 131072 with slew
32768, and a kernel without the clamp would be back at the ramp's start 2.7 s into a call at 48 kHz (at a jump's slew for the one output
whose product is 0 mod 2^32, at smaller slews for as long as the wrapped product stays below the ramp's distance).

  broadcast handle   shape (1, 1, 1, 1, 1, 1, 1) — one audio output per two bytes —, two streams, untuned and tuned to (h, 0) (the shape has
                     generic kernels alone), plain and metered: one call of 140 000 outputs at slew 32768 and at 32767, calls of 60 000,
                     10 000 and 70 001 outputs at slew 1 (J passes 65536 inside the second, J + j + 1 passes 131072 inside the third) and
                     a set to new targets at slew 3 behind them, which rebases from the saturated count.  Exact: blend 0, the gain moving,
                     L = R = mu_j am with am a diff_gain = 0 handle's L.  Once with both at work, at §4.16's derived tolerance.
  stereo sink        exact and default form, 2 x 140 000 samples, 75 us, slews 32768, 32767 and 1, 1024 -> 32768 and 32768 -> 1024, as one
                     call and as calls of 60 000, 10 000 and 70 000: the exact form bit for bit the host routine and, beyond sample
                     32768, bit for bit the host routine given a flat (ht, ht) from the state carried there — a comparison that does not
                     go through the shared header's count; the default form within the sink's three caps of the exact form.
audio_state() and hicut_state() are held to their references after every call."""
import numpy as np
import pytest

import audio_ref as ar
import hicut_ref as hr
import pcm_params as pp
from test_bcast_audio_gpu import _set
from test_bcast_tuned_gpu import _same
from test_pcm_hicut_gpu import GAIN, _bits, _caps, _start, emu

pytestmark = pytest.mark.gpu

ONE = ar.ONE
NS, N, MORE = 2, 140001, 20000                                  # streams; samples (= d's = audio outputs) a stream of the run, and behind it
BT, VT = 12345, 23456
CUTS = (60000, 10000, 70001)
WRAP = 131072                                                   # n * 32768 leaves 32 bits here
PILOT = np.array([0.6 + 0.8j], np.complex64)                    # one pilot tap with both parts: c = -2 qr qi / pw = -0.96, so as = -0.96 dg am
FLAT = 32768                                                    # the sink's ramps have ended by this sample at every slew tested

_rows = []


def _iq(pkg):
    """two FM rows, made once"""
    if not _rows:
        iq = pkg.make_iq(NS, N + MORE, mode="fm", first_id=8300)
        iq.setflags(write=False)
        _rows.append(iq)
    return _rows[0]


def _handle(pkg, diff_gain, tuned):
    """shape (1, 1, 1, 1, 1, 1, 1): unit channel, audio and RDS taps, one pilot tap; untuned, or tuned to (h, 0) and rot 0"""
    one = np.ones(1, np.float32)
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=one, audio_coeffs=one, rds_coeffs=one, pilot_coeffs=PILOT, pilot_min=1e-3, diff_gain=diff_gain,
                                                rds_gain=1.0, fir_decim=1, audio_decim=1, rds_decim=1, n_streams=NS, max_bytes_per_call=2 * (N + MORE),
                                                force_generic=True))
    if tuned:
        bc.tune(ctaps=np.tile(np.array([1.0, 0.0], np.float32), (NS, 1)), rot=np.zeros(NS, np.float32))
    assert bc.kernel_name == "bcast-generic%s T1 D1 P1 Ta1 Da1 Tr1 Dr1" % ("-tuned" if tuned else ""), bc.kernel_name
    return bc


def _prepare(bc, blend0):
    """whatever the handle's conditioning was: the streams from their first byte, blend at blend0 and gain at 1, every ramp complete"""
    bc.clear_audio()
    ref = ar.AudioState(NS)
    _set(blend0, ONE, ONE, ref)(bc)
    bc.reset()
    ref.complete()
    ref.check(bc.audio_state())
    return ref


def _run(bc, iq, cuts, ref, metered=False, start=0):
    """the calls one after the other from sample `start`: (L, R, bb, b, v), audio_state held to the reference after each"""
    parts, pos, bs, vs = ([], [], []), start, [], []
    for c in cuts:
        out = bc.process_batch_metered(iq[:, 2 * pos:2 * (pos + c)]) if metered else bc.process_batch(iq[:, 2 * pos:2 * (pos + c)])
        assert out[0].shape == out[1].shape == (NS, c) and out[2].shape == (NS, c)
        for acc, x in zip(parts, out[:3]):
            acc.append(x)
        pos += c
        b, v = ref.call(c)
        bs.append(b)
        vs.append(v)
        ref.check(bc.audio_state())
    return tuple(np.concatenate(p, 1) for p in parts) + (np.concatenate(bs, 1), np.concatenate(vs, 1))


def _exact(got, am, where, start=0):
    """blend 0: L = R = mu_j am with one rounding, bb the mono handle's"""
    mu = (got[4].astype(np.float64) / ONE).astype(np.float32)
    sl = slice(start, start + got[0].shape[1])
    assert not got[3].any() and np.array_equal(got[0], mu * am[0][:, sl]) and np.array_equal(got[1], mu * am[0][:, sl]), where
    assert _same(got[2], am[2][:, sl]), where


@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "tuned"])
def test_broadcast_gain_ramp_through_the_saturated_count_is_exact(pkg, tuned):
    iq = _iq(pkg)
    with _handle(pkg, 1.0, tuned) as bc, _handle(pkg, 0.0, tuned) as mono:
        am = mono.process_batch(iq)
        name = bc.kernel_name
        assert am[0].shape == (NS, N + MORE) and am[0][:, WRAP - 1].any()      # there is audio at the one output where a wrap would show
        # (a), (b): one call of 140 000 outputs, plain and metered; n * slew passes 2^32 at n = 131072 (slew 32768) and n = 131077 (32767)
        for slew in (ONE, ONE - 1):
            assert (WRAP - 1) * slew < 2 ** 32 <= (WRAP + 5) * slew
            for metered in (False, True):
                ref = _prepare(bc, 0)
                _set(None, VT, slew, ref)(bc)
                assert bc.kernel_name == name + " blend"
                got = _run(bc, iq, (N - 1,), ref, metered)
                assert (got[4] == VT).all() and ref.J == ar.J_MAX
                _exact(got, am, (name, slew, metered))
        # (c) slew 1 over three calls: J passes 65536 inside the second, J + j + 1 passes 131072 inside the third
        ref = _prepare(bc, 0)
        _set(None, VT, 1, ref)(bc)
        got = _run(bc, iq, CUTS, ref)
        assert CUTS[0] < ar.J_MAX < CUTS[0] + CUTS[1] < WRAP < sum(CUTS) == N and ref.J == ar.J_MAX
        assert got[4][0, ONE - VT - 2] == VT + 1 and (got[4][:, ONE - VT - 1:] == VT).all()
        _exact(got, am, (name, "slew 1"))
        # (d) a set behind them, the streams running on: the rebase starts from the saturated count
        _set(None, [3210, ONE], 3, ref)(bc)
        assert ref.J == 0 and list(ref.v0) == [VT, VT]
        more = _run(bc, iq, (MORE // 2, MORE // 2), ref, start=N)
        assert list(more[4][:, 0]) == [VT - 3, VT + 3] and list(more[4][:, -1]) == [3210, ONE] and len(np.unique(more[4][0])) > 6000
        _exact(more, am, (name, "slew 3 behind the saturated count"), start=N)
    print("%s: L = R = mu_j am exactly over 140 000 outputs at slews 32768 and 32767 (plain and metered), over calls of %s at slew 1, and "
          "over %d outputs behind a set from the saturated count" % (name, CUTS, MORE))


@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "tuned"])
def test_broadcast_blend_and_gain_through_the_saturated_count_at_the_derived_tolerance(pkg, tuned):
    """(blend, gain) -> (12345, 23456), no power of two, at slew 32768 over one call of 140 000 outputs, and at slew 1 over the three calls.
    Expected mu_j (am +- beta_j as) in float64 with am the diff_gain = 0 handle's L and as = (L - R) / 2 of the plain handle, tolerance 4 *
    2^-23 (|am| + |as|) per output (tests/test_bcast_audio_gpu.py derives it).  The same comparison against the ramps' START values — what
    output 131071 would carry if n * slew left 32 bits — must fail from that output on: it can tell the two apart there."""
    iq = _iq(pkg)[:, :2 * N]
    with _handle(pkg, 1.0, tuned) as bc, _handle(pkg, 0.0, tuned) as mono, _handle(pkg, 1.0, tuned) as plain:
        am = mono.process_batch(iq)[0].astype(np.float64)
        full = plain.process_batch(iq)
        as_ = (full[0].astype(np.float64) - full[1].astype(np.float64)) / 2
        assert float(np.abs(as_[:, WRAP:]).max()) > 0.01
        tol = 4 * 2.0 ** -23 * (np.abs(am) + np.abs(as_))
        for slew, cuts in ((ONE, (N - 1,)), (1, CUTS)):
            ref = _prepare(bc, ONE)
            _set(BT, VT, slew, ref)(bc)
            got = _run(bc, iq, cuts, ref)
            n = got[0].shape[1]
            assert _same(got[2], full[2][:, :n]) and (got[3][:, -1] == BT).all() and (got[4][:, -1] == VT).all()

            def errors(b, v):
                beta, mu = b / ONE, v / ONE
                return np.maximum(np.abs(got[0] - mu * (am[:, :n] + beta * as_[:, :n])), np.abs(got[1] - mu * (am[:, :n] - beta * as_[:, :n])))
            e = errors(got[3].astype(np.float64), got[4].astype(np.float64))
            print("%s, slew %d: worst error / tolerance %.3f over %d outputs a stream" % (bc.kernel_name, slew, float((e / np.maximum(tol[:, :n], 1e-30)).max()), n))
            assert (e <= tol[:, :n]).all()
            snapped = errors(np.float64(ONE), np.float64(ONE))[:, WRAP - 1:] > tol[:, WRAP - 1:n]
            assert snapped.mean() > 0.9, float(snapped.mean())


# ---- the stereo sink -------------------------------------------------------------------------------------------------------------------
def _sink_calls(sink, left, right, cuts, ref):
    parts, at = [], 0
    for c in cuts:
        parts.append(sink.process_batch(left[:, at:at + c], right[:, at:at + c]))
        at += c
        ref.call(c)
        ref.check(sink.hicut_state())
    return np.concatenate(parts, axis=1), sink.state()


@pytest.mark.parametrize("slew", [32768, 32767, 1])
def test_sink_high_cut_through_the_saturated_count(pkg, slew):
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    n = 140000
    left, right = emu.sink_inputs(NS, n // 2)
    h0, ht = emu.hicut_ramps(NS, 1024)                              # stream 0: 1024 -> 32768, stream 1: 32768 -> 1024
    assert left.shape == (NS, n) and hr.ramp(1024, 32768, slew, FLAT) == 32768 and hr.ramp(32768, 1024, slew, FLAT) == 1024
    want, want_st = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, slew, 0)
    # the plateau on its own: the ramping part's state carried, then flat (ht, ht) — the count plays no part in it
    head, st = emu.host_reference(pkg, left[:, :FLAT], right[:, :FLAT], alpha, GAIN, h0, ht, slew, 0)
    flat, flat_st = emu.host_reference(pkg, left[:, FLAT:], right[:, FLAT:], alpha, GAIN, ht, ht, ONE, 0, st)
    assert np.array_equal(head, want[:, :2 * FLAT])
    exact = {}
    for cuts in ((n,), (60000, 10000, 70000)):
        for form in ("exact", "default"):
            with pkg.StereoPcmSink(NS, alpha, GAIN, exact=form == "exact") as sink:
                _start(sink, h0, ht, slew)
                ref = hr.HicutState(NS)
                ref.set(h0, ONE)
                ref.complete()
                ref.set(ht, slew)
                ref.check(sink.hicut_state())
                got, st_dev = _sink_calls(sink, left, right, cuts, ref)
                assert ref.J == hr.J_MAX and np.array_equal(sink.hicut_state()[0], ht)
            if form == "exact":
                assert np.array_equal(got, want) and np.array_equal(_bits(st_dev), _bits(want_st)), (slew, cuts, np.argwhere(got != want)[:4])
                assert np.array_equal(got[:, 2 * FLAT:], flat) and np.array_equal(_bits(st_dev), _bits(flat_st)), (slew, cuts, "the plateau")
                exact[cuts] = (got, st_dev)
            else:
                ok, lsb, share, cap, rel = _caps(got, st_dev, *exact[cuts])
                print("sink, slew %d, calls %s: default form against exact: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" % (
                    slew, cuts, lsb, share, cap, rel))
                assert ok, (slew, cuts, lsb, share, rel)
    print("sink, slew %d: the exact form bit for bit the host routine over %d samples a stream and, from sample %d on, the host routine at a flat "
          "high-cut" % (slew, n, FLAT))
