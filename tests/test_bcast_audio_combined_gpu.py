"""The features of DESIGN.md §4.14 to §4.17 together, as an operator uses them — tune, meter, re-tune, condition, with the PCM sink behind
the handle — on tests/tuned_cases.py's default shape, three streams of 125 000 B, on the fast and on the generic kernels.

  1. a real re-tune in mid-ramp: tests/retune_cases.py's moves (+5 kHz, -7 kHz and across the rot wrap, with the carry) after N0 samples, at
     blend 0 with a gain ramp of slew 9 running.  L = R = mu_j times the L of a diff_gain = 0 handle re-tuned the same way, bitwise; bb and
     pilot_count are that handle's; the re-tune leaves the ramps where they are.
  2. the whole receiver: a tuned handle with both ramps at slew 7 and a StereoPcmSink whose high-cut ramps at slew 7, through a metered call
     with the sink, a PCM call that passes no audio rows, and a second metered call with the sink.  L and R of the metered calls are bitwise
     those of a second conditioned handle without a sink, the records bitwise an unconditioned handle's, the PCM of all three calls within
     1 LSB of the host high-cut routine over the second handle's L and R with state and count carried, the sink's states within 1e-6
     max(|st|, 0.25), and both counts move on across the call that passed no audio rows."""
import numpy as np
import pytest

import audio_ref as ar
import hicut_ref as hr
import pcm_params as pp
import retune_cases as rc
import tuned_cases as tc
from test_bcast_audio_gpu import FIELDS, _mk, _set
from test_bcast_tuned_gpu import _same, _want_name
from test_pcm_hicut_gpu import GAIN, emu
from test_pcm_hicut_gpu import _set as _set_hicut

pytestmark = pytest.mark.gpu

ONE = ar.ONE
CASE = ("default", 3, "signal")


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_a_real_retune_in_mid_ramp(pkg, generic):
    su = rc.case_setup(pkg, CASE)
    shape, ns, iq = su["shape"], su["ns"], su["iq"]
    cuts = [2 * rc.N0, tc.NBYTES - 2 * rc.N0]
    retune = lambda b: b.retune(ctaps=su["new"][0], rot=su["new"][1], carry=su["carry"])
    vt = np.array([ONE // 5, 0, 12345])
    assert rc.DELTAS[:ns] == ("+5k", "-7k", "wrap") and not np.array_equal(su["old"][1], su["new"][1])
    with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic, 0.0) as mono:
        am, parts, bs, vs, pos = [], [], [], [], 0
        for h_ in (bc, mono):
            h_.tune(ctaps=su["old"][0], rot=su["old"][1])
        ref = ar.AudioState(ns)
        _set(0, ONE, ONE, ref)(bc)                                   # blend 0 by a jump; tune and reset complete ramps, a set before the first call
        bc.reset()                                                   # ... needs the reset to be complete
        ref.complete()
        _set(None, vt, 9, ref)(bc)
        for k, c in enumerate(cuts):
            if k == 1:
                before = bc.audio_state()
                retune(bc)
                retune(mono)
                after = bc.audio_state()
                assert all(np.array_equal(before[f], after[f]) for f in before)     # the ramps are untouched ...
                ref.check(after)
                assert (after["gain"] != after["gain_target"]).all() and (after["gain"] < ONE).all()   # ... and in mid-ramp
                assert bc.kernel_name == _want_name(shape, generic, True) + " blend"
            am.append(mono.process_batch(iq[:, pos:pos + c]))
            parts.append(bc.process_batch(iq[:, pos:pos + c]))
            b, v = ref.call(parts[-1][0].shape[1])
            bs.append(b)
            vs.append(v)
            ref.check(bc.audio_state())
            pos += c
    for k in range(2):
        mu = (vs[k].astype(np.float64) / ONE).astype(np.float32)
        assert not bs[k].any()
        assert np.array_equal(parts[k][0], mu * am[k][0]) and np.array_equal(parts[k][1], mu * am[k][0]), (k, "L = R = mu am")
        assert _same(parts[k][2], am[k][2]) and np.array_equal(parts[k][3], am[k][3]), (k, "bb, pilot_count")
    assert len(np.unique(vs[1][0])) == vs[1].shape[1] and int(am[1][3].max()) > 0 and float(np.abs(am[1][0]).max()) > 0.1


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
def test_the_whole_receiver(pkg, generic):
    su = tc.case_setup(pkg, CASE)
    shape, ns, iq = su["shape"], su["ns"], su["iq"]
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    cuts = [2 * 20001, 2 * 19999, tc.NBYTES - 2 * 40000]
    chunks = [iq[:, sum(cuts[:k]):sum(cuts[:k + 1])] for k in range(3)]
    bt, vt = np.array([5000, 12001, 19002]), np.array([29768, 20767, 11766])
    ht = np.array([1024, 8192, 12000])
    with _mk(pkg, shape, ns, generic) as bc, _mk(pkg, shape, ns, generic) as second, _mk(pkg, shape, ns, generic) as plain, \
            pkg.StereoPcmSink(ns, alpha, GAIN) as sink:
        for h_ in (bc, second, plain):
            h_.tune(ctaps=su["ctaps"], rot=su["rot"])
        ref = ar.AudioState(ns)
        _set(bt, vt, 7, ref)(bc)
        _set(bt, vt, 7)(second)
        assert _set_hicut(sink, ht, 7) == 0
        href = hr.HicutState(ns)
        href.set(ht, 7)
        href.check(sink.hicut_state())
        name = _want_name(shape, generic, True)
        assert bc.kernel_name == second.kernel_name == name + " blend" and plain.kernel_name == name
        state, worst = np.zeros((ns, 2), np.float32), 0
        for k, c in enumerate(chunks):
            want = second.process_batch(c)                           # a second conditioned handle without a sink
            if k == 1:
                l, r, pcm, w, pc = bc.process_batch_pcm(sink, c, with_audio=False)
                assert l is None and r is None
                plain.process_batch(c)
            else:
                l, r, pcm, w, pc, m = bc.process_batch_metered(c, sink=sink)
                assert _same(l, want[0]) and _same(r, want[1]), (k, "L, R")
                records = plain.process_batch_metered(c)[4]          # an unconditioned handle's
                for f in FIELDS:
                    assert np.array_equal(m[f], records[f]), (k, f)
                assert int(m["n_pilot"].max()) > 0
            assert _same(w, want[2]) and np.array_equal(pc, want[3]), (k, "bb, pilot_count")
            na = want[0].shape[1]
            a0, at, sl, J = href.call(na)
            assert sl == 7 and J == sum(cuts[:k]) // 2 // shape[1] // shape[4]
            wpcm, state = emu.host_reference(pkg, want[0], want[1], alpha, GAIN, a0, at, sl, J, state)
            d = np.abs(pcm.astype(np.int32) - wpcm.astype(np.int32))
            worst = max(worst, int(d.max()))
            assert pcm.shape == wpcm.shape and d.max() <= 1, (k, int(d.max()), np.argwhere(d > 1)[:4])
            bc.synchronize()
            b, v = ref.call(na)                                      # both counts moved on by this call's outputs, audio rows passed or not
            ref.check(bc.audio_state())
            href.check(sink.hicut_state())
            assert (b[:, -1] != bt).all() and (href.now() != ht).all() and int(np.abs(wpcm).max()) > 1000      # every ramp still running
        st = sink.state()
    rel = float(np.max(np.abs(st - state) / np.maximum(np.abs(state), 0.25)))
    print("%s with a conditioned sink, metered / PCM without audio rows / metered: worst PCM %d LSB, state %.3g relative" % (name + " blend", worst, rel))
    assert np.all(np.abs(st - state) <= 1e-6 * np.maximum(np.abs(state), 0.25)), (st, state)
