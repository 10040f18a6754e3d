"""The stereo PCM sink's ramped high-cut on the device (csrc/sdrfm_sink_hicut.h, csrc/sdrfm_sink_stereo.hip; include/sdrfm.h) against
the host routine sdrfm_pcm_deemph_stereo_hicut_s16, which tests/test_hicut_cpu.py holds to the definition bit for bit.

  exact form     bit for bit the host routine, PCM and states, on every shape of tests/test_pcm_sink_params_gpu.py, every stream with its own (h0, ht),
                 at the four slews, at 50 us, 75 us, alpha = 1 and alpha = 0.05; 32768 everywhere is a never-conditioned sink; the host routine one
                 sample further along the ramp is NOT what the device gives.
  default form   within the sink's three caps (1 LSB; a share of differing outputs <= 1e-3 + 2 / size; states within 1e-6 max(|st|, 0.25)) of the exact
                 form at 50 us and 75 us over the ramps tests/test_pcm_hicut_scan_cpu.py shows to hold by the arithmetic alone.
  cuts, state, the corner, the one-call forms, the device-pointer form: below.
The inputs are tools/pcm_stereo_scan_emulate.py's sink_inputs, two calls per shape.  Every test prints its worst figures (pytest -s)."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

import hicut_ref as hr
import pcm_params as pp
import test_pcm_stereo_sink_gpu as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_hicut_scan_emulate")

SHAPES = [(1, 19), (3, 20), (63, 4864), (65, 4865), (2, 9729)]
SLEWS = (1, 7, 40, 32768)
VALUES = (1024, 1025, 8192, 32767, 32768)
# every stream its own (h0, ht): the ramping pairs first (a shape of one stream ramps), then the flat ones
PAIRS = [(a, b) for a in VALUES for b in VALUES if a != b] + [(a, a) for a in VALUES]
GAIN = pp.DEFAULT_GAIN


def _pkg():
    return importlib.import_module("stm32f7-rtlsdr_amd")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pairs(ns, shift=0):
    p = [PAIRS[(s + shift) % len(PAIRS)] for s in range(ns)]
    return np.array([a for a, _ in p], np.int64), np.array([b for _, b in p], np.int64)


@functools.lru_cache(maxsize=None)
def _inputs(ns, n):
    x = emu.sink_inputs(ns, n)
    for a in x:
        a.setflags(write=False)
    return x


def _set(sink, hicut, slew):
    """sdrfm_pcm_stereo_sink_set_hicut with the slew as it is (StereoPcmSink.set_hicut takes a ramp time): the status"""
    q = None if hicut is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hicut), (sink.n_streams,)), dtype=np.uint16)
    return int(sink._lib.sdrfm_pcm_stereo_sink_set_hicut(sink._h, q.ctypes.data if q is not None else None, int(slew)))


def _start(sink, h0, ht, slew):
    """the sink's ramps at (h0 -> ht, slew, J = 0) and its states zero: a jump to h0, completed by reset, then the set"""
    assert _set(sink, h0, 32768) == 0
    sink.reset()
    assert _set(sink, ht, slew) == 0


def _calls(sink, left, right, cuts):
    parts, at = [], 0
    for c in cuts:
        parts.append(sink.process_batch(left[:, at:at + c], right[:, at:at + c]))
        at += c
    return np.concatenate(parts, axis=1), sink.state()


@functools.lru_cache(maxsize=None)
def _exact(aname, ns, n, lo, slew):
    """the exact form's PCM and states under the default form's ramps, two calls, computed once: the reference of the default form (never modified)"""
    pkg = _pkg()
    alpha = pp.alpha_of(pkg.load_library(), aname)
    left, right = _inputs(ns, n)
    h0, ht = emu.hicut_ramps(ns, lo)
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
        _start(sink, h0, ht, slew)
        pcm, st = _calls(sink, left, right, (n, n))
    pcm.setflags(write=False)
    st.setflags(write=False)
    return pcm, st


def _caps(a, sa, b, sb):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    rel = float(np.max(np.abs(sa - sb) / np.maximum(np.abs(sb), 0.25)))
    share, cap = float((d != 0).mean()), 1e-3 + 2.0 / d.size
    ok = d.max() <= 1 and share <= cap and bool(np.all(np.abs(sa - sb) <= 1e-6 * np.maximum(np.abs(sb), 0.25)))
    return ok, int(d.max()), share, cap, rel


# ---- the exact form ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slew", SLEWS)
@pytest.mark.parametrize("aname", ["50us", "75us", "1", "0.05"])
def test_exact_form_is_the_host_routine_bit_for_bit(pkg, aname, slew):
    alpha = pp.alpha_of(pkg.load_library(), aname)
    for ns, n in SHAPES:
        left, right = _inputs(ns, n)
        h0, ht = _pairs(ns, shift=slew % 7)
        with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
            _start(sink, h0, ht, slew)
            got, st_dev = _calls(sink, left, right, (n, n))
        want, st = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, slew, 0)
        assert np.array_equal(got, want), (ns, n, np.argwhere(got != want)[:4])
        assert np.array_equal(_bits(st_dev), _bits(st)), (ns, n, st_dev, st)
    print("exact, alpha %s = %.9g, slew %d: PCM and states equal the host routine's bit for bit at %s" % (aname, alpha, slew, SHAPES))


def test_a_sink_set_to_32768_everywhere_is_a_never_conditioned_exact_sink(pkg):
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    for ns, n in SHAPES:
        left, right = _inputs(ns, n)
        with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as plain:
            want, want_st = _calls(plain, left, right, (n, n))
            assert plain.hicut_state()[2] == 0
        with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
            assert _set(sink, 32768, 7) == 0
            assert sink.hicut_state()[2] == 7                                              # conditioned: the conditioned kernel runs
            got, st = _calls(sink, left, right, (n, n))
        assert np.array_equal(got, want) and np.array_equal(_bits(st), _bits(want_st)), (ns, n)


def test_the_comparison_sees_a_ramp_one_sample_off(pkg):
    """the exact form against the host routine given J + 1: must differ on a ramping stream — the bit-for-bit tests above can tell"""
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    ns, n = 3, 20
    left, right = _inputs(ns, n)
    h0, ht = np.array([1024, 32768, 8192]), np.array([32768, 1024, 8192])
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
        _start(sink, h0, ht, 40)
        got, _ = _calls(sink, left, right, (n, n))
    same, _ = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, 40, 0)
    off, _ = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, 40, 1)
    assert np.array_equal(got, same)
    share = (got != off).mean(axis=1)
    print("against the host routine at J + 1: share of differing outputs per stream %s (stream 2 is flat)" % np.round(share, 3))
    assert share[0] > 0 and share[1] > 0 and share[2] == 0


# ---- the default form ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,slew", emu.RAMPS, ids=["%d-slew%d" % r for r in emu.RAMPS])
@pytest.mark.parametrize("aname", ["50us", "75us"])
def test_default_form_within_the_three_caps_of_the_exact_form(pkg, aname, lo, slew):
    alpha = pp.alpha_of(pkg.load_library(), aname)
    worst, fails = [0, 0.0, 0.0], []
    for ns, n in SHAPES:
        left, right = _inputs(ns, n)
        h0, ht = emu.hicut_ramps(ns, lo)
        with pkg.StereoPcmSink(ns, alpha, GAIN) as sink:
            _start(sink, h0, ht, slew)
            a, sa = _calls(sink, left, right, (n, n))
        b, sb = _exact(aname, ns, n, lo, slew)
        ok, lsb, share, cap, rel = _caps(a, sa, b, sb)
        print("default, %s, %d <-> 32768 at slew %d, %d x %d: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" % (
            aname, lo, slew, ns, n, lsb, share, cap, rel))
        worst = [max(worst[0], lsb), max(worst[1], share), max(worst[2], rel)]
        if not ok:
            fails.append((ns, n, lsb, share, rel))
    print("default, %s, %d <-> 32768 at slew %d: worst PCM %d LSB, share %.3g, state %.3g relative" % (aname, lo, slew, worst[0], worst[1], worst[2]))
    assert not fails, fails


# ---- cuts ----------------------------------------------------------------------------------------------------------------------------------------------
CUTS = [(0, 1, 18, 19, 20, 4865), (4865, 20, 19, 18, 1, 0)]


@pytest.mark.parametrize("slew", [1, 7])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_any_cut_into_calls(pkg, exact, slew):
    """ramps running (slew 1: throughout; slew 7: the ramp ends inside the 4865-sample call): the exact form gives the bits of the one call, the
    default form stays within the caps of the exact form's one call"""
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    ns, n = 3, sum(CUTS[0])
    left, right = (a[:, :n] for a in _inputs(3, 4865))
    h0, ht = emu.hicut_ramps(ns, 1024)
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
        _start(sink, h0, ht, slew)
        one, one_st = _calls(sink, left, right, (n,))
    want, want_st = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, slew, 0)
    assert np.array_equal(one, want) and np.array_equal(_bits(one_st), _bits(want_st))
    for cuts in CUTS:
        with pkg.StereoPcmSink(ns, alpha, GAIN, exact=exact) as sink:
            _start(sink, h0, ht, slew)
            got, st = _calls(sink, left, right, cuts)
            assert np.array_equal(sink.hicut_state()[0], [hr.ramp(h0[s], ht[s], slew, n) for s in range(ns)])
        if exact:
            assert np.array_equal(got, one) and np.array_equal(_bits(st), _bits(one_st)), cuts
        else:
            ok, lsb, share, cap, rel = _caps(got, st, one, one_st)
            print("default, cuts %s, slew %d: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" % (cuts, slew, lsb, share, cap, rel))
            assert ok, (cuts, lsb, share, rel)


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------------
def test_get_hicut_follows_every_set_and_every_call(pkg):
    alpha = pp.alpha_of(pkg.load_library(), "50us")
    ns = 3
    left, right = _inputs(ns, 4865)
    ref = hr.HicutState(ns)
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
        ref.check(sink.hicut_state())
        state = np.zeros((ns, 2), np.float32)
        at = 0
        for hicut, slew, count in [([1024, 8192, 32768], 7, 300), (None, 40, 19), ([32768, 32768, 1024], 40, 500), ([2048, 2048, 2048], 32768, 1),
                                   ([32768, 1024, 4096], 1, 700)]:
            assert _set(sink, hicut, slew) == 0
            ref.set(hicut, slew)
            ref.check(sink.hicut_state())
            for c in (count, 0, 20):
                h0, ht, sl, J = ref.call(c)
                got = sink.process_batch(left[:, at:at + c], right[:, at:at + c])
                want, state = emu.host_reference(pkg, left[:, at:at + c], right[:, at:at + c], alpha, GAIN, h0, ht, sl, J, state)
                assert np.array_equal(got, want), (hicut, slew, c)
                ref.check(sink.hicut_state())
                at += c
        assert np.array_equal(_bits(sink.state()), _bits(state))
        assert not np.array_equal(ref.now(), ref.ht)                                       # the last ramps are still running ...
        sink.reset()                                                                       # ... and reset completes them, the settings kept
        ref.complete()
        ref.check(sink.hicut_state())
        assert np.array_equal(sink.hicut_state()[0], [32768, 1024, 4096]) and sink.hicut_state()[2] == 1 and not sink.state().any()
        got = sink.process_batch(left[:, :300], right[:, :300])
        want, _ = emu.host_reference(pkg, left[:, :300], right[:, :300], alpha, GAIN, ref.ht, ref.ht, 1, 0)
        assert np.array_equal(got, want)
        # the Python mirror: floats, one value for all, a ramp time
        assert sink.set_hicut(0.25, ramp_ms=50.0) == 14
        assert np.array_equal(sink.hicut_state()[1], [8192] * 3) and sink.hicut_state()[2] == 14
        sink.clear_hicut()
        ref.set(None, 0)
        ref.check(sink.hicut_state())


def test_a_set_in_mid_ramp_gives_the_same_bits_for_two_cuts_round_it(pkg):
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    ns = 3
    left, right = _inputs(ns, 4865)
    outs = []
    for exact in (True, False):
        for cuts_a, cuts_b in (((150, 150), (400,)), ((299, 1), (1, 399))):
            with pkg.StereoPcmSink(ns, alpha, GAIN, exact=exact) as sink:
                _start(sink, [32768, 1024, 8192], [1024, 32768, 8192], 40)                 # 794 samples to the end: 300 in, the ramps are half way
                a, _ = _calls(sink, left[:, :300], right[:, :300], cuts_a)
                mid = sink.hicut_state()[0].copy()
                assert _set(sink, [32768, 32768, 1024], 7) == 0                            # new targets from where the ramps stand
                assert np.array_equal(sink.hicut_state()[0], mid) and list(mid) == [32768 - 12000, 1024 + 12000, 8192]
                b, st = _calls(sink, left[:, 300:700], right[:, 300:700], cuts_b)
            outs.append((np.concatenate([a, b], axis=1), st))
        if exact:
            assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
            first, st0 = emu.host_reference(pkg, left[:, :300], right[:, :300], alpha, GAIN, [32768, 1024, 8192], [1024, 32768, 8192], 40, 0)
            second, st1 = emu.host_reference(pkg, left[:, 300:700], right[:, 300:700], alpha, GAIN, mid, [32768, 32768, 1024], 7, 0, st0)
            assert np.array_equal(outs[0][0], np.concatenate([first, second], axis=1)) and np.array_equal(_bits(outs[0][1]), _bits(st1))
    for k in (2, 3):                                                                       # the default form: each cut within the caps of the exact form
        ok, lsb, share, cap, rel = _caps(outs[k][0], outs[k][1], outs[0][0], outs[0][1])
        assert ok, (k, lsb, share, rel)


def test_clear_hicut_gives_back_the_default_forms_bits(pkg):
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    ns, n = 65, 4865
    left, right = _inputs(ns, n)
    with pkg.StereoPcmSink(ns, alpha, GAIN) as plain:
        want, want_st = _calls(plain, left, right, (n, n))
    with pkg.StereoPcmSink(ns, alpha, GAIN) as sink:
        _start(sink, 2048, 4096, 7)
        cond = sink.process_batch(left[:, :n], right[:, :n])
        assert not np.array_equal(cond, want[:, :2 * n])
        sink.clear_hicut()
        assert sink.hicut_state()[2] == 0 and (sink.hicut_state()[0] == 32768).all() and (sink.hicut_state()[1] == 32768).all()
        sink.reset()
        got, st = _calls(sink, left, right, (n, n))
    assert np.array_equal(got, want) and np.array_equal(_bits(st), _bits(want_st))


def test_every_refusal_changes_nothing(pkg):
    lib = pkg.load_library()
    alpha = pp.alpha_of(lib, "50us")
    E = pkg.lib.EINVAL
    ns, n = 3, 20
    left, right = _inputs(ns, n)
    h0, ht = np.array([1024, 32768, 8192]), np.array([32768, 1024, 4096])
    want, want_st = emu.host_reference(pkg, left, right, alpha, GAIN, h0, ht, 40, 0)
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=True) as sink:
        _start(sink, h0, ht, 40)
        a = sink.process_batch(left[:, :n], right[:, :n])
        before = sink.hicut_state()
        ok = np.full(ns, 8192, np.uint16)
        for bad in ([1023, 8192, 8192], [8192, 8192, 32769], [0, 8192, 8192], [8192, 65535, 8192]):
            assert _set(sink, bad, 40) == E, bad                                           # a value outside [1024, 32768]
        assert lib.sdrfm_pcm_stereo_sink_set_hicut(sink._h, ok.ctypes.data, 0) == E        # a slew of 0 with an array
        assert _set(sink, ok, 32769) == E and _set(sink, None, 32769) == E and _set(sink, None, 0xFFFFFFFF) == E
        with pytest.raises(pkg.SdrfmError) as e:
            sink.set_hicut(0.01)                                                           # below 1/32, through the Python mirror
        assert e.value.status == E
        with pytest.raises(pkg.SdrfmError) as e:
            sink.set_hicut(3.0)
        assert e.value.status == E
        after = sink.hicut_state()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2] == 40
        assert lib.sdrfm_pcm_stereo_sink_get_hicut(sink._h, None, None, None) == 0          # any pointer may be NULL
        b = sink.process_batch(left[:, n:], right[:, n:])
        assert np.array_equal(np.concatenate([a, b], axis=1), want) and np.array_equal(_bits(sink.state()), _bits(want_st))
    # a sink whose smallest effective coefficient would fall below 0.001 is refused and stays a plain sink; 0.032 is taken
    x = _inputs(1, 19)
    small = float(np.float32(0.03))
    assert np.float32(small) * np.float32(0.03125) < np.float32(0.001) <= np.float32(0.032) * np.float32(0.03125)
    with pkg.StereoPcmSink(1, small, GAIN, exact=True) as sink, pkg.StereoPcmSink(1, small, GAIN, exact=True) as plain:
        assert _set(sink, 8192, 40) == E and _set(sink, None, 40) == E
        assert sink.hicut_state()[2] == 0
        sink.clear_hicut()                                                                 # (returning to the plain kernels is always possible)
        assert np.array_equal(sink.process_batch(x[0][:, :19], x[1][:, :19]), plain.process_batch(x[0][:, :19], x[1][:, :19]))
    with pkg.StereoPcmSink(1, 0.032, GAIN, exact=True) as sink:
        assert _set(sink, 1024, 40) == 0


# ---- the corner ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_corner_of_a_settled_stream(pkg):
    """A 400 Hz and an 8 kHz tone of 1 rad through h = 8192 and h = 32768 (jumps; the exact form, so the PCM is the definition's), 4800 samples; the
    amplitudes fitted over the last 2400 (whole periods of both tones: sine, cosine and DC are orthogonal there).  One-pole response in float64 with the
    fp32 coefficient the definition uses: |H| = a / sqrt(1 - 2 (1 - a) cos w + (1 - a)^2).
    Margin.  The start-up transient is (1 - a)^2400 <= e^-145: nothing.  A PCM sample differs from the ideal response by at most 0.5 LSB of rounding
    plus the fp32 arithmetic's error: a step rounds its difference and its fma, 2^-24 (a |x - y| + |y|) together, and the recursion sums those with
    weights (1 - a)^k, so at most 2^-24 |y| / a (1 + a) in y, with |y| <= 1 rad and a >= 0.06 that is 0.017 LSB after the gain; the tone's own fp32
    rounding and that of y * gain add 0.001 each: e <= 0.52.  The fitted (sine, cosine) pair is the projection of the samples on two orthogonal columns
    of norm sqrt(N / 2), so an error vector of norm <= e sqrt(N) moves the fitted amplitude by at most e sqrt(2) = 0.74 LSB.  The ratio
    A(8192) / A(32768) of the 8 kHz tone (about 1042 / 4479 LSB) must therefore lie between (A1 - 0.74) / (A2 + 0.74) and (A1 + 0.74) / (A2 - 0.74)
    of the theory: about 8.7e-4 relative."""
    lib = pkg.load_library()
    alpha = float(lib.sdrfm_pcm_alpha(48000.0, 75e-6))
    fs, n, skip = 48000.0, 4800, 2400
    t = np.arange(n, dtype=np.float64) / fs
    tones = [400.0, 400.0, 8000.0, 8000.0]
    hs = np.array([8192, 32768, 8192, 32768])
    left = np.stack([np.sin(2 * np.pi * f * t) for f in tones]).astype(np.float32)
    right = np.ascontiguousarray(-left)
    with pkg.StereoPcmSink(4, alpha, GAIN, exact=True) as sink:
        assert _set(sink, hs, 32768) == 0
        pcm = sink.process_batch(left, right)
    assert np.array_equal(pcm[:, 0::2][:, skip:], -pcm[:, 1::2][:, skip:])                 # R = -L: the channels share the coefficient
    amp, theory = np.zeros(4), np.zeros(4)
    for s in range(4):
        w = 2 * np.pi * tones[s] / fs
        cols = np.stack([np.ones(n - skip), np.sin(w * np.arange(skip, n)), np.cos(w * np.arange(skip, n))], 1)
        coef, *_ = np.linalg.lstsq(cols, pcm[s, 0::2][skip:].astype(np.float64), rcond=None)
        amp[s] = np.hypot(coef[1], coef[2])
        a = float(hr.alphas(alpha, hs[s]))
        theory[s] = float(np.float32(GAIN)) * a / np.sqrt(1.0 - 2.0 * (1.0 - a) * np.cos(w) + (1.0 - a) ** 2)
    d = 0.52 * np.sqrt(2.0)
    print("fitted amplitudes (LSB) %s, one-pole theory %s; corners %.0f and %.0f Hz" % (
        np.round(amp, 2), np.round(theory, 2), float(pkg.hicut_corner_hz(alpha, 8192, fs)), float(pkg.hicut_corner_hz(alpha, 32768, fs))))
    assert np.all(np.abs(amp - theory) <= d), (amp, theory)
    for lo_, hi_ in ((2, 3), (0, 1)):                                                      # 8 kHz, then 400 Hz
        ratio = amp[lo_] / amp[hi_]
        assert (theory[lo_] - d) / (theory[hi_] + d) <= ratio <= (theory[lo_] + d) / (theory[hi_] - d), (ratio, theory[lo_] / theory[hi_])
    # what the high-cut is for: the 8 kHz tone loses more than 12 dB against the plain de-emphasis, the 400 Hz tone less than 3.5 dB
    assert 20 * np.log10(amp[2] / amp[3]) < -12.0 and 20 * np.log10(amp[0] / amp[1]) > -3.5


# ---- the one-call forms --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(kind):
    """a separate plain handle's calls over the stations of tests/test_pcm_stereo_sink_gpu.py: computed once"""
    pkg = _pkg()
    with sg._handle(pkg, "stereo" if kind == "stereo" else "bcast", False) as ref:
        if kind == "metered":
            return tuple(ref.process_batch_metered(sg._chunk(k)) for k in range(sg.NCALLS))
        return tuple(ref.process_batch(sg._chunk(k)) for k in range(sg.NCALLS))


@pytest.mark.parametrize("kind", ["stereo", "bcast", "metered"])
def test_one_call_forms_with_a_conditioned_sink(pkg, kind):
    """4 streams x 3 calls: L, R (bb, pilot_count, the records) bit for bit a separate plain handle's; the PCM within 1 LSB of the host high-cut routine
    over THAT handle's L and R with the states and the count carried; the states within the cap.  The ramps (slew 7 from 32768 down to four targets)
    run through all three calls, so a count that did not advance with the launch behind the handle's call would show."""
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    plain = _plain(kind)
    na = plain[0][0].shape[1]
    ht = np.array([1024, 8192, 32768, 12000])
    h0 = np.full(sg.NS, 32768)
    want, J = [], 0
    state = np.zeros((sg.NS, 2), np.float32)
    for k in range(sg.NCALLS):
        w, state = emu.host_reference(pkg, plain[k][0], plain[k][1], alpha, GAIN, h0, ht, 7, J, state)
        want.append(w)
        J = min(J + na, 65536)
    assert hr.ramp(32768, 1024, 7, (sg.NCALLS - 1) * na) != 1024 and max(int(np.abs(w).max()) for w in want) > 1000
    worst = 0
    with sg._handle(pkg, "stereo" if kind == "stereo" else "bcast", False) as dm, pkg.StereoPcmSink(sg.NS, alpha, GAIN) as sink:
        assert _set(sink, ht, 7) == 0
        for k in range(sg.NCALLS):
            r = dm.process_batch_metered(sg._chunk(k), sink=sink) if kind == "metered" else dm.process_batch_pcm(sink, sg._chunk(k))
            rest = r[:2] + r[3:]                                                           # the plain call's tuple
            assert len(rest) == len(plain[k])
            for got, ref in zip(rest, plain[k]):
                if ref.dtype.names:
                    assert got.tobytes() == ref.tobytes(), (kind, k)
                else:
                    g, w = (a.view(np.float32) if a.dtype == np.complex64 else a for a in (got, ref))
                    assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (kind, k)
            d = np.abs(r[2].astype(np.int32) - want[k].astype(np.int32))
            worst = max(worst, int(d.max()))
            assert d.max() <= 1, (kind, k, int(d.max()), np.argwhere(d > 1)[:4])
            dm.synchronize()
            assert np.array_equal(sink.hicut_state()[0], [hr.ramp(32768, ht[s], 7, (k + 1) * na) for s in range(sg.NS)]), k
        st = sink.state()
    rel = float(np.max(np.abs(st - state) / np.maximum(np.abs(state), 0.25)))
    print("%s one call with a conditioned sink: worst PCM %d LSB, state %.3g relative" % (kind, worst, rel))
    assert np.all(np.abs(st - state) <= 1e-6 * np.maximum(np.abs(state), 0.25)), (st, state)


# ---- the device-pointer form ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "default"])
def test_device_pointer_form_on_odd_rows_with_canaries(pkg, exact):
    """rows 4 bytes past a 16-byte boundary, at a pitch that is no multiple of 16 bytes, canaries before, between and behind the PCM rows, on the
    caller's stream; two calls"""
    import torch
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    ns, n = 65, 4865
    astride, pstride = n + 2, 2 * n + 4
    assert (4 * astride) % 16 and (2 * pstride) % 16 and pstride % 2 == 0
    left, right = _inputs(ns, n)
    h0, ht = emu.hicut_ramps(ns, 2048)
    want, want_st = _exact("75us", ns, n, 2048, 7)
    stream = torch.cuda.Stream()
    flat = {k: [torch.zeros(ns * astride + 8, dtype=torch.float32, device="cuda") for _ in range(2)] for k in ("l", "r")}
    pflat = [torch.full((ns * pstride + 16,), 12345, dtype=torch.int16, device="cuda") for _ in range(2)]
    rows = lambda f: f[1:1 + ns * astride].view(ns, astride)                               # 256-byte aligned allocations: element 1 is 4 bytes past
    prow = lambda f: f[2:2 + ns * pstride].view(ns, pstride)
    for k in range(2):
        rows(flat["l"][k])[:, :n] = torch.from_numpy(np.array(left[:, k * n:(k + 1) * n]))      # (copies: the shared inputs are read-only)
        rows(flat["r"][k])[:, :n] = torch.from_numpy(np.array(right[:, k * n:(k + 1) * n]))
        assert rows(flat["l"][k]).data_ptr() % 16 == 4 and prow(pflat[k]).data_ptr() % 16 == 4
    torch.cuda.synchronize()
    with pkg.StereoPcmSink(ns, alpha, GAIN, exact=exact) as sink:
        _start(sink, h0, ht, 7)
        sink.set_stream(stream.cuda_stream)
        for k in range(2):
            sink.process_batch_device(rows(flat["l"][k]), rows(flat["r"][k]), prow(pflat[k]), n)
        stream.synchronize()
        st = sink.state()
        assert np.array_equal(sink.hicut_state()[0], [hr.ramp(h0[s], ht[s], 7, 2 * n) for s in range(ns)])
    got = []
    for k in range(2):
        whole = pflat[k].cpu().numpy()
        body = whole[2:2 + ns * pstride].reshape(ns, pstride)
        assert (whole[:2] == 12345).all() and (whole[2 + ns * pstride:] == 12345).all() and (body[:, 2 * n:] == 12345).all(), k
        got.append(body[:, :2 * n])
    got = np.concatenate(got, axis=1)
    if exact:
        assert np.array_equal(got, want) and np.array_equal(_bits(st), _bits(want_st))
    else:
        ok, lsb, share, cap, rel = _caps(got, st, want, want_st)
        print("default, device pointers: max |PCM difference| %d, share %.3g (cap %.3g), state %.3g relative" % (lsb, share, cap, rel))
        assert ok, (lsb, share, rel)
