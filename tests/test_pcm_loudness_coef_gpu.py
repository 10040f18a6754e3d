"""The loudness meter on the device at every coefficient set of its domain (csrc/sdrfm_loudness.h), where the existing device
tests run the default set alone.  tests/loudness_cases.py lists the sets — the K-weighting re-derived at four other rates and a stress grid of
pole positions — with the two figures tests/test_loudness_emulate_cpu.py measured for each on the CPU; a set whose figures are at most an
eighth of the hard conditions is in domain, and the device is held to 8 x ITS figures:  |e - e_host| <= RTOL_set e_host + ATOL_set block_len,
within 1e-9 and 1e-3 LSB^2 per sample for every set here.  The reference is the C routine on the PCM the device returned, call by call with
its state carried; pos and the block counts are exact.  The rows are the ones the figures were measured on, where the scan's error peaks."""
import numpy as np
import pytest

import loudness_cases as lc

pytestmark = pytest.mark.gpu

IN_DOMAIN = [name for name in lc.coef_sets() if lc.in_domain(name)]


def _sink(pkg):
    return pkg.StereoPcmSink(2, 1.0, 1.0, exact=True)


def _rows(Li, Ri):
    return np.ascontiguousarray(Li, dtype=np.float32), np.ascontiguousarray(Ri, dtype=np.float32)


def _used(got, want, bl, rtol, atol):
    """the largest share of the bound a difference takes (printed, never asserted on)"""
    d, bound = np.abs(np.asarray(got) - np.asarray(want)), rtol * np.asarray(want) + atol * bl
    return float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _run(pkg, sink, name, coef, bl, calls, tag):
    """the calls of one row through a sink already enabled with coef at bl, from sub-block 0: every call against the C routine.  Returns the
    largest share of the bound that was used"""
    rtol, atol = lc.coef_tolerance(name)
    st, at, used = None, 0, 0.0
    for k, (Li, Ri) in enumerate(calls):
        pcm = sink.process_batch(*_rows(Li, Ri))
        assert np.array_equal(pcm, lc.interleave(Li, Ri))                                    # alpha = 1, gain = 1: the case's values are the PCM
        first, got = sink.read_loudness()
        want, st = pkg.pcm_loudness_host(pcm, bl, coef, state=st)
        assert first == at and got.shape == want.shape, (tag, k, first, at, got.shape, want.shape)
        dev = sink.loudness_state()
        used = max(used, _used(got, want, bl, rtol, atol), _used(dev["e"], st["e"], bl, rtol, atol))
        ok, why = lc.within(got, want, bl, rtol, atol)
        assert ok, (tag, k, why)
        assert np.array_equal(dev["pos"], st["pos"]), (tag, k)
        ok, why = lc.within(dev["e"], st["e"], bl, rtol, atol)
        assert ok, (tag, k, "open energy", why)
        at += got.shape[1]
    assert at == sum(c[0].shape[1] for c in calls) // bl
    return used


def test_the_domain_holds_what_the_issue_names():
    assert {"default", "k32000", "k44100", "k96000"} <= set(IN_DOMAIN) and "k192000" not in IN_DOMAIN
    assert not [n for n in IN_DOMAIN if "pi-1e-" in n] and len(IN_DOMAIN) >= 12
    for name in IN_DOMAIN:
        rtol, atol = lc.coef_tolerance(name)
        assert rtol <= 1e-9 and atol <= 1e-3, name


@pytest.mark.parametrize("name", IN_DOMAIN)
def test_every_set_of_the_domain(pkg, name):
    """DC at the positive rail in two calls, a full-range burst and three calls of zeros, a full-range row of TILE + 1 pairs; block_len 64
    and 4800; two streams, the second with L and R exchanged"""
    coef = lc.coef_sets()[name]
    used = {}
    for bl in lc.COEF_BLOCK_LENS:
        for row, calls in lc.coef_rows(False).items():
            with _sink(pkg) as sink:
                sink.enable_loudness(bl, (lc.TILE + 1) // bl + 1, coef=coef)
                used[row] = max(used.get(row, 0.0), _run(pkg, sink, name, coef, bl, calls, (name, bl, row)))
    print("%-24s RTOL %.3g ATOL %.3g: of the bound, at most %s" % ((name,) + lc.coef_tolerance(name) + (", ".join("%.2f on %s" % (v, k) for k, v in used.items()),)))


def test_enabling_again_with_another_set_starts_over(pkg):
    """one sink, one set after the other without disabling in between: every enable starts at sub-block 0 from zero state and meters with
    the new set — a table or a coefficient left over from the set before shows on the DC row"""
    bl = 64
    calls = lc.coef_rows(False)["dc_pos"]
    order = ["k96000", "hp r=0.999 th=pi-0.3", "default", "hp real 0.999 -0.9", "k32000"]
    assert all(lc.in_domain(n) for n in order)
    outside = lc.coef_sets()["k192000"]
    with _sink(pkg) as sink:
        for name in order:
            coef = lc.coef_sets()[name]
            sink.enable_loudness(bl, 4800 // bl, coef=coef)
            assert not sink.loudness_state().tobytes().strip(b"\0"), name
            _run(pkg, sink, name, coef, bl, calls, ("again", name))
            before = sink.loudness_state()
            with pytest.raises(pkg.SdrfmError) as e:                                         # a set outside the domain is refused ...
                sink.enable_loudness(bl, 4800 // bl, coef=outside)
            assert e.value.status == pkg.lib.EINVAL
            assert sink.loudness_state().tobytes() == before.tobytes(), name                 # ... and the live meter stays as it was
        # the sets differ where it matters: the default's energies on this row are not the last set's
        a = pkg.pcm_loudness_host(lc.interleave(*calls[0]), bl, lc.coef_sets()["default"])[0]
        b = pkg.pcm_loudness_host(lc.interleave(*calls[0]), bl, lc.coef_sets()["k32000"])[0]
        assert not lc.within(a, b, bl)[0]
