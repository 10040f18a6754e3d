"""The true-peak kernel (csrc/sdrfm_truepeak.h) over the tables it accepts: 2, 4 and 8 phases of 4, 12, 16 and 64 taps from
taps.truepeak_coef, and tables at the half-row bound against rail input, whose values reach 2 * 65535 * 32768 = 4 294 901 760, the top of the
32-bit half of the key.  n = 257 and 4801; the reference and the rule — integer equality of all eight fields — are
tests/test_pcm_truepeak_gpu.py's."""
import numpy as np
import pytest

import truepeak_ref as ref

pytestmark = pytest.mark.gpu


def _agree(pkg, got, pcm, limit, coef, tag):
    want, _ = ref.records(pcm, coef, limit)
    assert ref.same(got, want), (tag, ref.diff(got, want))
    host, _ = pkg.pcm_truepeak_host(pcm, limit, coef)
    assert ref.same(host, want), (tag, "the C routine", ref.diff(host, want))


@pytest.mark.parametrize("NT", [4, 12, 16, 64])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_designed_tables(pkg, P, NT):
    coef = pkg.truepeak_coef(P, NT)
    rng = np.random.default_rng(3500 + 100 * P + NT)
    for n in (257, 4801):
        L, R = ref.random_full_range(rng, 3, n)
        with pkg.StereoPcmSink(3, ref.ALPHA, ref.GAIN) as sink:
            sink.enable_truepeak(coef=coef)
            assert sink.truepeak_phases == P
            cuts = (0, 5, 8, n // 3, n)                                                     # calls of 5 and 3 pairs: shorter than any history but NT = 4's
            parts = [sink.process_batch(*ref.rows_of(L[:, u:v], R[:, u:v])) for u, v in zip(cuts, cuts[1:])]
            got = sink.read_truepeak()
        pcm = np.concatenate(parts, axis=1)
        assert int(np.abs(pcm.astype(np.int32)).max()) > 30000
        _agree(pkg, got, pcm, ref.LIMIT_M1, coef, (P, NT, n))
        assert (got["n"] == n).all() and (got["peak_l"] > 1 << 29).all()


@pytest.mark.parametrize("P,NT", [(2, 4), (4, 12), (8, 64), (8, 16)])
def test_a_table_at_the_bound_against_the_rail(pkg, P, NT):
    """exact form: every tap of the table is negative with sum of |coef| = 65535 per half-row, the input a constant -32768, so every product is
    positive and A = 4 294 901 760 from pair NT - 1 at the latest — either half-row is 65535 * 32768, one short of wrapping an int32 — and a
    full-range row through the same table"""
    coef = ref.bound_table(P, NT)
    assert pkg.load_library().sdrfm_truepeak_check_coef(coef.ctypes.data, P, NT) == 0
    rng = np.random.default_rng(3600 + NT)
    for n in (257, 4801):
        L = np.full((2, n), -32768, np.int64)
        R = L.copy()
        R[1], _ = ref.random_full_range(rng, 1, n)
        for limit in (ref.BOUND_PEAK, ref.BOUND_PEAK - 1):
            with pkg.StereoPcmSink(2, ref.ALPHA, ref.GAIN, exact=True) as sink:
                sink.enable_truepeak(coef=coef, limit=limit)
                pcm = sink.process_batch(*ref.rows_of(L, R))
                got = sink.read_truepeak()
            assert np.array_equal(pcm, ref.interleave(L, R))
            _agree(pkg, got, pcm, limit, coef, (P, NT, n, limit))
            assert (got["peak_l"] == 4294901760).all() and int(got["peak_r"][0]) == 4294901760 and (got["at_l"] <= NT - 1).all()
            assert (got["over_l"] > 0).all() == (limit < ref.BOUND_PEAK) and (got["over_l"] == 0).all() == (limit == ref.BOUND_PEAK)
