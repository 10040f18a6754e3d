"""The cases of tests/limit_cases.py on the CPU: the case list is complete (it is the set of shapes for which the library itself answers, nothing
left out on either side), the skewed tables are what they say they are and sit where sdrfm_truepeak_check_coef draws its line, and at every case
the GPU tests run against the definition the host routines sdrfm_pcm_limit_s16 / sdrfm_pcm_tplimit_s16 equal the numpy definition
(tests/limit_ref.py, tests/limit_tp_ref.py) in PCM, all state words and all four record fields — so that holding the device to the host routine
elsewhere in tests/test_pcm_limit_shapes_gpu.py is holding it to the definition.  Every comparison is integer equality."""
import numpy as np
import pytest

import limit_cases as cases
import limit_ref as ref


def test_the_sample_shapes_are_the_ones_the_library_answers_for(pkg):
    lib = pkg.load_library()
    taken = [lw for lw in range(0, 11) if lib.sdrfm_pcm_limit_state_words(lw) != 0]
    assert cases.sample_shapes() == taken and len(taken) == 7
    assert all(lib.sdrfm_pcm_limit_state_words(lw) == 4 * ((1 << lw) - 1) for lw in taken)


def test_the_true_peak_shapes_are_the_ones_the_library_answers_for(pkg):
    """over the whole grid lw 0 .. 10, P 1 .. 9, NT 0 .. 68: a triple is a case exactly when sdrfm_pcm_tplimit_state_words answers for (lw, NT) and
    sdrfm_truepeak_check_coef takes a table of [P, NT]"""
    lib = pkg.load_library()
    zeros = np.zeros(9 * 68 + 1, np.int16)
    table_ok = {(P, NT): lib.sdrfm_truepeak_check_coef(zeros.ctypes.data, P, NT) == 0 for P in range(1, 10) for NT in range(0, 69)}
    taken = {(lw, P, NT) for lw in range(0, 11) for P in range(1, 10) for NT in range(0, 69)
             if lib.sdrfm_pcm_tplimit_state_words(lw, NT) != 0 and table_ok[(P, NT)]}
    shapes = cases.tp_shapes()
    assert len(shapes) == len(set(shapes)) == 234 and all(sum(1 for s in shapes if s[1] == P) == 78 for P in (2, 4, 8))
    assert set(shapes) == taken, (sorted(set(shapes) - taken)[:5], sorted(taken - set(shapes))[:5])
    for lw, P, NT in shapes:
        assert lib.sdrfm_pcm_tplimit_state_words(lw, NT) == 4 * ((1 << lw) - 1) + NT and lib.sdrfm_pcm_tplimit_latency(lw, NT) == cases.latency(lw, NT)


def test_the_definition_cases_are_shapes_and_cross_the_host_routines_block_border():
    for form, lw, P, NT, table in cases.DEFINITION_CASES:
        assert lw in cases.sample_shapes() if form == "sample" else (lw, P, NT) in cases.tp_shapes()
        assert cases.TILE + cases.latency(lw, NT) + 2 > 1024 and cases.DEFINITION_SECOND > 1024     # LIMIT_BLOCK of csrc/limit.c and csrc/limit_tp.c


@pytest.mark.parametrize("P", cases.PHASES)
def test_skew_tables_are_skewed_bounded_and_sit_at_the_librarys_line(pkg, P):
    """at every tap count, loose and at the bound: asymmetric, no row a row reversed, every half-row's sum <= 65535 (== 65535 at the bound), taken by
    sdrfm_truepeak_check_coef — and refused with any one half-row raised by 1"""
    lib = pkg.load_library()
    for NT in cases.TAPS:
        for at_bound in (False, True):
            c = cases.skew_table(P, NT, 7, at_bound)
            assert c.dtype == np.int16 and c.shape == (P, NT) and c.flags.c_contiguous
            assert not np.array_equal(c, c[::-1, ::-1]) and cases.table_is_skewed(c), (P, NT, at_bound)
            assert np.array_equal(c, cases.skew_table(P, NT, 7, at_bound)) and not np.array_equal(c, cases.skew_table(P, NT, 8, at_bound))
            sums = cases.half_sums(c)
            assert (sums <= cases.HALF_MAX).all() and (not at_bound or (sums == cases.HALF_MAX).all()), (P, NT, sums)
            assert (c < 0).any() and (c > 0).any() and len(np.unique(np.abs(c))) > 1
            assert lib.sdrfm_truepeak_check_coef(c.ctypes.data, P, NT) == 0
            if at_bound:
                for p in range(P):
                    for h in range(2):
                        half = c[p, h * (NT // 2):(h + 1) * (NT // 2)].astype(np.int64)
                        room = ((half >= 0) & (half < 32767)) | ((half < 0) & (half > -32768))
                        if not room.any():                                                       # 32767 beside -32768: int16 has no larger half-row
                            assert NT == 4
                            continue
                        k = int(np.argmax(room))
                        over = c.copy()
                        over[p, h * (NT // 2) + k] += 1 if half[k] >= 0 else -1                  # one LSB further from zero
                        assert int(cases.half_sums(over)[p, h]) == cases.HALF_MAX + 1
                        assert lib.sdrfm_truepeak_check_coef(over.ctypes.data, P, NT) == pkg.lib.EINVAL, (P, NT, p, h)


def test_the_rail_burst_reaches_the_largest_sum_the_table_allows():
    for P, NT in ((2, 4), (4, 12), (8, 64)):
        c = cases.skew_table(P, NT, 7, True)
        b = cases.rail_burst(c).astype(np.int64).reshape(-1, 2)
        assert b.shape == (NT, 2) and set(np.unique(b)) == {-32768, 32767} and np.array_equal(b[:, 0] < 0, b[:, 1] > 0)
        a = [abs(int((c[0].astype(np.int64) * (16 * b[::-1, ch])).sum())) for ch in range(2)]    # the burst's last pair meets tap 0
        assert max(a) >= 0.9999 * cases.SUM_MAX and max(a) <= cases.SUM_MAX < 1 << 36


@pytest.mark.parametrize("form,lw,P,NT,table", cases.DEFINITION_CASES)
def test_the_host_routine_is_the_definition_at_the_cases_the_device_runs(pkg, form, lw, P, NT, table):
    """the five corners, a call of TILE + L + 2 pairs with a rail burst straddling pair TILE, then 1500 pairs from the carried state"""
    case = cases.definition_case(form, lw, P, NT, table)
    par = np.array(case["par"], dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
    st, rec, at = None, None, 0
    for k, n in enumerate(case["cuts"]):
        x = case["x"][:, 2 * at:2 * (at + n)]
        if form == "sample":
            out, st, rec = pkg.pcm_limit_host(x, lw, 1, 0, par, st, rec)
        else:
            out, st, rec = pkg.pcm_limit_tp_host(x, lw, 1, 0, par, st, rec, coef=case["coef"])
        assert np.array_equal(out, case["out"][k]), (k, [s for s in range(5) if not np.array_equal(out[s], case["out"][k][s])])
        assert np.array_equal(st, case["state"][k]) and [ref.rec_tuple(r) for r in rec] == case["rec"][k], k
        assert (np.abs(out.astype(np.int64)).max(axis=1) <= par["ceiling"]).all()
        at += n
    if table == "bound":
        assert case["peak"] >= 0.999 * cases.SUM_MAX                                             # the burst under G = 65536 reaches the bound
    assert [r[1] > 0 for r in case["rec"][1]] == [True, True, True, True, False]                 # every corner limits but the gain of 0
