"""CPU checks of the hist kernels' step geometry on tests/bcast_hist_cases.py's Python copies of the host functions — the
table of the section, the bins wholly behind the plain layout and inside the budget, fast-plain implies fast-hist over every (Ta, Tr) the
header accepts — and of the reference side of the GPU case that is held to tests/scan_ref.py from bytes: how many of its d's sit at a bin
edge."""
import os
import re

import numpy as np

import bcast_hist_cases as bh
import pilot_shape_cases as ps
import scan_hist_cases as hc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stm32f7-rtlsdr_amd", "csrc")
SHAPES = [bh.DEFAULT, bh.TABLE_DEFAULT] + ps.BCAST_SHAPES + [ps.BCAST_D64, bh.TOP_SHAPE]


def test_geometry_table():
    for tuned in (False, True):
        for shape in (bh.TABLE_DEFAULT, bh.DEFAULT):
            plain, hist = ps.bcast_step(shape, tuned, generic=False), bh.hist_step(shape, tuned, generic=False)
            assert plain["fast"] and hist["fast"] and plain["NDT"] == hist["NDT"] == 1023, (plain, hist)
            assert 2 * hist["lds"] <= 160 << 10                      # still two workgroups per compute unit of 160 KiB
            if shape == bh.TABLE_DEFAULT:
                assert (plain["lds"], hist["lds"]) == bh.DEFAULT_LDS[tuned], (tuned, plain["lds"], hist["lds"])
        assert bh.hist_name(bh.DEFAULT, tuned, False) == ps.bcast_name(bh.DEFAULT, tuned, False) + " + hist"
        assert bh.hist_name(bh.DEFAULT, tuned, False, blend=True) == ps.bcast_name(bh.DEFAULT, tuned, False) + " blend + hist"
        for shape, want in bh.STEPS.items():
            got = (ps.bcast_step(shape, tuned)["NDT"], bh.hist_step(shape, tuned)["NDT"])
            assert got == want[tuned], (shape, tuned, got, want[tuned])
    assert bh.STEPS[ps.BCAST_D64][True][0] == ps.BCAST_D64_STEPS[True] and bh.STEPS[ps.BCAST_D64][False][0] == ps.BCAST_D64_STEPS[False]


def test_bins_lie_behind_the_plain_layout_and_inside_the_budget():
    for shape in SHAPES:
        for tuned in (False, True):
            for generic in ((False, True) if shape[:3] == (64, 10, 101) else (True,)):
                plain, st = ps.bcast_step(shape, tuned, generic), bh.hist_step(shape, tuned, generic)
                off = bh.bins_offset(shape, tuned, st["NY"], st["NDT"])
                assert st["lds"] % 16 == 0 and off % 16 == 0 and st["lds"] <= ps.LDS_BUDGET, (shape, tuned, st)
                assert off >= bh.plain_lds(shape, tuned, st["NY"], st["NDT"]) and off + bh.HIST_LDS_BYTES == st["lds"], (shape, tuned, off, st)
                assert 2 <= st["NY"] <= plain["NY"] and st["NDT"] == st["NY"] - 1 and st["H"] == plain["H"], (shape, plain, st)
                if st["NDT"] == plain["NDT"]:
                    assert st["lds"] - plain["lds"] in range(bh.HIST_LDS_BYTES, bh.HIST_LDS_BYTES + 16)
                else:                                               # LDS-limited: one more pair of y's would not fit beside the bins
                    assert not st["fast"] and bh.hist_lds(shape, tuned, st["NY"] + 2, st["NY"] + 1) > ps.LDS_BUDGET, (shape, tuned, st)


def test_fast_plain_implies_fast_hist_over_every_tap_count():
    """T 64, D 10, P 101: wherever the plain form takes the fast kernel's step, the bins fit beside it"""
    worst = 0
    for tuned in (False, True):
        for Ta in range(1, bh.MAX_TAPS + 1):
            for Tr in range(1, bh.MAX_TAPS + 1):
                shape = (64, 10, 101, Ta, 5, Tr, 25)
                if bh.plain_lds(shape, tuned, ps.FAST_NY, ps.FAST_NY - 1) <= ps.LDS_BUDGET:
                    lds = bh.hist_lds(shape, tuned, ps.FAST_NY, ps.FAST_NY - 1)
                    assert lds <= ps.LDS_BUDGET, (tuned, Ta, Tr, lds)
                    worst = max(worst, lds)
    print("the largest fast hist step takes %d of %d bytes" % (worst, ps.LDS_BUDGET))
    assert worst == bh.hist_lds((64, 10, 101, 256, 5, 256, 25), True, ps.FAST_NY, ps.FAST_NY - 1)


def test_python_copies_follow_the_source():
    """the source computes the hist LDS as this file does, and leaves the scan handle's headers alone"""
    src = open(os.path.join(CSRC, "sdrfm_bcast.hip")).read()
    assert re.search(r"size_t bcast_hist_lds\([^)]*\) \{\s*return hist_bins_offset\(bcast_lds\([^)]*\)\) \+ HIST_LDS_BYTES;", src)
    assert re.search(r"size_t bcast_hist_lds_tuned\([^)]*\) \{\s*return hist_bins_offset\(bcast_lds_tuned\([^)]*\)\) \+ HIST_LDS_BYTES;", src)
    assert "f.hist_fast = f.fast && f.hist_step.lds <= PF_LDS_BUDGET;" in src
    seven = r"k_bcast<\d+, \d+, \d+, (?:true|false), %s, (?:true|false), true>"
    assert len(re.findall(seven % "true", src)) == 8 and not re.search(seven % "false", src)     # the eight hist instantiations, all metered


def test_bracket_check_holds_on_the_definition_and_catches_a_moved_count():
    rng = np.random.default_rng(5)
    d = rng.uniform(-np.pi, np.pi, 5000).astype(np.float32)
    dq = np.rint(d * hc.Q24).astype(np.int64)
    meters = np.zeros(2, np.dtype([("n", "<u8"), ("freq_q", "<i8")]))
    meters["n"], meters["freq_q"] = (d.size, 0), (int(dq.sum()), 0)
    hist = np.stack([hc.hist_of(d), np.zeros(bh.BINS, np.uint64)]).astype(np.uint32)
    bh.check_rows(meters, hist)
    moved = hist.copy()
    b = int(np.flatnonzero(moved[0])[0])
    moved[0, b] -= 1
    moved[0, 457] += 5000                                           # the sum and the bracket both break
    for bad in (moved, np.roll(hist, 40, axis=1)):
        try:
            bh.check_rows(meters, bad)
        except AssertionError:
            continue
        raise AssertionError("check_rows took a wrong row")


def test_reference_case_has_few_d_at_a_bin_edge(pkg):
    """the GPU case held to tests/scan_ref.py from bytes: per stream at most 0.4 % of the reference's d's within 1e-5 rad of a bin edge (the
    inputs alone keep it: no constant rows, the unmodulated carriers in the middle of a bin)"""
    cs = bh.ref_case(pkg)
    assert "const" not in cs["names"] and cs["shape"] == bh.DEFAULT[:3]
    for s, r in enumerate(cs["refs"]):
        share = hc.edge_share(r["d"])
        print("stream %d (%s at %+.4f): %.3f %% of %d d's at an edge" % (s, cs["names"][s], cs["cycles"][s], 100 * share, r["d"].size))
        assert share <= hc.EDGE_CAP, (s, cs["names"][s], share)
