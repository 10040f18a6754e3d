"""CPU checks of tests/pilot_shape_cases.py, the reference side of tests/test_scan_shapes_gpu.py and tests/test_bcast_tuned_shapes_gpu.py: the
step geometry every shape gets from the Python copies of scan_lds, bcast_lds and bcast_lds_tuned (and that these copies are the ones the
older sweeps carry), the long call's split, how many outputs of every case sit at the pilot gate — tuned_cases.EXCLUDED_CAP is a
condition the cases were chosen to meet, from the references alone — and the magnitude case's conditions."""
import numpy as np
import pytest

import pilot_shape_cases as ps
import scan_ref as sr
import tuned_cases as tc
from test_bcast_shapes_gpu import _ndt as bcast_ndt
from test_bcast_shapes_gpu import _split
from test_scan_gpu import _ndt as scan_ndt

SCAN_IDS = [ps.scan_id(s) for s in ps.SCAN_SHAPES]
BCAST_IDS = [ps.bcast_id(s) for s in ps.BCAST_SHAPES]


# ---- the geometry table ---------------------------------------------------------------------------------------------------------------
def test_scan_steps_are_the_host_geometrys():
    for shape in ps.SCAN_SHAPES:
        st = ps.scan_step(shape)
        assert st["NDT"] == st["NY"] - 1 == scan_ndt(*shape) and st["lds"] <= ps.LDS_BUDGET, (shape, st)
        print("scan %s: NY %d, NDT %d, H %d, LDS %d bytes" % (ps.scan_id(shape), st["NY"], st["NDT"], st["H"], st["lds"]))
        if shape in ps.SCAN_LDS_LIMITED:
            ndt, lds = ps.SCAN_STEPS[shape]
            assert st["NDT"] == ndt < 1023 and lds in (None, st["lds"]), (shape, st)
            T, D, P = shape
            assert ps.scan_lds(T, D, P, st["NY"] + 2, st["NY"] + 1) > ps.LDS_BUDGET      # the next larger step does not fit
        else:
            assert st["NDT"] == 1023, (shape, st)
    assert ps.scan_step((1, 1, 1))["H"] == 0 == ps.scan_step((256, 1, 1))["H"]
    assert ps.LDS_BUDGET - ps.scan_step((255, 17, 3))["lds"] == 8
    assert ps.scan_step((64, 10, 101), generic=False) == dict(NY=1024, NDT=1023, lds=ps.scan_lds(64, 10, 101, 1024, 1023), fast=True, H=100)
    assert [ps.scan_name(s, False) for s in ps.SCAN_SHAPES + [(64, 10, 101)]].count("scan-fast T64 D10 P101") == 1


def test_bcast_steps_are_the_host_geometrys():
    for shape in ps.BCAST_SHAPES:
        T, D, P, Ta, Da, Tr, Dr = shape
        for tuned in (False, True):
            st = ps.bcast_step(shape, tuned)
            assert st["lds"] <= ps.LDS_BUDGET and st["NDT"] == st["NY"] - 1 and st["H"] == P - 1 + max(Ta, Tr) - 1, (shape, tuned, st)
            print("bcast %s %s: NY %d, NDT %d, H %d, LDS %d bytes" % (ps.bcast_id(shape), "tuned" if tuned else "untuned", st["NY"], st["NDT"], st["H"],
                                                                      st["lds"]))
        assert ps.bcast_step(shape, False)["NDT"] == bcast_ndt(T, D, P, Ta, Tr, False)
        # the fast kernels are claimed at T64 D10 P101 alone, and there by the tuned form as well: T more words fit
        fast = (T, D, P) == (64, 10, 101)
        assert ps.bcast_step(shape, False, generic=False)["fast"] == ps.bcast_step(shape, True, generic=False)["fast"] == fast, shape
        assert ("fast" in ps.bcast_name(shape, True, False)) == fast and "generic-tuned" in ps.bcast_name(shape, True, True)
    steps = {tuned: ps.bcast_step(ps.BCAST_D64, tuned) for tuned in (False, True)}
    assert {t: s["NDT"] for t, s in steps.items()} == ps.BCAST_D64_STEPS and steps[True]["NDT"] < steps[False]["NDT"] < 1023
    assert steps[True]["H"] == 509 > 2 * steps[True]["NDT"]          # the prologue alone takes three steps
    wide = ps.bcast_step((256, 16, 255, 256, 1, 256, 1), True)
    assert wide["NDT"] < ps.bcast_step((256, 16, 255, 256, 1, 256, 1), False)["NDT"] < 1023


@pytest.mark.parametrize("kind", ["scan", "bcast"])
def test_the_long_call_is_the_smallest_with_three_workgroups_of_two_full_steps(kind):
    """by the copy of front_split, at 1 .. 8 workgroups a unit: the long call meets the geometry, one step less does not, and every case
    fits a metered call's 4 MiB"""
    for idx, shape in enumerate(ps.SCAN_SHAPES if kind == "scan" else ps.BCAST_SHAPES):
        st = ps.scan_step(shape) if kind == "scan" else ps.bcast_step(shape, False)
        ns = (ps.SCAN_STREAMS if kind == "scan" else ps.BCAST_STREAMS)[idx]
        D = shape[1]
        cuts, long_ = ps.ragged_cuts(D, st["H"], st["NDT"], ns, () if kind == "scan" else (shape[4], shape[6]), 1)
        M = long_ // 2 // D
        assert M % st["NDT"] == 0 and ps.split_ok(M, st["NDT"], st["H"], ns) and not ps.split_ok(M - st["NDT"], st["NDT"], st["H"], ns), (shape, M)
        for ndt in {st["NDT"], ps.bcast_step(shape, True)["NDT"]} if kind == "bcast" else {st["NDT"]}:
            for per_cu in ps.PER_CU:
                bps, span = _split(M, ndt, st["H"], ns, per_cu * ps.CUS)
                assert bps >= 3 and span >= 2 * ndt, (shape, ndt, per_cu, bps, span)
        assert sum(cuts) <= ps.MAX_CALL and 0 in cuts and 2 in cuts and long_ in cuts
        phase, phases = 0, []
        for c in cuts:
            phases.append(phase)
            phase = (phase + c // 2) % D
        assert D == 1 or any(p != 0 for p in phases[cuts.index(long_):]), (shape, cuts)   # the long call starts at a phase != 0
        if st["H"] >= 4:
            assert any(0 < c // 2 // D < st["H"] for c in cuts), (shape, cuts)


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.SCAN_SHAPES, ids=SCAN_IDS)
def test_few_d_of_a_scan_case_sit_at_the_gate(pkg, shape):
    case = ps.scan_case(pkg, shape)
    shares = ps.scan_shares(case)
    print("scan %s: %s, pilot_min %.4g, n %d, n_pilot %s, shares at the gate %s" % (
        ps.scan_id(shape), "/".join(case["names"]), case["pilot_min"], case["refs"][0]["rec"]["n"], [r["rec"]["n_pilot"] for r in case["refs"]],
        ["%.5f" % v for v in shares]))
    assert max(shares) <= tc.EXCLUDED_CAP, (shape, shares)
    assert case["iq"].shape == (case["ns"], sum(case["cuts"])) and all(r["rec"]["n"] == sum(case["cuts"]) // 2 // shape[1] for r in case["refs"])
    assert len(set(case["cycles"])) == min(case["ns"], 5)            # the offsets differ
    # the threshold of the exact comparisons lies inside the rows' powers
    pm = ps.mid_gate(case["names"], [r["pw"] for r in case["refs"]])
    assert any(0 < int((r["pw"] >= np.float32(pm) ** 2).sum()) < r["pw"].size for r in case["refs"]), (shape, pm)


@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=BCAST_IDS)
def test_few_outputs_of_a_broadcast_case_sit_at_the_gate(pkg, shape):
    case = ps.bcast_case(pkg, shape)
    frac, keep_a, keep_r, n_amb = tc.case_keeps(case, case["refs"])
    print("bcast %s: %s, pilot_min %.4g, M %d, pilot counts %s, d's at the gate %s, %.3f %% of the outputs excluded" % (
        ps.bcast_id(shape), "/".join(case["names"]), case["pilot_min"], case["refs"][0]["d"].size, [r["rds"]["count"] for r in case["refs"]], n_amb,
        100 * frac))
    assert frac <= tc.EXCLUDED_CAP, (shape, frac)
    assert case["iq"].shape == (case["ns"], sum(case["cuts"]))
    T, D, P, Ta, Da, Tr, Dr = shape
    M = sum(case["cuts"]) // 2 // D
    assert all(r["L"].size == M // Da and r["bb"].size == M // Dr for r in case["refs"])


# ---- the record at the top of its range -------------------------------------------------------------------------------------------
def test_magnitude_case_meets_its_conditions_on_the_reference(pkg):
    m = ps.magnitude_case(pkg)
    f64 = np.float64
    # the taps sit on the refusal bounds exactly
    assert np.abs(m["ctaps"].astype(f64)).sum(1).tolist() == [16.0, 16.0]
    assert float(np.abs(m["b"].real.astype(f64)).sum() + np.abs(m["b"].imag.astype(f64)).sum()) == 8.0
    assert m["iq"].shape == (2, ps.MAG_WARM + ps.MAG_BYTES) and ps.MAG_BYTES == 4 << 20
    r0, r1 = m["refs"]
    first = ps.MAG_WARM // 2
    for r in (r0, r1):
        assert r["rec"]["n"] == 1 << 21 and r["rec"]["n_pilot"] == 1 << 21              # MAG_GATES[0]: every d of the call passes
        assert int((r["pw"][first:] >= np.float32(ps.MAG_GATES[1]) ** 2).sum()) == 0    # MAG_GATES[1]: none does
    pw, p = r0["pw"][first:].astype(f64), r0["p"][first:].astype(f64)
    d = r0["d"][first:].astype(f64)
    print("magnitude case, stream 0: max p %.0f, |d| in [%.4f, %.4f], max pw 2^24 = 2^%.2f, max g 2^20 = 2^%.2f, pilot2_q = 2^%.2f, rf_q = 2^%.2f" % (
        p.max(), np.abs(d).min(), np.abs(d).max(), np.log2(pw.max()) + 24, 2 * np.log2(pw.max()) + 20, np.log2(r0["rec"]["pilot2_q"]),
        np.log2(r0["rec"]["rf_q"])))
    print("magnitude case, stream 1: mean d %.4f, freq_q = -2^%.2f" % (r1["d"][first:].astype(f64).mean(), np.log2(-r1["rec"]["freq_q"])))
    assert p.max() == 8323200.0                                      # the bound of tests/test_scan_ref.py's worst case
    assert pw.max() * 2.0 ** 24 >= 2.0 ** 33 and pw.max() ** 2 * 2.0 ** 20 >= 2.0 ** 38
    assert 2 ** 59 <= r0["rec"]["pilot2_q"] < 2 ** 62 and 2 ** 51 <= r0["rec"]["rf_q"] < 2 ** 52
    assert r1["rec"]["freq_q"] <= -2 ** 46
    # what a 32-bit conversion of pw or g would make of it differs from the record
    q24 = np.rint((r0["pw"][first:] * np.float32(2.0 ** 24)).astype(np.float32)).astype(np.int64)
    assert int(q24.sum()) == r0["rec"]["pilot_q"] and int(q24.astype(np.int32).astype(np.int64).sum()) != r0["rec"]["pilot_q"]
    assert sr.rec_of(r0["rec"])["reserved"] == 0
