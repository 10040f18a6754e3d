"""CPU checks of tests/audio_shape_cases.py, the reference side of tests/test_bcast_audio_shapes_gpu.py: what the slew rule
achieves at every shape of tests/pilot_shape_cases.py — the ramps move at the long call's first output, still move two workgroup spans into
it, have ended before its last, and differ between the streams —, and the condition under which the GPU comparison can tell a kernel that
reads the wrong stream's record, or counts the outputs since the set one off, from a right one: the expected L or R moves by more than 2 TOL
on a kept output of every stream.  The share of outputs at the pilot gate needs no check here: blending does not move the gate, and
tests/test_pilot_shapes_cpu.py holds these cases to tuned_cases.EXCLUDED_CAP."""
import numpy as np
import pytest

import audio_ref as ar
import audio_shape_cases as asc
import pilot_shape_cases as ps
import tuned_cases as tc

TOL = 1e-5                                                      # tests/test_bcast_tuned_gpu.py's (a GPU module: not imported here)
IDS = [ps.bcast_id(s) for s in ps.BCAST_SHAPES]
SILENT = {(ps.BCAST_D64, 2)}                                    # (shape, stream): the const row half a cycle a sample away, |am| <= 1.5e-8


def test_starts_and_targets_are_distinct_and_no_power_of_two():
    (b0, v0), (bt, vt) = asc.starts(7), asc.targets(7)
    assert list(bt[:3]) == [5000, 12001, 19002] and list(vt[:3]) == [29768, 20767, 11766]
    for a in (b0, v0, bt, vt):
        assert len(set(a.tolist())) == 7 and all(0 < int(x) < ar.ONE and int(x) & (int(x) - 1) for x in a), a
    dist = np.concatenate([np.abs(bt - b0), np.abs(vt - v0)])
    assert (dist.min(), dist.max()) == (13885, 19384)
    for ns in (1, 3):                                            # fewer streams take the first of the seven
        assert all(np.array_equal(x[:ns], y) for x, y in zip((b0, v0, bt, vt), asc.starts(ns) + asc.targets(ns)))


def test_the_vectorised_ramp_is_the_scalar_one():
    rng = np.random.default_rng(5)
    for _ in range(200):
        x0, xt = (int(v) for v in rng.integers(0, ar.ONE + 1, 2))
        slew, J = int(rng.choice([1, 2, 7, 159, 4096, ar.ONE - 1, ar.ONE])), int(rng.choice([0, 1, 65535, 65536, 131071, 200000]))
        assert ar.ramp_outputs(x0, xt, slew, J, 40).tolist() == [ar.ramp(x0, xt, slew, J + j + 1) for j in range(40)]


@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=IDS)
def test_what_the_slew_achieves(shape):
    rm = asc.case_ramps(shape)
    ns, a0, a1, b, v = rm["ns"], rm["a0"], rm["a1"], rm["b"], rm["v"]
    a_long = a1 - a0
    assert rm["counts"][rm["cuts"].index(max(rm["cuts"]))] == a_long and b.shape == v.shape == (ns, rm["bounds"][-1])
    want = asc.SHORT_SLEW if a_long < asc.SHORT else max(asc.SLEW_FLOOR.get(shape, 1), ar.ONE // (a_long // 2))
    assert rm["slew"] == want and (rm["rule"] == "the shape's floor") == (shape in asc.SLEW_FLOOR), rm["rule"]
    # output 0 is one slew away from the starts: the set stands before the row's first byte
    assert np.array_equal(np.abs(b[:, 0] - rm["b0"]), np.full(ns, rm["slew"])) and np.array_equal(np.abs(v[:, 0] - rm["v0"]), np.full(ns, rm["slew"]))
    ends = []
    for s in range(ns):
        for x, xt in ((b[s], rm["bt"][s]), (v[s], rm["vt"][s])):
            end = int(np.flatnonzero(x != xt)[-1]) + 1               # the first output at the target
            ends.append(end)
            assert x[a0] != x[a0 - 1] and x[a0] != xt, (shape, s, "not moving at the long call's first output")
            assert a0 < end < a1 - 1, (shape, s, end, a0, a1)        # it ends inside the long call
            assert len(np.unique(x[a0:a1])) > min(1000, a_long // 8), (shape, s, "a step, not a ramp")
        # the stream's conditioning is still moving two workgroup spans into the long call, at the widest split the device may choose
        assert max(ends[-2:]) > a0 + rm["span"], (shape, s, ends[-2:], a0, rm["span"])
    mid = (a0 + a1) // 2
    pairs = [(int(b[s, mid]), int(v[s, mid])) for s in range(ns)]
    assert len(set(p[0] for p in pairs)) == ns and len(set(p[1] for p in pairs)) == ns, (shape, pairs)
    print("%s: %d streams, A_long %d from output %d, slew %d (%s), two spans <= %d outputs, the ramps end %d .. %d outputs into the long call" % (
        ps.bcast_id(shape), ns, a_long, a0, rm["slew"], rm["rule"], rm["span"], min(ends) - a0, max(ends) - a0))


def test_no_present_shape_takes_the_short_rule():
    assert min(asc.case_ramps(s)["a1"] - asc.case_ramps(s)["a0"] for s in ps.BCAST_SHAPES) == 410 >= asc.SHORT
    assert asc.slew_of(ps.BCAST_D64, 63) == (ar.ONE // 8, "short") and asc.slew_of(ps.BCAST_D64, 64)[0] == 1024


def test_the_call_bounds_are_the_decimators():
    """a handle's audio count of a call is what floor division of the samples so far gives: the case's bounds against a walk of the phases"""
    for shape in ps.BCAST_SHAPES:
        D, Da = shape[1], shape[4]
        rm = asc.case_ramps(shape)
        phase, dphase, counts = 0, 0, []
        for c in rm["cuts"]:
            m = (phase + c // 2) // D
            phase = (phase + c // 2) % D
            counts.append((dphase + m) // Da)
            dphase = (dphase + m) % Da
        assert counts == rm["counts"], shape


@pytest.mark.parametrize("shape", ps.BCAST_SHAPES, ids=IDS)
def test_the_comparison_can_tell_a_wrong_count_and_a_wrong_record(pkg, shape):
    ac = asc.audio_case(pkg, shape)
    case, rm = ac["case"], ac["ramps"]
    frac, keep_a, keep_r, n_amb = tc.case_keeps(case, case["refs"])
    silent = asc.silent_streams(ac, keep_a)
    assert {(shape, s) for s in silent} == {k for k in SILENT if k[0] == shape}, (shape, silent)
    for r in case["refs"]:                                           # the expected rows at blend = gain = 1 are the reference's own L and R
        l, r_ = ar.blend(r["stereo"]["am"], r["stereo"]["as_"], ar.ONE, ar.ONE)
        assert np.array_equal(l, r["L"]) and np.array_equal(r_, r["R"])
    for what in asc.WRONG:
        if what == asc.WRONG[1] and rm["ns"] == 1:
            assert np.array_equal(ac["wrong"][what][0], ac["L"])     # one stream: its record rotates onto itself
            continue
        moved = []
        for s in range(rm["ns"]):
            d = np.maximum(np.abs(ac["wrong"][what][0][s].astype(np.float64) - ac["L"][s]), np.abs(ac["wrong"][what][1][s].astype(np.float64) - ac["R"][s]))
            moved.append(float(d[keep_a[s]].max()))
            assert s in silent or moved[-1] > 2 * TOL, (shape, what, s, case["names"][s], moved[-1])
        print("%s, %s: the expected rows move by %s" % (ps.bcast_id(shape), what, ["%.3g" % m for m in moved]))
