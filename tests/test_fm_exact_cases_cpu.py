"""CPU pre-check of tests/test_fm_exact_shapes_gpu.py: every case of tests/fm_exact_cases.py through the FM call path's host arithmetic
(csrc/sdrfm_fm_call.h, driven by tests/native/fm_exact_cases.cpp with the FmGeom of a bit-exact handle on a 256-CU device).  Each call must reach the
class the table names for it — generic tile size, design B's segments, the short last one, the folded hand-over, the first call's fix-up — so that a
case that silently stopped reaching its class fails here and does not go unnoticed on the GPU.  The oracle leg: the taps' unit absolute sum that TOL is
stated for, that a reversed or shifted tap moves the reference by more than 100 TOL on the streams the GPU test feeds, and the exact zeros of the
zero-sum case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fm_exact_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Row = xc.namedtuple("Row", "N M A phase_x phase_d kind NA tiles fold subtiles short_first fixup min_subtiles")


@pytest.fixture(scope="module")
def cases_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("native") / "fm_exact_cases")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests/native/fm_exact_cases.cpp")], check=True, cwd=ROOT,
                   capture_output=True, text=True)
    return exe


def _answers(exe, T, D, Ta, Da, ns, calls):
    """((NA, lds, supported) of the handle, [Row per call])"""
    args = [str(v) for v in (T, D, Ta, Da, ns)] + ["%d:%d" % c for c in calls]
    r = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(calls) + 1, r.stdout
    rows = [Row(*[v if k == 5 else int(v) for k, v in enumerate(line.split())]) for line in lines[1:]]
    return tuple(int(v) for v in lines[0].split()), rows


def _generic_lds(shape, NA):
    """the generic kernel's block at NA outputs per tile: xs | ys | ds | h | g (csrc/sdrfm.hip: k_generic)"""
    T, D, Ta, Da = shape
    ND = (NA - 1) * Da + Ta
    return ((ND * D + T) + (ND + 1)) * 8 + (ND + T + Ta) * 4


# ---- A. the generic kernel ---------------------------------------------------------------------------------------------------------------------------
def test_the_generic_shapes_cover_every_tile_size():
    assert sorted({na for na, _ in xc.GENERIC_SHAPES}) == [1, 2, 4, 8, 16, 32, 64]
    shapes = [s for _, s in xc.GENERIC_SHAPES]
    assert len(set(shapes)) == len(shapes) == 17 and (256, 64, 256, 64) in shapes
    assert all(1 <= T <= 256 and 1 <= D <= 64 and 1 <= Ta <= 256 and 1 <= Da <= 64 for T, D, Ta, Da in shapes)
    assert sorted(xc.generic_na(s) for s in xc.UNALIGNED_SHAPES) == [1, 4, 64]
    assert all(xc.generic_streams(s) > 1 for s in xc.UNALIGNED_SHAPES)
    assert {xc.generic_streams(s) for s in shapes} == {1, 3, 7}
    off, pad = xc.UNALIGNED_LAYOUT
    assert off % 2 == 1 and pad % 2 == 1


@pytest.mark.parametrize("shape", [s for _, s in xc.GENERIC_SHAPES], ids=xc.shape_id)
def test_every_generic_shape_reaches_its_tile_size_and_its_ragged_classes(cases_exe, shape):
    T, D, Ta, Da = shape
    ns, NA = xc.generic_streams(shape), xc.generic_na(shape)
    calls = xc.generic_calls(shape)
    total = xc.generic_total(shape)
    (na, lds, supported), rows = _answers(cases_exe, T, D, Ta, Da, ns, [(c.nsamp, 16) for c in calls])
    assert na == NA and supported == 1 and lds <= 160 * 1024, (shape, na, lds)
    assert lds == _generic_lds(shape, NA) and (lds <= 48 * 1024 or NA == 1), (shape, lds)
    assert NA == 64 or _generic_lds(shape, 2 * NA) > 48 * 1024, shape     # NA halves only while the block does not fit 48 KiB
    for row in rows:
        assert row.kind == ("-" if row.N == 0 else "g") and (row.N == 0 or row.NA == NA), (shape, row)
        assert row.tiles == (row.A + NA - 1) // NA and row.fold == 0 and row.short_first == 0 and row.fixup == 0, (shape, row)
    why = {c.why: row for c, row in zip(calls, rows)}
    # the classes a ragged list must hold, wherever the shape has them
    assert rows[0].N == 0 and rows[1].N == 1
    assert (D >= 2) == ("M=0,N>0" in why) and (D < 2 or (why["M=0,N>0"].M == 0 and why["M=0,N>0"].N > 0))
    assert (Ta >= 3) == ("0<M<Ta-1" in why) and (Ta < 3 or 0 < why["0<M<Ta-1"].M < Ta - 1)
    assert (T >= 3) == ("N<T-1" in why) and (T < 3 or 0 < why["N<T-1"].N < T - 1)
    odd_after = [k for k in range(len(rows) - 1) if rows[k + 1].phase_x % 2 == 1]
    assert (D >= 2) == bool(odd_after), (shape, odd_after)
    seen_d = {row.phase_d for row in rows}
    assert len(seen_d) >= min(3, Da), (shape, seen_d)
    long, tail = why["long"], why["tail"]
    assert long.tiles >= 3 and long.A >= 3 * NA + 1 and (long.A % NA != 0 or NA == 1) and long.M >= Ta + 2 * Da, (shape, long)
    assert tail.N > 0 and tail.A >= 1, (shape, tail)             # a call behind the long one reads the state it handed over
    # ... and the same stream in one call
    _, (one,) = _answers(cases_exe, T, D, Ta, Da, ns, [(total, 16)])
    assert total % 2 == 1 and one.N == total and one.A == sum(r.A for r in rows), (shape, one)
    assert one.kind == "g" and one.tiles >= 3 and (one.A % NA != 0 or NA == 1) and one.M >= Ta + 2 * Da, (shape, one)


def test_the_largest_generic_block_is_above_the_default_dynamic_lds_limit(cases_exe):
    (na, lds, supported), _ = _answers(cases_exe, 256, 64, 256, 64, 7, [(4097, 16)])
    assert (na, supported) == (1, 1) and 64 * 1024 < lds <= 160 * 1024, lds


# ---- B. design B ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_design_b_table_is_well_formed():
    cases = xc.all_b_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and set(names) == set(xc.REACH)
    assert len(xc.B_INSTANCES) == 7 and xc.B_INSTANCES[-1] == (64, 16, 5, 8)      # (the / 16 rate gets the R = 8 tile)
    for c in cases + list(xc.DEV_R8_CASES):
        assert c.name in xc.REACH or c in xc.DEV_R8_CASES
        for k in c.calls:
            assert k.cls in (16, 4) and (c.device or k.cls == 16), (c.name, k)
            if (c.T, c.D) in ((64, 10), (32, 10)):
                assert k.nsamp % 480 != 0, (c.name, k)               # off design S's whole lane segments
    assert {c.ns for c in cases} == {1, 3, 7, 520, 342}
    assert {k.cls for c in cases if c.device for k in c.calls} == {16, 4}


@pytest.mark.parametrize("case", xc.all_b_cases(), ids=lambda c: c.name)
def test_every_design_b_call_reaches_the_class_the_table_names(cases_exe, case):
    Ta, NYT = xc.B_TA, 64 * case.R
    yaff = xc.y_aff(case.T, case.D)
    (gna, _, _), rows = _answers(cases_exe, case.T, case.D, Ta, case.Da, case.ns, [(c.nsamp, c.cls) for c in case.calls])
    reach = xc.REACH[case.name]
    assert len(reach) == len(rows) == len(case.calls)
    n_seen = 0
    for k, (call, row, want) in enumerate(zip(case.calls, rows, reach)):
        got = xc.Reach(row.kind, row.NA, row.tiles, row.fold, row.short_first, row.fixup, row.min_subtiles)
        assert got == want, (case.name, k, call, row)
        assert row.N == call.nsamp and row.A > 0 and row.subtiles == (row.M + NYT - 1) // NYT, (case.name, k, row)
        if row.kind == "g":
            assert row.NA == gna and row.tiles == (row.A + gna - 1) // gna
        last = row.A - (row.tiles - 1) * row.NA                      # outputs of the last segment
        assert 0 < last <= row.NA
        why = call.why
        if why == "first-b":
            assert n_seen == 0 and row.kind == "b" and row.M == yaff + Ta and not row.short_first and row.fixup >= 1
        elif why == "first-g":
            assert n_seen == 0 and row.kind == "g" and row.M == yaff + Ta - 1 and row.short_first and row.fixup == 0
        elif why == "one-subtile":
            assert n_seen > 0 and (row.kind, row.tiles, row.subtiles, row.fold) == ("b", 1, 1, 1)
        elif why == "many-short-last":
            assert row.kind == "b" and case.ns == 1 and row.tiles == row.subtiles == 11 and last < row.NA and row.min_subtiles == 1
        elif why == "no-fold":
            assert row.kind == "b" and row.fold == 0 and case.Da <= row.M < Ta
        elif why == "even-phase":
            assert row.kind == "b" and row.phase_x % 2 == 0 and row.phase_x > 0
        elif why == "odd-phase":
            assert row.kind == "g" and row.phase_x % 2 == 1
        elif why == "back-on-b":
            assert row.kind == "b" and rows[k - 1].kind == "g" and row.phase_x == 0
        elif why == "segments":
            assert row.kind == "b" and row.tiles == {3: 5, 7: 3}[case.ns] == row.subtiles and last < row.NA and row.fold == 1
            assert (row.fixup >= 1) == (k == 0)
        elif why.startswith("back-off-"):
            assert row.kind == "b" and row.min_subtiles == int(why[-1]) and row.tiles == (2 if why[-1] == "2" else 3), (case.name, k, row)
        else:
            assert why in ("b", "phase_d") and row.kind == "b"
        n_seen += row.N
    if case.name.endswith("one-stream"):
        # the phases: design B at an even non-zero phase_x, the generic kernel behind an odd one, design B back; every phase_d under design B
        assert {r.phase_d for r in rows if r.kind == "b"} == set(range(case.Da)), case.name
        kinds = "".join(r.kind for r in rows)
        assert "bgg" in kinds and kinds.endswith("b")
    if case.name.endswith("342-streams"):
        assert rows[0].NA == 615


def test_the_development_r8_cases_reach_their_segments(cases_exe):
    """b(64, 10, 8) as SDRFM_FAST_R=8 selects it: the same cut in sub-tiles of 512 decimated outputs (the plan here is the product's R = 12 tile, so only the
    counts the GPU test relies on are checked: calls design B serves at phase_x 0, off design S's lane segments)."""
    for case in xc.DEV_R8_CASES:
        _, rows = _answers(cases_exe, case.T, case.D, xc.B_TA, case.Da, case.ns, [(c.nsamp, c.cls) for c in case.calls])
        assert all(r.kind == "b" and r.phase_x == 0 and r.N % 480 != 0 for r in rows), case.name
        assert all((r.M + 511) // 512 >= 4 for r in rows), case.name


# ---- the oracle leg ----------------------------------------------------------------------------------------------------------------------------------
def test_every_shapes_audio_taps_have_unit_absolute_sum():
    for taps, shapes in ((xc.generic_taps, [s for _, s in xc.GENERIC_SHAPES]), (xc.b_taps, xc.B_INSTANCES)):
        for s in shapes:
            h, g = taps(s)
            assert h.dtype == g.dtype == np.float32 and h.size == s[0]
            assert abs(float(np.abs(g.astype(np.float64)).sum()) - 1.0) <= 1e-6, s
            assert all(v.size < 4 or not np.array_equal(v, v[::-1]) for v in (h, g)), s   # asymmetric: a reversed tap order changes the result


@pytest.mark.parametrize("shape", [s for _, s in xc.GENERIC_SHAPES], ids=xc.shape_id)
def test_the_comparison_can_tell_a_reversed_and_a_shifted_tap(pkg, oracle_mod, shape):
    """What the GPU test's inputs are chosen for: on the very streams it feeds a shape, a reference with the channel taps reversed, or the audio taps
    shifted by one, is further than 100 TOL from the true one on every carrier and noise stream — a kernel with that index wrong cannot pass.  (The
    constant and the counter streams are there for their byte patterns: a counter repeats every 128 samples, which / 64 turns into a period of two.)"""
    T, D, Ta, Da = shape
    h, g = xc.generic_taps(shape)
    rows = xc.generic_rows(pkg, shape)
    for s, row in enumerate(rows):
        if xc.STREAM_CLASSES[s % 4] in ("const", "counter"):
            continue
        want = oracle_mod.Oracle(h, g, D, Da).process(row)
        assert want.size >= 3 * xc.generic_na(shape) + 1
        wrong = ([("h reversed", h[::-1].copy(), g)] if T >= 2 else []) + ([("g shifted", h, np.roll(g, 1))] if Ta >= 2 else [])
        assert wrong or shape == (1, 1, 1, 1)
        for what, hw, gw in wrong:
            e = float(np.max(np.abs(oracle_mod.Oracle(hw, gw, D, Da).process(row).astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)))
            assert e > 100 * 1e-5, (shape, s, what, e)


@pytest.mark.parametrize("T,D,Ta,Da", xc.ZERO_SHAPES, ids=lambda v: str(v))
def test_the_zero_sum_taps_give_positive_zero_on_every_oracle_output(oracle_mod, T, D, Ta, Da):
    h, g = xc.zero_sum_taps(T, Ta)
    assert float(h.astype(np.float64).sum()) == 0.0
    rows = xc.zero_rows(T, D, Da, 12 if Ta == xc.B_TA else 0)
    want = oracle_mod.Oracle(h, g, D, Da).process(rows[0])
    assert want.size == rows.shape[1] // 2 // D // Da and want.size > 0
    assert not want.view(np.uint32).any(), np.flatnonzero(want.view(np.uint32))[:8]
    mixed = oracle_mod.Oracle(h, g, D, Da).process(rows[1])
    assert np.isfinite(mixed).all() and np.abs(mixed).max() > 1e-3   # the second stream leaves the zeros and comes back
