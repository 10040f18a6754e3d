"""CPU pre-check of tests/test_fm_shapes_gpu.py: every case of tests/fm_shape_cases.py through the FM call path's host arithmetic (csrc/sdrfm_fm_call.h,
driven by tests/native/fm_shape_cases.cpp with the FmGeom sdrfm_create arrives at on a 256-CU device).  Each call must reach the design the GPU test
names for it — a case that silently stopped reaching its design would otherwise only show on the GPU."""
import os
import shutil
import subprocess

import pytest

import fm_shape_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("native") / "fm_shape_cases")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests/native/fm_shape_cases.cpp")], check=True, cwd=ROOT,
                   capture_output=True, text=True)
    return exe


def _answers(exe, case):
    args = [str(v) for v in (case.T, case.D, case.Da, case.ns, int(case.bit_exact), case.n_routed, case.route_at)]
    args += ["%d:%d:%d:%d" % (c.nsamp, c.cls, int(c.overlap), int(c.device)) for c in case.calls]
    r = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=60)
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(case.calls), r.stdout
    return rows


def test_the_table_is_well_formed():
    cases = fc.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert sorted(len(v) for v in fc.LAYOUTS.values()) == [2, 3, 6]
    for cls, layouts in fc.LAYOUTS.items():
        for off, pad in layouts:
            for nbytes in (3200, 4800, 3072):                    # (call sizes of whole 16-byte pieces: the class is the layout's alone)
                assert fc.align_class(4096 + off, nbytes + pad) == cls, (cls, off, pad)
    assert all(fc.align_class(4096 + o, s) == c for c, (o, p) in fc.REPRESENTATIVE.items() for s in (3200 + p,))
    assert fc.ONE_NSAMP % 400 == 0 and fc.ONE_NSAMP // 10 // 128 >= 512              # (one stream fills 256 CUs twice over with 512 steps)
    for c in cases:
        assert c.calls and all(k.expect in ("fast-q", "fast-s", "fast-b", "generic") for k in c.calls), c.name
        assert not any(k.overlapped and not (k.overlap and k.expect == "fast-q") for k in c.calls), c.name


@pytest.mark.parametrize("case", fc.all_cases(), ids=lambda c: c.name)
def test_every_call_reaches_the_design_the_gpu_test_names(cases_exe, case):
    for k, (call, row) in enumerate(zip(case.calls, _answers(cases_exe, case))):
        nsamp, M, A, q_fit, q_ok, stream_ok, fast_ok, prev_dev, prev_q, geo_ok, overlapped, fuse = row
        assert nsamp == call.nsamp and A > 0, (case.name, k, row)
        word = "fast-q" if q_ok else "fast-s" if stream_ok else "fast-b" if fast_ok else "generic"
        assert word == call.expect, (case.name, k, word, call.expect, row)
        # (the table's buffers never share rows and its audio buffers alternate: SDRFM_F_OVERLAP holds wherever the previous call and the geometry allow it)
        assert bool(overlapped) == call.overlapped, (case.name, k, row)
        if case.n_routed and q_ok and k >= case.route_at:
            assert call.mixed == ("one" if fuse else "two"), (case.name, k, row)
        else:
            assert call.mixed is None, (case.name, k)
        if call.cls != 16 and call.device:
            assert not q_fit and not stream_ok, (case.name, k, row)  # fm_q_fit and fm_stream_ok refuse an unaligned row


def test_which_term_refuses_the_flag_in_the_overlap_cases(cases_exe):
    """The length rule of fm_ovl_geometry_ok decides alone in "prev-short" (design Q served the 1200-sample call, from device rows); in the cases behind
    design B the previous call is what refuses the flag, whatever the geometry says."""
    rows = _answers(cases_exe, fc.by_name("overlap-prev-short"))
    nsamp, M, A, q_fit, q_ok, stream_ok, fast_ok, prev_dev, prev_q, geo_ok, overlapped, fuse = rows[2]
    assert rows[1][0] == 1200 and rows[1][4] == 1                  # the short call is design Q's
    assert (q_ok, prev_dev, prev_q, geo_ok, overlapped) == (1, 1, 1, 0, 0), rows[2]
    assert rows[1][10] == 1 and rows[3][10] == 1                   # ... and it is itself overlapped, as is the call behind the refused one
    for name, k in (("overlap-prev-4-aligned", 2), ("overlap-prev-not-whole-pieces", 2), ("overlap-prev-served-by-b", 1), ("overlap-flag-on-unaligned", 2),
                    ("overlap-prev-served-by-b-then-routed", 2)):
        row = _answers(cases_exe, fc.by_name(name))[k]
        assert row[4] == 1 and row[7] == 1 and row[8] == 0 and row[10] == 0, (name, row)   # design Q's call, a device buffer before it, not design Q's
    assert _answers(cases_exe, fc.by_name("overlap-prev-served-by-b"))[1][9] == 1            # (the geometry alone would have allowed it)
    assert _answers(cases_exe, fc.by_name("overlap-prev-served-by-b-then-routed"))[2][9] == 0   # (4-aligned rows before it)
