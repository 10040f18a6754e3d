"""CPU pre-check of tests/test_fm_host_paths_gpu.py: every ladder of tests/fm_host_cases.py at a 32-audio-tap geometry through the FM call path's host
arithmetic (csrc/sdrfm_fm_call.h, driven by tests/native/fm_shape_cases.cpp with the FmGeom sdrfm_create arrives at on a 256-CU device), as host rows and
as the ring's device rows.  Each call must reach the word the table names, and each ladder must still hold every class of call it was built for — a ladder
that silently stopped reaching fm_short_first, an odd phase_x or design Q would otherwise only show on the GPU.  Behind them, the ring's refusals that need
no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import fm_host_cases as hc
import fm_shape_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c for c in hc.all_cases() if c.mode == "fm"]            # (the other inputs reuse a ladder)


@pytest.fixture(scope="module")
def cases_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("native") / "fm_shape_cases")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests/native/fm_shape_cases.cpp")], check=True, cwd=ROOT,
                   capture_output=True, text=True)
    return exe


def _answers(exe, case, device, cls):
    g = case.geom
    args = [str(v) for v in (g.T, g.D, g.Da, 1, int(case.flags == "bit_exact"), 0, 1)]
    args += ["%d:%d:0:%d" % (c.N, cls, device) for c in case.calls]
    r = subprocess.run([exe] + args, capture_output=True, text=True, check=True, timeout=60)
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(case.calls), r.stdout
    return rows


def test_the_table_is_well_formed():
    cases = hc.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert {c.geom for c in cases} == set(hc.GEOMS) and {c.flags for c in cases} == set(hc.FLAGS)
    assert {c.geom for c in cases if c.flags == "force_generic"} == {hc.GEOMS[0]}
    for g in hc.GEOMS:
        assert {c.mode for c in cases if c.geom == g} == {"fm", "random", "const"}
    assert [c.name for c in cases if c.ladder == "q"] == ["T64-D10-Ta32-Da5-default-q-fm"]
    for c in cases:
        assert all(k.nbytes % 2 == 0 for k in c.calls), c.name
        assert sum(1 for k in c.calls if k.N) > hc.n_slots(c) or c.ladder == "q", c.name      # a submit meets a full ring
        total = sum(k.N for k in c.calls)
        assert total == 2 * fs.ONE_NSAMP if c.ladder == "q" else total < 150000, (c.name, total)
        assert hc.slot_stride(hc.slot_bytes(c)) % 256 == 0 and fs.align_class(0, hc.slot_stride(hc.slot_bytes(c))) == 16
        for k in c.calls:
            assert (k.word is None) == (k.N == 0 or not hc.names_words(c.geom)), (c.name, k)
            assert k.word in (None, "fast-q", "fast-b", "generic"), (c.name, k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_ladder_holds_the_classes_it_was_built_for(case):
    g = case.geom
    tags = set().union(*(k.tags for k in case.calls))
    for t in case.must:
        assert t in tags, (case.name, t)
    first = case.calls[0]
    if case.ladder == "main":
        # the calls that keep n_seen + 1 < T come one after the other from the first sample on, more than one of them, and the next call crosses
        kept = [k for k in case.calls if "start-kept" in k.tags]
        assert first.N == 1 and len(kept) >= 3 and kept == list(case.calls[:len(kept)]) and "start-crossed" in case.calls[len(kept)].tags
        crossing = case.calls[len(kept)]
        assert crossing.M >= hc.y_aff(g) + g.Ta and crossing.A > 0          # long enough for the fast kernel and its fix-up
        assert case.calls[len(kept) + 1].N == 0
        assert any(k.N > 0 and k.A == 0 and k.n_seen + 1 >= g.T for k in case.calls)
        # an odd count at an even phase, and directly or one small call behind it the call at an odd phase that restores the even one
        i = next(i for i, k in enumerate(case.calls) if "ring-2mod4" in k.tags)
        assert case.calls[i].N % 2 == 1 and any("phase-restored" in k.tags and k.N >= hc.BASE // 2 for k in case.calls[i + 1:i + 3])
        for nbytes in (65534, 65536, 65538):
            k = next(k for k in case.calls if k.nbytes == nbytes)
            assert k.phase_x % 2 == 0 and k.A > 0, (case.name, k)             # (the fast kernel's call where the handle has one)
    if case.ladder in ("below", "at"):
        assert first.n_seen == 0 and first.phase_x == 0 and first.M == hc.y_aff(g) + g.Ta - (1 if case.ladder == "below" else 0) and first.A > 0
    if case.ladder == "q":
        assert [k.N for k in case.calls] == [fs.ONE_NSAMP] * 2 and all((k.phase_x, k.phase_d) == (0, 0) for k in case.calls)
    if hc.names_words(g) and case.flags != "force_generic":
        words = {k.word for k in case.calls}
        assert case.ladder == "q" or ("generic" in words and "fast-b" in words), (case.name, words)
        if case.ladder in ("below", "at"):
            assert first.word == ("generic" if case.ladder == "below" else "fast-b")
        if case.ladder == "q":
            assert words == {"fast-q"}
        if case.ladder == "main":
            for t in hc.CLASS_TAGS + ("switch-65534", "switch-65536", "switch-65538"):
                assert all(k.word == "fast-b" for k in case.calls if t in k.tags), (case.name, t)
            assert all(k.word == "generic" for k in case.calls if "odd-phase" in k.tags or "no-audio" in k.tags)
            assert [k.word for k in case.calls if "start-crossed" in k.tags] == ["fast-b"]


@pytest.mark.parametrize("case", [c for c in CASES if hc.names_words(c.geom) and c.flags != "force_generic"], ids=lambda c: c.name)
def test_every_call_reaches_the_word_the_table_names(cases_exe, case):
    """as host rows (device = 0: 16-aligned) and as the ring's rows (device = 1 with the class of a 256-aligned pointer and the slot's stride)"""
    ring_cls = fs.align_class(0, hc.slot_stride(hc.slot_bytes(case)))
    for device, cls in ((0, 16), (1, ring_cls)):
        for k, (call, row) in enumerate(zip(case.calls, _answers(cases_exe, case, device, cls))):
            nsamp, M, A, q_fit, q_ok, stream_ok, fast_ok = row[:7]
            assert (nsamp, M, A) == (call.N, call.M, call.A), (case.name, k, row)
            assert not stream_ok, (case.name, k, row)                       # (one stream never fills the machine for design S)
            if call.N == 0:
                assert call.word is None
                continue
            word = "fast-q" if q_ok else "fast-b" if fast_ok else "generic"
            assert word == call.word, (case.name, k, device, word, call.word, row)


def test_a_forced_generic_handle_names_the_generic_kernel_for_every_call():
    for case in hc.all_cases():
        if case.flags == "force_generic":
            assert all(k.word == "generic" for k in case.calls if k.N), case.name


# ---- the ring's refusals that need no device ------------------------------------------------------------------------------------------------------
def test_ring_calls_refuse_null_arguments_without_touching_the_gpu(pkg):
    lib = pkg.load_library()
    EINVAL = 16
    out = C.c_void_p(0xDEAD)
    assert lib.sdrfm_ring_create(None, 15, 262144, C.byref(out)) == EINVAL and not out.value      # (*out is NULL after a refusal)
    assert lib.sdrfm_ring_create(None, 15, 262144, None) == EINVAL
    byte = (C.c_uint8 * 2)()
    n = C.c_uint32(7)
    buf = (C.c_float * 4)()
    assert lib.sdrfm_ring_submit(None, C.addressof(byte), 2) == EINVAL
    assert lib.sdrfm_ring_submit(None, None, 0) == EINVAL
    assert lib.sdrfm_ring_collect(None, C.addressof(buf), 4, C.byref(n), 0) == EINVAL
    assert lib.sdrfm_ring_collect(None, C.addressof(buf), 4, C.byref(n), 1) == EINVAL
    assert lib.sdrfm_ring_destroy(None) is None                                                   # harmless
