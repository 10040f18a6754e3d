"""The FM handle's create-time plan (csrc/sdrfm_fm_plan.h: fm_plan — which designs a handle owns, its FmGeom, its names) on the CPU, held to
tests/golden/fm_plan_mi355x.json: what sdrfm_create arrived at on an MI355X BEFORE the planning function existed, printed by an instrumented copy of
that library for every case of tests/fm_plan_cases.py.  The inputs are the recorded answers of the runtime and of design Q's translation unit plus the
verdicts on the taps, computed here from the same taps by the library's own routines (tests/native/fm_plan_case.cpp); every field must match, the
doubles exactly (they are literals)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fm_plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stm32f7-rtlsdr_amd", "csrc")
RECORD = pc.load_record()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("native")
    exe, obj = str(d / "fm_plan_case"), str(d / "qtaps.o")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-c", "-o", obj, os.path.join(CSRC, "qtaps.c")], check=True, cwd=ROOT, capture_output=True, text=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests/native/fm_plan_case.cpp"), obj, "-lm"], check=True,
                   cwd=ROOT, capture_output=True, text=True)
    return exe


def _plan(exe, pkg, tmp_path, rec, refuse_q=False, facts=None):
    h, g = pc.taps(pkg, rec["T"], rec["D"], rec["Ta"], rec["Da"], rec["taps"])
    path = str(tmp_path / "taps.f32")
    np.concatenate([h, g]).astype(np.float32).tofile(path)
    r = rec["plan"]["runtime"]
    facts = facts or "%d:%d:%d:%d:%d" % (r["n_cu"], r["q_default_nslot"], r["q_default_lds"], r["mix_lds"], r["mix_blocks_per_cu"])
    args = [rec["T"], rec["D"], rec["Ta"], rec["Da"], pc.N_STREAMS, rec["flags"], int(refuse_q), facts, path]
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True, timeout=60)
    return json.loads(out.stdout)


def _without_runtime(plan):
    return {k: v for k, v in plan.items() if k != "runtime"}


def test_the_record_covers_the_cases():
    assert sorted(RECORD) == sorted(c[0] for c in pc.cases())
    assert all(r["plan"]["runtime"]["n_cu"] == 256 for r in RECORD.values())
    kinds = {(r["plan"]["geo"]["has_q"], r["plan"]["geo"]["has_fast"], r["plan"]["geo"]["has_s"], r["plan"]["geo"]["has_mix_tile"]) for r in RECORD.values()}
    assert {(1, 1, 1, 1), (1, 1, 0, 1), (1, 0, 0, 0), (0, 1, 1, 0), (0, 1, 0, 0), (0, 0, 0, 0)} <= kinds   # every combination of designs a handle can end up with
    assert RECORD["T64-D10-Ta32-Da5-bandpass"]["plan"]["geo"]["has_q"] == 0 and RECORD["T64-D16-Ta32-Da8-default"]["plan"]["geo"]["NA"] == 32


@pytest.mark.parametrize("cid", sorted(RECORD))
def test_the_plan_is_the_recorded_one(plan_exe, pkg, tmp_path, cid):
    rec = RECORD[cid]
    got, want = _plan(plan_exe, pkg, tmp_path, rec), _without_runtime(rec["plan"])
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (cid, key, got[key], want[key])
    assert rec["name_after_create"] == want["names"]["kernel"]


@pytest.mark.parametrize("shape", ["T%d-D%d-Ta%d-Da%d" % s for s in pc.WITH_INSTANCE + pc.WITHOUT])
def test_a_handle_refused_design_q_plans_as_a_bit_exact_one(plan_exe, pkg, tmp_path, shape):
    """sdrfm_create plans again without design Q when its tables or routing state cannot be allocated: the recorded SDRFM_CFG_BIT_EXACT plan (whose guard
    fields are zero as well: neither handle has a guard)."""
    got = _plan(plan_exe, pkg, tmp_path, RECORD[shape + "-default"], refuse_q=True)
    assert got == _without_runtime(RECORD[shape + "-bit-exact"]["plan"])


@pytest.mark.parametrize("cid", sorted(c for c in RECORD if c.endswith("-default")))
def test_the_native_checks_facts_are_the_recorded_ones(plan_exe, pkg, tmp_path, cid):
    """tests/native/fm_geom.h keeps an MI355X's answers for fm_call_check.cpp and fm_shape_cases.cpp: planned with them, every default handle is the recorded one"""
    assert _plan(plan_exe, pkg, tmp_path, RECORD[cid], facts="mi355x") == _without_runtime(RECORD[cid]["plan"])
