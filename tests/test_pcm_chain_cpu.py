"""CPU: the arithmetic of the PCM sink inside the demodulator's launch (csrc/sdrfm_sink_chain.h) restated in numpy (tools/pcm_chain_emulate.py), held to the host
routine sdrfm_pcm_deemph_s16 (csrc/pcm_sink.c) — the bit-exact definition of the sink — without a GPU.  The emulator takes the chain's tables from the library
(sdrfm_sink_chain_tables), publishes a run's end state as the kernel does (scan value times dinv) and cuts a call into the launch's own runs and flushes
(csrc/sdrfm_fm_call.h through tests/native/pcm_chain_runs.cpp, the run geometry of csrc/sdrfm_q.hip restated in run_cuts).

The written answer on alpha = 1 (test_a_runs_last_flush_ends_off_a_multiple_of_eight_...): at the shapes tests/test_pcm_sink_params_gpu.py runs, every one of the 34
runs of the chain's two calls (83 to 90 outputs each, one flush) ends its last flush off a multiple of 8 outputs, so dinv[k >= 1] IS applied, and at alpha = 1 it is infinite times a scan value of 0:
NaN, which then finishes the successor's first 64 outputs and is carried into the next call.  The positions are reachable; alpha = 1 is safe only because
sdrfm_sink_chain_tables answers 1 (the sink's own kernel) wherever (1 - alpha)^8 is not a normal float."""
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pcm_params as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
emu = importlib.import_module("pcm_chain_emulate")

GAIN = np.float32(pp.DEFAULT_GAIN)
# tests/test_pcm_sink_params_gpu.py's plan for the chain: 64 streams, 64 channel taps, / 10 / 5, three calls of 48 000, 48 400 and 96 000 samples on a 256-CU device
# with 12 design-Q waves per CU (what sdrfm_create arrives at on an MI355X: tests/native/fm_call_check.cpp); the stream's first call goes to the sink's own kernel
PLAN_NBYTES = [96000, 96800, 192000]


def _audio(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    return (1.3 * np.sin(2 * np.pi * 1000 * t + 0.3) + 0.6 * np.sin(2 * np.pi * 3100 * t) + 0.3 * np.sin(2 * np.pi * 12000 * t) +
            0.05 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def runs_exe(tmp_path_factory):
    """tests/native/pcm_chain_runs.cpp, built: the host arithmetic the launch uses"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("native") / "pcm_chain_runs")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests/native/pcm_chain_runs.cpp")], check=True, cwd=ROOT,
                   capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def plan_runs(runs_exe):
    """{nbytes: (M, A, runs)} of the plan's calls"""
    exe = runs_exe
    r = subprocess.run([exe, "64", "10", "32", "5", "64", "256", "12"] + [str(n) for n in PLAN_NBYTES], capture_output=True, text=True, check=True, timeout=60)
    out = {}
    for line in r.stdout.splitlines():
        nbytes, M, A, q_fit, fits, runs, with_chain = (int(v) for v in line.split())
        assert q_fit and fits and with_chain, line                 # design Q serves every call of the plan, with the chain
        out[nbytes] = (M, A, runs)
    assert out == {96000: (4800, 960, 11), 96800: (4840, 968, 11), 192000: (9600, 1920, 23)}, out    # (150, 152 and 300 quads: runs of 13 quads at least)
    return out


def _emulate_plan(pkg, plan_runs, alpha, gain, overlap, seed, force_chain=False):
    """The plan's three calls of one stream: (PCM values by the library's path for this alpha, the host routine's, emulated state, host state).  The first call is the
    sink's own kernel's (design Q's first call of a stream holds no chain: the exact chain stands for it), the others the chain's when the library lets it serve."""
    lib = pkg.load_library()
    chain = force_chain or emu.chain_tables(alpha)[0] == 2
    got, want, st, est = [], [], 0.0, 0.0
    for k, nbytes in enumerate(PLAN_NBYTES):
        M, A, runs = plan_runs[nbytes]
        x = _audio(A, seed + k)
        w, st = pkg.pcm_deemph_s16_host(x, alpha, gain, st)
        if k == 0 or not chain:
            g, est = pkg.pcm_deemph_s16_host(x, alpha, gain, est)
            g = g[0::2].astype(np.int32)
        else:
            g, est = emu.chain_emulate(x, alpha, gain, cuts=emu.run_cuts(M, A, runs, 5, overlap), state0=est)
        got.append(g)
        want.append(w[0::2].astype(np.int32))
    return np.concatenate(got), np.concatenate(want), est, st


def _hold(got, want, est, st, what):
    d = np.abs(got - want)
    assert d.max() <= 1, (what, int(d.max()), int(np.argmax(d)))
    assert (d > 0).mean() < 0.01, (what, float((d > 0).mean()))     # different only where y * gain sits on a rounding boundary
    assert abs(est - st) <= 1e-6 * max(abs(st), 0.25), (what, est, st)


@pytest.mark.parametrize("tau", [75e-6, 50e-6])
@pytest.mark.parametrize("run_len", [76, 400, 800, 1500])
def test_runs_sunk_on_their_own_are_within_one_lsb_of_the_exact_chain(pkg, tau, run_len):
    """Runs of 76 outputs (the shortest the host allows: 12 owned quads), 400 (BASELINE configs[2]), 800 (configs[3]'s share: two flushes per run) and 1500 (three)."""
    lib = pkg.load_library()
    alpha = float(lib.sdrfm_pcm_alpha(48000.0, tau))
    state = 0.0
    emu_state = 0.0
    for call in range(3):
        x = _audio(4800, 10 * call + int(tau * 1e6))
        want, state = pkg.pcm_deemph_s16_host(x, alpha, GAIN, state)
        got, emu_state = emu.chain_emulate(x, alpha, GAIN, run_len=run_len, state0=emu_state)
        d = np.abs(got - want[0::2].astype(np.int32))
        assert d.max() <= 1, (call, int(d.max()), int(np.argmax(d)))
        assert (d > 0).mean() < 0.01                              # different only where y * gain sits on a rounding boundary
        assert abs(emu_state - state) <= 1e-6 * max(abs(state), 0.25), (emu_state, state)


def test_full_scale_and_clipping(pkg):
    lib = pkg.load_library()
    alpha = float(lib.sdrfm_pcm_alpha(48000.0, 75e-6))
    x = (3.0 * _audio(4800, 3)).astype(np.float32)                  # drives the sink into its clamp
    want, _ = pkg.pcm_deemph_s16_host(x, alpha, GAIN)
    got, _ = emu.chain_emulate(x, alpha, GAIN)
    assert want.max() == 32767 and want.min() == -32768
    assert np.abs(got - want[0::2].astype(np.int32)).max() <= 1


def test_why_the_scheme_needs_a_short_memory(pkg):
    """(1 - alpha)^64 must be below rounding for a run's own end state to stand for the true one: at SDRFM_CHAIN_MIN_ALPHA it is 5e-8; at alpha = 0.05 (a 400 us time
    constant) a run's first 64 outputs are not all its predecessor reaches and the scheme is off by whole LSBs — which is why such a sink is served by the stand-alone
    kernel instead (sdrfm_sink_chain_params answers 1)."""
    assert (1.0 - 0.231) ** 64 <= 5.1e-8
    x = (_audio(4800, 9) + np.float32(0.8)).astype(np.float32)     # (a DC offset: a state that matters)
    want, _ = pkg.pcm_deemph_s16_host(x, 0.05, GAIN)
    got, _ = emu.chain_emulate(x, 0.05, GAIN, run_len=100)
    assert np.abs(got - want[0::2].astype(np.int32)).max() > 4


# ---- which alphas the chain serves ---------------------------------------------------------------------------------------------------------------------------
def test_the_chain_serves_alpha_from_0_231f_up_to_where_its_tables_stay_normal(pkg):
    """sdrfm_sink_chain_tables answers 2 for [0.231f, 1 - 1.8e-5] and 1 outside: the float below 0.231f (a run's end state would still depend on its
    predecessor's), and every alpha so close to 1 that (1 - alpha)^8 is subnormal or 0 — there dinv[7] = (1 - alpha)^-7 overflows or is about to."""
    lib = pkg.load_library()
    mode = {name: emu.chain_tables(pp.alpha_of(lib, name))[0] for name in pp.ALPHAS}
    assert sorted(n for n, m in mode.items() if m == 2) == sorted(pp.CHAIN_ALPHAS) and set(mode.values()) == {1, 2}, mode
    one = np.float32(1.0)
    for a, want in ((np.nextafter(one, np.float32(0)), 1), (np.float32(1 - 1e-6), 1), (np.float32(1 - 1e-5), 1), (np.float32(1 - 1.7e-5), 1),
                    (np.float32(1 - 1.9e-5), 2), (np.float32(1 - 1e-4), 2)):
        m, pc, w, dinv = emu.chain_tables(a)
        assert m == want, (float(a), m)
        if m == 2:
            assert pc >= np.finfo(np.float32).tiny and w[0] >= np.finfo(np.float32).tiny and np.isfinite(dinv).all(), (float(a), pc, w, dinv)
    m, pc, w, dinv = emu.chain_tables(1.0)
    assert pc == 0 and w.tolist() == [0] * 7 + [1] and dinv[0] == 1 and np.isinf(dinv[1:]).all()


def test_a_runs_last_flush_ends_off_a_multiple_of_eight_at_the_shapes_the_gpu_tests_run(pkg, plan_runs):
    """The written answer: can a run's last flush end off a multiple of 8 outputs at a shape design Q accepts?  Yes: every run of these calls does.  A run owns the audio outputs
    [floor(32 q0 / 5), floor(32 q1 / 5)) (quads of 32 decimated outputs, / 5), 83 to 90 of them here, sunk in one flush: no count is a multiple of 8.  So the publish multiplies
    the scan's value by dinv[k], k >= 1, and at alpha = 1 (dinv = inf, scan value 0) the chain WOULD publish NaN: shown here with the library's tables and its answer
    overridden.  Nothing in the geometry protects alpha = 1; sdrfm_sink_chain_tables' answer does."""
    lib = pkg.load_library()
    off, total = 0, 0
    for overlap in (False, True):
        for nbytes in PLAN_NBYTES[1:]:
            M, A, runs = plan_runs[nbytes]
            ends = emu.last_flush_ends(emu.run_cuts(M, A, runs, 5, overlap))
            assert all(e > 0 for e in ends), ends                  # (at these shapes every run publishes from its last flush's scan)
            off += sum(e % 8 != 0 for e in ends)
            total += len(ends)
    assert total == 68 and off == 68, (off, total)               # (11 + 23 runs, overlapped and not)
    assert emu.chain_tables(1.0)[0] == 1
    got, want, est, st = _emulate_plan(pkg, plan_runs, 1.0, GAIN, True, 40, force_chain=True)
    assert np.isnan(est)                                            # the carried word of the stream's next call
    assert (got != want).sum() >= 64                                # and the first 64 outputs of every run behind a NaN publish


# ---- every alpha the chain serves, at the launch's own cut ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name", pp.ALPHAS)
def test_the_launchs_own_runs_meet_the_host_routine_at_every_alpha(pkg, plan_runs, name, overlap):
    """Every alpha of the GPU sweep by the path the library takes for it: the chain (emulated at the launch's cut, the publish through dinv and the fix-up through
    dpow included) where sdrfm_sink_chain_tables answers 2, the sink's own kernel otherwise — at alpha = 1 and near it too."""
    lib = pkg.load_library()
    alpha = pp.alpha_of(lib, name)
    for gain in (GAIN, -GAIN, np.float32(0.0)):
        got, want, est, st = _emulate_plan(pkg, plan_runs, alpha, gain, overlap, 20)
        _hold(got, want, est, st, (name, float(gain)))


@pytest.mark.parametrize("alpha", [1 - 1.9e-5, 1 - 1e-4, 0.999])
def test_the_chain_just_below_its_upper_end_meets_the_host_routine(pkg, plan_runs, alpha):
    """The largest alphas the chain serves: (1 - alpha)^8 barely normal, dinv[7] up to 1e33; products that underflow in the scan are off by 2^-149 dinv[7] < 1e-11."""
    lib = pkg.load_library()
    alpha = float(np.float32(alpha))
    assert emu.chain_tables(alpha)[0] == 2
    got, want, est, st = _emulate_plan(pkg, plan_runs, alpha, GAIN, True, 30)
    _hold(got, want, est, st, alpha)


# ---- small calls at both audio decimations: every run owns what its predecessor's state reaches ----------------------------------------------------------------
@pytest.mark.parametrize("D,Da", [(10, 5), (8, 8), (16, 5)])
def test_every_run_of_a_small_chained_call_owns_more_than_its_predecessors_reach(pkg, runs_exe, D, Da):
    """A run publishes its end state from its own outputs alone and finishes its first FIX = 64 outputs with its predecessor's state: both need a run that owns more
    than 64 AUDIO outputs.  The host counted 13 quads of 32 decimated outputs per run at every rate — 76 audio outputs at Da = 5, but 48 at Da = 8: a 2.048 MS/s call
    of 832 decimated outputs went out as two runs of 52 audio outputs, and the state the sink carried lacked (1 - alpha)^52 of what came before the run (1.1e-6 of
    max(|st|, 0.25) on tests/test_q_taps_gpu.py's carriers, measured on the device and reproduced here before csrc/sdrfm_fm_call.h counted audio outputs).  264
    streams on 256 CUs, every call of 1 .. 52 units of 8 D Da samples: wherever the chain rides in the launch every run owns more than 64 audio outputs, and the
    state behind two such calls is the host routine's within 1e-6 max(|st|, 0.25)."""
    lib = pkg.load_library()
    alpha = pp.alpha_of(lib, "75us")
    unit = 8 * D * Da
    sizes = [2 * unit * k for k in range(1, 53)]
    r = subprocess.run([runs_exe, "7", str(D), "32", str(Da), "264", "256", "12"] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=60)
    chained, shortest, worst = 0, None, 0.0
    for line in r.stdout.splitlines():
        nbytes, M, A, q_fit, fits, runs, with_chain = (int(v) for v in line.split())
        if not q_fit:
            assert M < 2 * 128 and not with_chain, line             # (one step per stream does not fill the machine: the bit-exact kernels' call)
            continue
        if not with_chain:                                          # (a call too short for one such run: the sink's own kernel follows the launch)
            continue
        chained += 1
        for overlap in (False, True):
            cuts = emu.run_cuts(M, A, runs, Da, overlap)
            own = min(c["j1"] - c["jlo"] for c in cuts)
            shortest = own if shortest is None else min(shortest, own)
            assert own > emu.FIX, (line, overlap, [(c["jlo"], c["j1"]) for c in cuts])
        if runs >= 2 and A <= 400:                                  # the smallest calls of two runs and more: the emulated state against the host routine's
            st = est = 0.0
            for k in range(2):
                x = (_audio(A, 50 + k) + np.float32(0.5)).astype(np.float32)
                _, st = pkg.pcm_deemph_s16_host(x, alpha, GAIN, st)
                _, est = emu.chain_emulate(x, alpha, GAIN, cuts=emu.run_cuts(M, A, runs, Da, False), state0=est)
            worst = max(worst, abs(est - st) / max(abs(st), 0.25))
            assert abs(est - st) <= 1e-6 * max(abs(st), 0.25), (line, est, st)
    assert chained >= 40 and shortest is not None
    print("D %d Da %d: %d chained calls, the shortest run owns %d audio outputs; worst state difference %.3g of max(|st|, 0.25)" % (D, Da, chained, shortest, worst))
