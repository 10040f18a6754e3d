#!/usr/bin/env python3
"""tools/pcm_chain_emulate.py — (CPU) the arithmetic of the PCM sink inside the demodulator's launch (csrc/sdrfm_sink_chain.h, the PCM block of csrc/sdrfm_q.hip's
flush_audio and the epilogue behind it), restated in numpy with the kernel's operation order.  Every run of a call is sunk on its own from state 0 — chunks of 8 per
lane, the chunk's contribution as a dot product with w[q] = alpha d^(7-q), six Hillis-Steele steps over the 64 lanes, the exact chain from the true carry-in —,
PUBLISHES its end state as the kernel does: from the scan of its last flush, sc[lane of the last output] * dinv[7 - (outputs in that lane's chunk - 1)], before the
second walk (a last flush with nothing in it: the state the earlier flushes left), finishes its first 64 outputs with fmaf(dpow[k], carry, y_local[k]), carry = what
its predecessor published, and hands its own published value on: to the next run, and behind the call's last run to the stream's next call.

The tables pc, w, dinv are the library's own (sdrfm_sink_chain_tables, plain host arithmetic: no device), and so is the answer whether the chain may serve an alpha.
The cut of a call into runs and of a run into flushes is the launch's: run_cuts() restates the run geometry at the top of q_wave (csrc/sdrfm_q.hip) for the number
of runs the host arithmetic of csrc/sdrfm_fm_call.h gives (tests/native/pcm_chain_runs.cpp prints it).  fixed_cuts() cuts at a fixed run length instead.
fp32 throughout (fused multiply-adds through float64: exact products, one rounding that differs from a true fma's in ~1e-9 of the cases).  Used by
tests/test_pcm_chain_cpu.py to hold the scheme to the host routine sdrfm_pcm_deemph_s16 within 1 LSB without a GPU, and to show why the scheme needs
(1 - alpha)^64 below rounding (SDRFM_CHAIN_MIN_ALPHA).  Run as a script: prints the comparison for 75 us / 50 us.
Test infrastructure: nothing here is on a product path."""
import ctypes as C

import numpy as np

F = np.float32
FIX, CH = 64, 8
WQB, ABS, STEP_OUT = 4, 4, 128          # csrc/sdrfm_q.hip: blocks (of 8 outputs) per quad, audio stages parked before a flush, outputs per step and per audio stage


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def pcm_word(v):
    c = np.clip(v.astype(F), F(-32768.0), F(32767.0))
    return np.rint(c).astype(np.int32)                           # (round-half-even, as the 1.5 * 2^23 addition does)


def _library():
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("stm32f7-rtlsdr_amd").load_library()


def chain_tables(alpha, lib=None):
    """sdrfm_sink_chain_tables: (2 = the chain may serve this alpha, 1 = the stand-alone kernel only; pc; w[8]; dinv[8]) as the launch's arguments hold them"""
    lib = _library() if lib is None else lib
    pc = C.c_float()
    w, dinv = (C.c_float * CH)(), (C.c_float * CH)()
    mode = lib.sdrfm_sink_chain_tables(C.c_float(alpha), C.byref(pc), w, dinv)
    return int(mode), F(pc.value), np.array(w[:], F), np.array(dinv[:], F)


# ---- the cut of a call into runs and flushes -----------------------------------------------------------------------------------------------------------------
def run_cuts(M, A, runs, Da, overlap):
    """Design Q's cut of one stream's call (M decimated outputs, A audio outputs, `runs` waves; overlap: the stream's first run warms up from the previous call's
    buffer): per run the audio outputs it owns [jlo, j1) and its flushes [(lo, hi)], the last of which is the run's last flush (fin; it may be empty: lo >= hi).
    q_wave's own integer arithmetic: runs are cut in quads of WQB blocks of 8 outputs, a run's step grid starts at its warm-up quad, an audio stage of 128 outputs
    follows every Da steps (and the last step), and the parked stages are flushed every ABS stages and behind the last step."""
    Bt = (M + 7) >> 3
    Qt = (Bt + WQB - 1) // WQB
    vs = 1 if overlap else 0
    Gq = Qt + runs - 1 + vs
    out = []
    for run in range(runs):
        e0, e1 = (run * Gq) // runs, ((run + 1) * Gq) // runs
        q0 = 0 if run == 0 else e0 - (run - 1 + vs)
        q1 = e1 - (run + vs)
        assert q0 < q1, "an empty run publishes nothing: its successor would wait in vain"
        warm = run > 0 or overlap
        b0, b1 = WQB * q0, min(WQB * q1, Bt)
        bs = b0 - WQB if warm else b0
        nsteps = (b1 - bs + 15) >> 4
        o0 = 8 * bs
        jg0 = o0 // Da                                             # (floor, also for the -32 of an overlapped call's first run)
        jlo = (o0 + 8 * WQB) // Da if warm else 0
        j1 = min((8 * b1) // Da, A)
        stages = (nsteps + Da - 1) // Da
        flushes, jfl, npend = [], jg0, 0
        for _ in range(stages):
            npend += 1
            if npend == ABS:
                flushes.append((max(jfl, jlo), min(j1, jfl + STEP_OUT * npend)))
                jfl += STEP_OUT * npend
                npend = 0
        flushes.append((max(jfl, jlo), min(j1, jfl + STEP_OUT * npend)))      # flush_audio(true), whatever is parked
        out.append(dict(jlo=jlo, j1=j1, flushes=flushes))
    # the runs tile [0, A): nothing sunk twice, nothing left out; a flush is one scan of the wave
    assert out[0]["jlo"] == 0 and out[-1]["j1"] == A and all(a["j1"] == b["jlo"] for a, b in zip(out, out[1:])), [(r["jlo"], r["j1"]) for r in out]
    for r in out:
        spans = [(lo, hi) for lo, hi in r["flushes"] if hi > lo]
        assert spans and spans[0][0] == r["jlo"] and spans[-1][1] == r["j1"] and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), r
        assert all(hi - lo <= 64 * CH for lo, hi in spans) and spans[0][1] - spans[0][0] >= min(FIX, r["j1"] - r["jlo"]), r
    return out


def fixed_cuts(n, run_len):
    """n outputs cut into runs of run_len (the last one takes a rest shorter than FIX: the host never leaves a run shorter than its predecessor's reach), flushes of
    512 outputs from the run's start"""
    out, pos = [], 0
    while pos < n:
        m = min(run_len, n - pos)
        if 0 < n - (pos + m) < FIX:
            m = n - pos
        out.append(dict(jlo=pos, j1=pos + m, flushes=[(q, min(q + 64 * CH, pos + m)) for q in range(pos, pos + m, 64 * CH)]))
        pos += m
    return out


def last_flush_ends(cuts):
    """outputs in the last flush of every run: the publish multiplies by dinv[0] = 1 only where this is a multiple of 8 (0: nothing is multiplied)"""
    return [max(r["flushes"][-1][1] - r["flushes"][-1][0], 0) for r in cuts]


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------------------------------------
def sink_flush(x, yrun, alpha, w, pc):
    """One flush of up to 512 outputs: (y of every output from the run's state so far, the state behind the last one by the second walk, the scan's values sc[64])"""
    n = x.size
    assert 0 < n <= 64 * CH
    xp = np.zeros(64 * CH, F)
    xp[:n] = x
    xr = xp.reshape(64, CH)
    sc = np.zeros(64, F)
    for q in range(CH):
        sc = fma(w[q], xr[:, q], sc)
    pw = F(pc)
    sc[0] = fma(pw, yrun, sc[0])
    d = 1
    while d < 64:
        o = np.concatenate([np.zeros(d, F), sc[:-d]])
        sn = fma(pw, o, sc)
        sc = np.where(np.arange(64) >= d, sn, sc).astype(F)
        pw = F(pw * pw)
        d <<= 1
    y = np.concatenate([[F(yrun)], sc[:-1]]).astype(F)
    ys = np.zeros((64, CH), F)
    valid = (np.arange(64)[:, None] * CH + np.arange(CH)[None, :]) < n
    for q in range(CH):
        yn = fma(alpha, (xr[:, q] - y).astype(F), y)
        ys[:, q] = yn
        y = np.where(valid[:, q], yn, y).astype(F)
    flat = ys.reshape(-1)[:n]
    return flat, F(flat[-1]), sc


def chain_emulate(x, alpha, gain, run_len=400, state0=0.0, cuts=None):
    """PCM (int32 values, one per output) and the state handed to the stream's next call, by the in-launch scheme, for one stream's call cut into `cuts` (run_cuts /
    fixed_cuts; None: fixed_cuts(x.size, run_len)).  The tables are taken whatever sdrfm_sink_chain_tables answers about alpha: the caller asks chain_tables()."""
    alpha, gain = F(alpha), F(gain)
    _, pc, w, dinv = chain_tables(alpha)
    with np.errstate(all="ignore"):
        dpow = np.power(1.0 - float(alpha), np.arange(1, FIX + 1, dtype=np.float64)).astype(F)
        x = np.asarray(x, F)
        cuts = fixed_cuts(x.size, run_len) if cuts is None else cuts
        assert cuts[-1]["j1"] == x.size
        out = np.zeros(x.size, np.int32)
        carry = F(state0)                                            # the predecessor's published end state
        for r in cuts:
            jlo, j1 = r["jlo"], r["j1"]
            yrun, ypub = F(0.0), None
            ys_all = np.zeros(j1 - jlo, F)
            for k, (lo, hi) in enumerate(r["flushes"]):
                if hi <= lo:
                    continue
                ys, yrun, sc = sink_flush(x[lo:hi], yrun, alpha, w, pc)
                ys_all[lo - jlo:hi - jlo] = ys
                if k == len(r["flushes"]) - 1:                       # fin: published from the scan, before the second walk
                    cntf = hi - lo
                    ypub = F(sc[(cntf - 1) // CH] * dinv[CH - 1 - (cntf - 1) % CH])
            if ypub is None:
                ypub = yrun                                          # (a last flush with nothing in it)
            nfix = min(FIX, j1 - jlo)
            ys_all[:nfix] = fma(dpow[:nfix], carry, ys_all[:nfix])   # the run's first outputs, finished with the predecessor's state
            out[jlo:j1] = pcm_word((ys_all * gain).astype(F))
            carry = ypub
    return out, float(carry)


def main():
    import importlib
    lib = _library()
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    rng = np.random.default_rng(5)
    t = np.arange(48000) / 48000.0
    x = (1.2 * np.sin(2 * np.pi * 1000 * t) + 0.5 * np.sin(2 * np.pi * 7300 * t) + 0.05 * rng.standard_normal(t.size)).astype(F)
    gain = F(32767.0 / (2 * np.pi * 75e3 / 240e3))
    for tau in (75e-6, 50e-6):
        alpha = float(lib.sdrfm_pcm_alpha(48000.0, tau))
        want, st = pkg.pcm_deemph_s16_host(x, alpha, gain)
        got, st2 = chain_emulate(x, alpha, gain)
        dd = np.abs(got - want[0::2].astype(np.int32))
        print("tau %.0f us: alpha %.4f, (1 - alpha)^64 = %.2e: max |PCM difference| %d LSB, %.3f %% of the outputs differ, state %.3e relative"
              % (tau * 1e6, alpha, (1 - alpha) ** 64, dd.max(), 100.0 * (dd > 0).mean(), abs(st2 - st) / max(abs(st), 0.25)))


if __name__ == "__main__":
    main()
