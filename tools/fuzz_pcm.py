#!/usr/bin/env python3
"""tools/fuzz_pcm.py [seconds=120] [seed=1] [mode=calls|lifecycle] — soak of sdrfm_process_batch_pcm (the PCM sink inside the demodulator's launch,
csrc/sdrfm_sink_chain.h).

mode=calls (the default): a fresh handle and a fresh sink per case; random stream counts, call lengths, call styles (overlapped or not, with or without an audio
buffer), time constants and routed streams; every call's PCM of a few streams against the host routine sdrfm_pcm_deemph_s16 carried over the calls' audio (1 LSB),
and the sink must report no chain error.  This mode checks the sink against the audio the launches wrote, not the audio against the oracle.

mode=lifecycle: ONE handle for the whole soak, its stream continuing from case to case; before each burst of calls a random event — nothing, sdrfm_pcm_sink_reset,
the sink destroyed and a new one created, or stand-alone sink calls among the burst's calls —, a random length per call.  A few streams are held to the ORACLE:
their audio (when the call writes it) within 1e-5, their PCM within 2 LSB of the host routine run over the oracle's audio, the state restarted at every reset or
new sink (tests/test_pcm_sink_lifecycle_gpu.py states the tolerances).

Prints one summary line; exit status 1 on a failure."""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lifecycle(budget, rng, pkg, lib, h, g):
    import torch
    from oracle.oracle import Oracle
    t0 = time.time()
    ns = int(rng.choice([64, 128, 256, 512]))
    alpha, gain = float(lib.sdrfm_pcm_alpha(48000.0, 75e-6)), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    unit, lmax = 400, 320000                                                     # samples: 8 audio periods; the longest call
    check = sorted({0, 3, ns - 1})                                               # (stream s carries row s % 8)
    orc = {s: Oracle(h, g) for s in check}
    st = {s: 0.0 for s in check}
    cases = calls = fused = events = 0
    worst, worst_a = 0, 0.0
    prev_iq = None                  # the previous burst's capture: the next burst's first overlapped call warms up from its last call's rows, which must stay intact
    sink = pkg.PcmSink(ns, alpha, gain)
    try:
        with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, max_bytes_per_call=2 * lmax)) as dm:
            while time.time() - t0 < budget:
                ev = str(rng.choice(["none", "reset", "new", "standalone"]))
                dm.synchronize()
                if ev == "reset":
                    sink.reset()
                elif ev == "new":
                    sink.close()
                    sink = pkg.PcmSink(ns, alpha, gain)
                if ev in ("reset", "new"):
                    st = {s: 0.0 for s in check}
                events += int(ev != "none")
                lens = [int(unit * rng.integers(20, lmax // unit + 1)) for _ in range(int(rng.integers(3, 9)))]
                rows = pkg.make_iq(8, sum(lens), mode="fm", first_id=int(rng.integers(1, 1 << 20)))
                iq = torch.from_numpy(rows).cuda().repeat(ns // 8, 1)
                style = [("standalone" if ev == "standalone" and rng.random() < 0.4 else "chain", bool(rng.random() < 0.8), bool(rng.random() < 0.6))
                         for _ in lens]
                audio = [torch.zeros((ns, n // 50), dtype=torch.float32, device="cuda") for n in lens]
                pcm = [torch.zeros((ns, 2 * (n // 50)), dtype=torch.int16, device="cuda") for n in lens]
                torch.cuda.synchronize()
                off, nas, names = 0, [], []
                for k, n in enumerate(lens):
                    kind, ovl, with_audio = style[k]
                    if kind == "standalone":                               # (the header's order between the two styles: both synchronised)
                        dm.synchronize(); sink.synchronize()
                        na = dm.process_batch_device(iq[:, 2 * off:], audio[k], nbytes=2 * n)
                        dm.synchronize()
                        sink.process_batch_device(audio[k], pcm[k], na)
                        sink.synchronize()
                    else:
                        na = dm.process_batch_pcm_device(sink, iq[:, 2 * off:], audio[k] if with_audio else None, pcm[k], nbytes=2 * n, overlap=ovl)
                        fused += int("+ pcm" in dm.kernel_name)
                    names.append((ev, kind, dm.kernel_name, ovl, with_audio, n))
                    nas.append(na)
                    off += n
                    calls += 1
                dm.synchronize()
                if sink.synchronize_status() != 0:
                    print("FAIL: the sink reports a chain error (case %d, event %s)" % (cases, ev))
                    return 1
                got_p = [p.cpu().numpy() for p in pcm]
                got_a = [a.cpu().numpy() for a in audio]
                for s in check:
                    want_a = orc[s].process(rows[s % 8])
                    if want_a.size != sum(nas):
                        print("FAIL: case %d: the oracle made %d outputs, the calls %d" % (cases, want_a.size, sum(nas)))
                        return 1
                    o = 0
                    for k, na in enumerate(nas):
                        w = want_a[o:o + na]
                        o += na
                        if style[k][0] == "standalone" or style[k][2]:
                            a = got_a[k][s][:na].astype(np.float64)
                            e = float(np.max(np.abs(a - w) / np.maximum(np.abs(w), 1.0))) if na else 0.0
                            worst_a = max(worst_a, e)
                            if e > 1e-5:
                                print("FAIL: case %d call %d stream %d: audio %.3g off the oracle (%s)" % (cases, k, s, e, names[k]))
                                return 1
                        want, st[s] = pkg.pcm_deemph_s16_host(w, alpha, gain, st[s])
                        d = np.abs(got_p[k][s][:2 * na].astype(np.int32) - want.astype(np.int32))
                        worst = max(worst, int(d.max()) if na else 0)
                        if na and d.max() > 2:
                            bad = np.nonzero(d[0::2] > 2)[0]
                            print("FAIL: case %d call %d stream %d: %d LSB off the host routine over the oracle's audio; outputs %s ... (%d of %d)"
                                  % (cases, k, s, int(d.max()), bad[:8], bad.size, na))
                            for i, nm in enumerate(names):
                                print("  call %d: %s" % (i, nm))
                            return 1
                prev_iq = iq
                cases += 1
    finally:
        sink.close()
    print("fuzz_pcm lifecycle: %d streams, %d cases, %d sink events, %d calls (%d with the chain inside the launch), worst %d LSB and %.3g audio against the oracle, "
          "0 failures, %.0f s" % (ns, cases, events, calls, fused, worst, worst_a, time.time() - t0))
    return 0


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    mode = sys.argv[3] if len(sys.argv) > 3 else "calls"
    import torch
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    lib = pkg.load_library()
    h, g = pkg.default_config(64)
    if mode == "lifecycle":
        return lifecycle(budget, rng, pkg, lib, h, g)
    assert mode == "calls", mode
    t0 = time.time()
    cases = calls = fused = 0
    worst = 0
    while time.time() - t0 < budget:
        ns = int(rng.choice([int(x) for x in os.environ["FUZZ_PCM_NS"].split(",")] if os.environ.get("FUZZ_PCM_NS") else [16, 48, 128, 256, 384, 512]))
        tau = float(rng.choice([75e-6, 50e-6]))
        alpha, gain = float(lib.sdrfm_pcm_alpha(48000.0, tau)), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
        unit = 400                                                                  # samples: 8 audio periods
        lens = [int(unit * rng.integers(20, 700)) for _ in range(int(rng.integers(3, 9)))]
        total = sum(lens)
        rows = pkg.make_iq(8, total, mode="fm", first_id=int(rng.integers(1, 1 << 20)))
        if rng.random() < 0.3:
            rows[3] = pkg.make_iq(1, total, mode="random", first_id=int(rng.integers(1, 1 << 20)))[0]
        iq = torch.from_numpy(rows).cuda().repeat(ns // 8, 1)
        namax = max(lens) // 50
        audio = [torch.zeros((ns, namax + int(rng.integers(0, 3))), dtype=torch.float32, device="cuda") for _ in range(len(lens))]
        pcm = [torch.zeros((ns, 2 * namax + 2 * int(rng.integers(0, 3))), dtype=torch.int16, device="cuda") for _ in range(len(lens))]
        torch.cuda.synchronize()
        check = [0, 3, ns - 1]
        with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, max_bytes_per_call=2 * max(lens))) as dm, pkg.PcmSink(ns, alpha, gain) as sink:
            off = 0
            host_state = {s: 0.0 for s in check}
            pending = []
            names = []
            for k, n in enumerate(lens):
                ovl = bool(rng.random() < 0.8)
                with_audio = bool(rng.random() < 0.6)
                if rng.random() < 0.1:
                    m = np.zeros(ns, np.uint8)
                    if rng.random() < 0.5:
                        m[3::8] = 1
                    dm.route(m)
                na = dm.process_batch_pcm_device(sink, iq[:, 2 * off:], audio[k], pcm[k], nbytes=2 * n, overlap=ovl) if with_audio else None
                if not with_audio:
                    # (no audio buffer: the reference audio comes from a second, plain handle below)
                    na = dm.process_batch_pcm_device(sink, iq[:, 2 * off:], None, pcm[k], nbytes=2 * n, overlap=ovl)
                fused += int("+ pcm" in dm.kernel_name)
                names.append((dm.kernel_name, ovl, with_audio, n))
                pending.append((k, off, n, na, with_audio))
                off += n
                calls += 1
            dm.synchronize()
            if sink.synchronize_status() != 0:
                print("FAIL: the sink reports a chain error (case %d)" % cases)
                return 1
        # the audio of the calls made without a buffer: the same capture through a plain handle, call by call
        need_ref = any(not p[4] for p in pending)
        ref = {}
        if need_ref:
            with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, max_bytes_per_call=2 * max(lens))) as d2:
                for (k, off_k, n, na, with_audio) in pending:
                    a = torch.zeros((ns, namax + 2), dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()                       # (the fill runs on torch's stream, the call on the handle's own: without this the fill may land on
                                                                   # top of the call's audio — seen once in ~100 000 calls as a stretch of zeros in the REFERENCE)
                    d2.process_batch_device(iq[:, 2 * off_k:], a, nbytes=2 * n)
                    d2.synchronize()
                    ref[k] = a[:, :na].cpu().numpy()
        for (k, off_k, n, na, with_audio) in pending:
            a = audio[k][:, :na].cpu().numpy() if with_audio else ref[k]
            p = pcm[k].cpu().numpy()
            for s in check:
                want, host_state[s] = pkg.pcm_deemph_s16_host(a[s], alpha, gain, host_state[s])
                d = int(np.abs(p[s][:2 * na].astype(np.int32) - want.astype(np.int32)).max())
                worst = max(worst, d)
                # (a call without an audio buffer is checked against another handle's audio, which routed streams' calls may serve by other kernels: within the
                # audio's own tolerance the PCM may then differ by more than the scan's 1 LSB; those calls are held to 2 LSB)
                if d > (1 if with_audio else 2):
                    print("FAIL: case %d call %d stream %d: %d LSB (ns %d, n %d, audio buffer %s)" % (cases, k, s, d, ns, n, with_audio))
                    dd = np.abs(p[s][:2 * na].astype(np.int32) - want.astype(np.int32))[0::2]
                    bad = np.nonzero(dd > 2)[0]
                    print("  outputs off by more than 2 LSB: %d of %d, first %s, last %s; got there %s, want %s" % (bad.size, na, bad[:8], bad[-4:], p[s][2 * bad[:6]], want[2 * bad[:6]]))
                    for i, nm in enumerate(names):
                        print("  call %d: %s" % (i, nm))
                    return 1
        cases += 1
    print("fuzz_pcm: %d cases, %d calls (%d with the chain inside the launch), worst %d LSB, 0 failures, %.0f s" % (cases, calls, fused, worst, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
