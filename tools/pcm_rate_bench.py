#!/usr/bin/env python3
"""The cost of the PCM rate matcher at 256 streams x 4800 pairs per call, device-resident, one process, no retries, each case
alternating in one loop with the call it follows:
  (a) the stereo sink's default form (sdrfm_pcm_stereo_sink_process_batch) on the same shape — the yardstick, from the same run;
  (b) the matcher with the default table (32 taps, 256 phases) at step 2^32 (1 + 1e-4): drift-locked, 48 kHz in and out;
  (c) the matcher with the default table for 48 -> 44.1 kHz (cutoff 0.9 * 44.1 / 48) at step round(2^32 * 480 / 441).
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers, so that no call finds its input where the one before left it.  The last timed call of (b) and of (c) is held to the host routine.
Prints one JSON line; --out writes the same line to a file (profiles/pcm_rate_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/pcm_rate_bench.py, in a run of its own."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

pkg = importlib.import_module("stm32f7-rtlsdr_amd")
ROT = 4


def _pairs(cur, calls, first, second):
    """`calls` rounds of first(k), second(k) on stream cur, each between two events: the two arrays of device times in microseconds"""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    for k, e in enumerate(ev):
        e[0].record(cur)
        first(k)
        e[1].record(cur)
        e[2].record(cur)
        second(k)
        e[3].record(cur)
    torch.cuda.synchronize()
    return (np.array([e[0].elapsed_time(e[1]) * 1e3 for e in ev]), np.array([e[2].elapsed_time(e[3]) * 1e3 for e in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, n = 256, 4800
    lib = pkg.load_library()
    alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), 9000.0
    rng = np.random.default_rng(5)
    t = np.arange(n) / 48000.0
    tones = [np.sin(2 * np.pi * rng.uniform(200.0, 15e3, (ns, 1)) * t[None, :] + rng.uniform(0, 6.28, (ns, 1))).astype(np.float32) for _ in range(2 * ROT)]
    left = [torch.from_numpy(tones[r]).cuda() for r in range(ROT)]
    right = [torch.from_numpy(tones[ROT + r]).cuda() for r in range(ROT)]
    pcm = [torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda") for _ in range(ROT)]
    step_b, step_c = pkg.step_for(48000, 48000, 100.0), pkg.step_for(48000, 44100)
    coef_b, coef_c = pkg.rate_coef(step=step_b), pkg.rate_coef(step=step_c)
    sink = pkg.StereoPcmSink(ns, alpha, gain)
    rm_b, rm_c = pkg.PcmRateMatcher(ns, coef_b), pkg.PcmRateMatcher(ns, coef_c)
    rm_b.set_step(step_b)
    rm_c.set_step(step_c)
    out = torch.zeros((ns, 2 * (n + 2)), dtype=torch.int16, device="cuda")
    cur = torch.cuda.Stream()                                     # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (sink, rm_b, rm_c):
        k.set_stream(cur.cuda_stream)
    for r in range(ROT):                                          # the matchers' inputs: what the sink leaves of four programmes
        sink.process_batch_device(left[r], right[r], pcm[r], n)
    sink.synchronize()

    def f_a(k):
        sink.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], n)

    def f_b(k):
        rm_b.process_batch_device(pcm[k % ROT], out, n)

    def f_c(k):
        rm_c.process_batch_device(pcm[k % ROT], out, n)

    for k in range(a.warmup):
        f_a(k); f_b(k); f_a(k); f_c(k)
    torch.cuda.synchronize()
    t_a1, t_b = _pairs(cur, calls, f_a, f_b)
    t_a2, t_c = _pairs(cur, calls, f_a, f_c)
    # two more calls of either matcher from reset, the second held to the host routine carried over the same two rows
    sink.synchronize()
    x1, x0 = pcm[1].cpu().numpy(), pcm[0].cpu().numpy()
    for rm, coef, step in ((rm_b, coef_b, step_b), (rm_c, coef_c, step_c)):
        rm.reset()
        rm.process_batch_device(pcm[1], out, n)
        cnt = rm.process_batch_device(pcm[0], out, n)
        rm.synchronize()
        got = out.cpu().numpy()
        for s in (0, ns // 2, ns - 1):
            _, p1, h1 = pkg.pcm_rate_host(x1[s], coef, step)
            want, _, _ = pkg.pcm_rate_host(x0[s], coef, step, p1, h1)
            assert int(cnt[s]) == want.size // 2 and np.array_equal(got[s, :want.size], want), "the matcher's row %d differs from the host routine's" % s
    med = lambda v: float(np.median(v))
    spread = lambda tag, v: {tag + "_us_median": med(v), tag + "_p10": float(np.percentile(v, 10)), tag + "_p90": float(np.percentile(v, 90))}
    res = dict(metric="pcm_rate_us", shape="256x4800 pairs", calls=calls, rotate=ROT, kernel=rm_b.kernel_name, n_taps=int(coef_b.shape[1]),
               phases=int(coef_b.shape[0] - 1), step_b=step_b, step_c=step_c)
    res.update(spread("a_sink_beside_b", t_a1))
    res.update(spread("b_rate_drift", t_b))
    res.update(spread("a_sink_beside_c", t_a2))
    res.update(spread("c_rate_44k1", t_c))
    res.update(b_over_a=med(t_b) / med(t_a1), c_over_a=med(t_c) / med(t_a2))
    for k in (sink, rm_b, rm_c):
        k.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
