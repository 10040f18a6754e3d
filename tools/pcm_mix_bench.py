#!/usr/bin/env python3
"""The cost of the PCM mix bus at 256 inputs -> 256 buses x 4800 pairs per call, device-resident, one process, no retries, the
four kinds alternating in one loop:
  (a) the mixer with two slots per bus, both live on different stations at half gain each — what a crossfade costs while it runs;
  (b) the mixer with one slot per bus at unity — plain selection;
  (c) the sample-form limiter's call (LW = 6) on the same rows — the chain's neighbour;
  (d) a device-to-device copy of the 256 x 4800 x 4 output bytes — the least a selection could cost.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers, so that no call finds its input where the one before left it.  Behind the timed loop the last call's rows of (a) and (b) and the
records are held to the host routine.  Prints one JSON line; --out writes the same line to a file (profiles/pcm_mix_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/pcm_mix_bench.py, in a run of its own."""
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
KINDS = ("a_mix_two_slots", "b_mix_one_slot", "c_limiter", "d_copy_d2d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, n, slew = 256, 4800, 32
    rng = np.random.default_rng(7)
    t = np.arange(n) / 48000.0
    rows = []
    for _ in range(ROT):                                                   # programmes of two tones per channel at about - 12 dBFS
        f = rng.uniform(100.0, 12e3, (ns, 2, 2, 1))
        ph = rng.uniform(0, 6.28, (ns, 2, 2, 1))
        x = (4000.0 * np.sin(2 * np.pi * f * t + ph)).sum(axis=2)
        rows.append(np.ascontiguousarray(np.rint(x).astype(np.int16).transpose(0, 2, 1).reshape(ns, 2 * n)))
    pcm = [torch.from_numpy(r).cuda() for r in rows]
    out2, out1, out_l, out_c = (torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda") for _ in range(4))
    two, one = pkg.PcmMixer(ns, ns, 2, slew), pkg.PcmMixer(ns, ns, 1, slew)
    src2 = np.stack([np.arange(ns), (np.arange(ns) + 1) % ns], axis=1)
    two.set_routes(src2, "stereo")
    two.set_gains(16384, jump=True)
    one.set_routes(np.arange(ns)[:, None], "stereo")
    one.set_gains(32768, jump=True)
    lim = pkg.PcmLimiter(ns, 6, 4)
    cur = torch.cuda.Stream()                                              # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (two, one, lim):
        k.set_stream(cur.cuda_stream)

    def f_a(k):
        two.process_batch(pcm[k % ROT], out2, n)

    def f_b(k):
        one.process_batch(pcm[k % ROT], out1, n)

    def f_c(k):
        lim.process_batch_device(pcm[k % ROT], out_l, n)

    def f_d(k):
        with torch.cuda.stream(cur):
            out_c.copy_(pcm[k % ROT], non_blocking=True)

    fs = (f_a, f_b, f_c, f_d)
    for k in range(a.warmup):
        for f in fs:
            f(k)
    torch.cuda.synchronize()
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in fs] for _ in range(calls)]
    for k in range(calls):
        for j, f in enumerate(fs):
            ev[k][j][0].record(cur)
            f(k)
            ev[k][j][1].record(cur)
    torch.cuda.synchronize()
    times = [np.array([ev[k][j][0].elapsed_time(ev[k][j][1]) * 1e3 for k in range(calls)]) for j in range(len(fs))]
    # the last timed call against the host routine, and the records of every call
    last = rows[(calls - 1) % ROT]
    got2, got1 = out2.cpu().numpy(), out1.cpu().numpy()
    sl2, J2 = two.slots()
    want2, _ = pkg.pcm_mix_host(last, sl2, slew, 65536)
    assert J2 == 65536 and np.array_equal(got2, want2), "the two-slot mixer differs from the host routine"
    assert np.array_equal(got1, last) and np.array_equal(out_c.cpu().numpy(), last), "the one-slot mixer at unity is not the identity"
    rec2, rec1 = two.read(), one.read()
    total = a.warmup + calls
    assert (rec2["n"] == total * n).all() and (rec1["n"] == total * n).all() and not rec1["clipped_l"].any() and not rec1["clipped_r"].any()
    assert int(rec1["peak"].max()) == max(int(np.abs(r.astype(np.int64)).max()) for r in rows)
    med = lambda v: float(np.median(v))
    res = dict(metric="pcm_mix_us", shape="256 -> 256 x 4800 pairs", calls=calls, warmup=a.warmup, rotate=ROT, kernel=two.kernel_name(),
               bytes_two_slots=3 * ns * n * 4, bytes_one_slot=2 * ns * n * 4, bytes_copy=2 * ns * n * 4)
    for tag, v in zip(KINDS, times):
        res.update({tag + "_us_median": med(v), tag + "_p10": float(np.percentile(v, 10)), tag + "_p90": float(np.percentile(v, 90))})
    res.update(a_over_copy=med(times[0]) / med(times[3]), b_over_copy=med(times[1]) / med(times[3]), a_over_limiter=med(times[0]) / med(times[2]),
               a_gb_per_s=3 * ns * n * 4 / med(times[0]) / 1e3, b_gb_per_s=2 * ns * n * 4 / med(times[1]) / 1e3)
    for k in (two, one, lim):
        k.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
