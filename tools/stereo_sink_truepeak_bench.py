#!/usr/bin/env python3
"""The cost of the stereo PCM sink's true-peak meter at 256 streams x 4800 samples per call, device-resident, one process, no
retries, the kinds alternating in one loop:
  (a) the stereo sink's default form on a plain sink — true peak disabled, the yardstick;
  (m) the same call on a sink with the audio meter (§4.20) alone — the first figure the add-on is reported against;
  (t) the same call with true peak enabled (the BS.1770-4 table, -1 dBTP): the sink's launch and k_pcm_truepeak behind it;
  (c) the same call with the audio meter, the loudness meter and true peak enabled;
  (h) the plain call followed by a copy of the same 256 PCM rows into pinned host memory — the alternative to metering on the device, and
      only its transfer: oversampling the rows on the host comes on top.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers, so that no call finds its input where the one before left it.  The last true-peak call's records are checked against the host
routine on the PCM the calls left.  On a tree without the true-peak meter (the parent commit) the kinds (a), (m) and (h) alone are timed:
--parent FILE merges such a run's line, so that one file holds the plain call's time before and after.  Prints one JSON line; --out writes
the same line to a file (profiles/stereo_sink_truepeak_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/stereo_sink_truepeak_bench.py, in a run of its own."""
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


def _group(cur, calls, fns):
    """`calls` rounds of every function of fns in turn on stream cur, each between two events: one array of device times in microseconds per function"""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(calls)]
    for k, row in enumerate(ev):
        for f, (e0, e1) in zip(fns, row):
            e0.record(cur)
            f(k)
            e1.record(cur)
    torch.cuda.synchronize()
    return [np.array([row[i][0].elapsed_time(row[i][1]) * 1e3 for row in ev]) for i in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None, help="the JSON line of a run of this tool on the parent commit: merged in under parent_*")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, na = 256, 4800
    have = hasattr(pkg.StereoPcmSink, "enable_truepeak")
    lib = pkg.load_library()
    alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    rng = np.random.default_rng(7)
    t = np.arange(na) / 48000.0
    left, right = [], []
    for r in range(ROT):                                          # programme-like rows: a few tones and noise per stream, a few dB under full scale
        f = rng.uniform(50.0, 15000.0, (ns, 3, 1))
        x = (np.sin(2 * np.pi * f * t[None, None, :] + rng.uniform(0, 6.28, (ns, 3, 1))).sum(axis=1) / 3 + 0.1 * rng.standard_normal((ns, na))) * 1.3
        left.append(torch.from_numpy(x.astype(np.float32)).cuda())
        right.append(torch.from_numpy(np.roll(x, 7, axis=1).astype(np.float32)).cuda())
    pcm = [torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda") for _ in range(ROT)]
    host = torch.zeros((ns, 2 * na), dtype=torch.int16).pin_memory()
    new = lambda: pkg.StereoPcmSink(ns, alpha, gain)
    plain, meter, copy = new(), new(), new()
    sinks = [plain, meter, copy]
    cur = torch.cuda.Stream()                                     # every sink and the events on one stream of our own
    torch.cuda.synchronize()
    meter.enable_meter(8)
    if have:
        tp, every = new(), new()
        sinks += [tp, every]
        tp.enable_truepeak()
        every.enable_meter(8)
        every.enable_loudness(4800, 64)
        every.enable_truepeak()
    for s in sinks:
        s.set_stream(cur.cuda_stream)
    sink_call = lambda s: (lambda k: s.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], na))

    def copy_call(k):
        copy.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], na)
        with torch.cuda.stream(cur):
            host.copy_(pcm[k % ROT], non_blocking=True)

    names = ["a_sink", "m_sink_meter", "h_sink_copy_to_host"] + (["t_sink_truepeak", "c_sink_all_three"] if have else [])
    fns = [sink_call(plain), sink_call(meter), copy_call] + ([sink_call(tp), sink_call(every)] if have else [])
    for k in range(a.warmup):
        for f in fns:
            f(k)
    torch.cuda.synchronize()
    times = dict(zip(names, _group(cur, calls, fns)))
    med = lambda v: float(np.median(v))
    out = dict(metric="stereo_sink_truepeak_us", shape="256x4800", calls=calls, rotate=ROT, truepeak=have)
    for name in names:
        v = times[name]
        out[name + "_us_median"], out[name + "_p10"], out[name + "_p90"] = med(v), float(np.percentile(v, 10)), float(np.percentile(v, 90))
    base = med(times["a_sink"])
    out.update(m_minus_a_us=med(times["m_sink_meter"]) - base, h_minus_a_us=med(times["h_sink_copy_to_host"]) - base)
    if have:
        # n counts every call since enable; one more call's records are what the host routine makes of the PCM it left
        tp.synchronize()
        got = tp.read_truepeak()
        total = a.warmup + calls
        assert (got["n"] == total * na).all(), "n"
        before = pcm[(calls - 1) % ROT].cpu().numpy()               # what the last timed call left: the next call's lead-in is its tail
        tp.process_batch_device(left[0], right[0], pcm[0], na)      # one more call, onto the zeroed records
        tp.synchronize()
        last = tp.read_truepeak()
        _, hist = pkg.pcm_truepeak_host(before)
        want, _ = pkg.pcm_truepeak_host(pcm[0].cpu().numpy(), hist=hist)
        assert last.tobytes() == want.tobytes(), "the records differ from the host routine's"
        rep = pkg.truepeak_report(got)
        d = med(times["t_sink_truepeak"]) - base
        out.update(t_minus_a_us=d, c_minus_a_us=med(times["c_sink_all_three"]) - base, t_over_a=med(times["t_sink_truepeak"]) / base,
                   truepeak_over_meter_addon=d / out["m_minus_a_us"], truepeak_over_copy_addon=d / out["h_minus_a_us"],
                   max_dbtp=float(np.max(rep["dbtp"])))
    if a.parent:
        with open(a.parent) as f:
            par = json.loads(f.read().strip().splitlines()[-1])
        for k in ("a_sink", "m_sink_meter", "h_sink_copy_to_host"):
            for suffix in ("_us_median", "_p10", "_p90"):
                out["parent_" + k + suffix] = par[k + suffix]
        out["a_minus_parent_a_us"] = out["a_sink_us_median"] - par["a_sink_us_median"]
    for s in sinks:
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
