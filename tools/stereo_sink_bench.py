#!/usr/bin/env python3
"""The device stereo PCM sink at 256 streams x 4800 samples per call (BASELINE configs[2]'s audio), device-resident, one process,
no retries, every pair alternating in one loop:
  (a) the stereo sink's default form, one launch over L and R;
  (b) two mono sdrfm_pcm_sink_process_batch launches back to back, one over the L rows and one over the R rows — the yardstick;
  (c) sdrfm_bcast_process_batch alone (256 x 240 000 samples, T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25);
  (d) sdrfm_bcast_process_batch_pcm: (c) and the sink behind it on the handle's stream.
Each figure is the median over the timed launches of the device time between two events around one launch (for (b): around the two).  The *_queued
figures time windows of 20 launches between two events, per launch: what a launch costs in a queue that is never empty.
Prints one JSON line; --out writes the same line to a file (profiles/stereo_sink_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/stereo_sink_bench.py, in a run of its own."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

pkg = importlib.import_module("stm32f7-rtlsdr_amd")


def _pairs(cur, calls, first, second):
    """`calls` rounds of first(), second() on stream cur, each between two events: the two arrays of device times in microseconds"""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    for e in ev:
        e[0].record(cur)
        first()
        e[1].record(cur)
        e[2].record(cur)
        second()
        e[3].record(cur)
    torch.cuda.synchronize()
    return (np.array([e[0].elapsed_time(e[1]) * 1e3 for e in ev]), np.array([e[2].elapsed_time(e[3]) * 1e3 for e in ev]))


def _queued(cur, windows, per, fn):
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        for _ in range(per):
            fn()
        e1.record(cur)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed launches of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, nsamp = 256, 240000
    lib = pkg.load_library()
    alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    h, g = pkg.default_config(64)
    iq = torch.from_numpy(pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 75e3, first_id=1)).cuda()
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), pilot_min=0.05, diff_gain=pkg.stereo_diff_gain(10, 2.4e6),
                                                rds_gain=pkg.rds_gain(10, 2.4e6), n_streams=ns, max_bytes_per_call=2 * nsamp))
    na, nr = bc.counts(2 * nsamp)
    assert na == 4800, na
    left = torch.zeros((ns, na), dtype=torch.float32, device="cuda")
    right = torch.zeros_like(left)
    bb = torch.zeros((ns, 2 * nr), dtype=torch.float32, device="cuda")
    pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
    pcm = torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda")
    pcm_l, pcm_r = torch.zeros_like(pcm), torch.zeros_like(pcm)
    stereo = pkg.StereoPcmSink(ns, alpha, gain)
    call_sink = pkg.StereoPcmSink(ns, alpha, gain)                  # the one-call form's
    mono_l, mono_r = pkg.PcmSink(ns, alpha, gain), pkg.PcmSink(ns, alpha, gain)
    cur = torch.cuda.Stream()                                     # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (bc, stereo, mono_l, mono_r):
        k.set_stream(cur.cuda_stream)
    bc.process_batch_device(iq, left, right, bb, pc)              # the sinks' input: a station's L and R

    def f_a():
        stereo.process_batch_device(left, right, pcm, na)

    def f_b():
        mono_l.process_batch_device(left, pcm_l, na)
        mono_r.process_batch_device(right, pcm_r, na)

    def f_c():
        bc.process_batch_device(iq, left, right, bb, pc)

    def f_d():
        bc.process_batch_pcm_device(call_sink, iq, left, right, pcm, bb, pc)

    for _ in range(a.warmup):
        f_a(); f_b(); f_c(); f_d()
    torch.cuda.synchronize()
    t_a, t_b = _pairs(cur, calls, f_a, f_b)
    t_c, t_d = _pairs(cur, calls, f_c, f_d)
    q_a, q_b = _queued(cur, 10, 20, f_a), _queued(cur, 10, 20, f_b)
    med = lambda t: float(np.median(t))
    out = dict(metric="stereo_sink_us", shape="256x4800 (sink), 256x240000 T64 D10 P101 Ta32 Da5 Tr255 Dr25 (bcast)", calls=calls,
               bcast_kernel=bc.kernel_name,
               a_stereo_sink_us_median=med(t_a), a_p10=float(np.percentile(t_a, 10)), a_p90=float(np.percentile(t_a, 90)),
               b_two_mono_sinks_us_median=med(t_b), b_p10=float(np.percentile(t_b, 10)), b_p90=float(np.percentile(t_b, 90)),
               c_bcast_us_median=med(t_c), c_p10=float(np.percentile(t_c, 10)), c_p90=float(np.percentile(t_c, 90)),
               d_bcast_pcm_us_median=med(t_d), d_p10=float(np.percentile(t_d, 10)), d_p90=float(np.percentile(t_d, 90)),
               a_over_b=med(t_a) / med(t_b), d_minus_c_us=med(t_d) - med(t_c),
               a_queued_us_median=med(q_a), b_queued_us_median=med(q_b))
    for k in (stereo, call_sink, mono_l, mono_r, bc):
        k.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
