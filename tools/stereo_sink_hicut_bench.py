#!/usr/bin/env python3
"""What the stereo PCM sink's ramped high-cut costs, at 256 streams x 4800 samples per call, device-resident, one process, no
retries, every pair alternating in one loop (tools/stereo_sink_bench.py's method):
  (a) the plain default form, a sink that was never conditioned — the yardstick: unchanged code;
  (b) the conditioned default form, every stream in mid-ramp in every timed call (half the streams up, half down, slew 1 between 1024 and 32768:
      31 744 samples to the end, turned round before every third call so that no call sees a finished ramp);
  (c) sdrfm_bcast_process_batch_pcm with a plain sink (256 x 240 000 samples, T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25);
  (d) the same call with a conditioned sink, its ramps likewise running.
Each figure is the median over the timed calls of the device time between two events around one call, with p10 and p90.  Every timed call starts
on an empty queue; the turn of the ramps (a host-side wait and a 1 KiB copy) happens outside the events.
Prints one JSON line; --out writes the same line to a file (profiles/stereo_sink_hicut_bench.json)."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

pkg = importlib.import_module("stm32f7-rtlsdr_amd")


def _timed(cur, calls, fns, before):
    """`calls` rounds over fns, each call between two events on stream cur, before[k]() (or None) ahead of its first event: one array of device
    times in microseconds per function"""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(calls)]
    for row in ev:
        for (e0, e1), fn, pre in zip(row, fns, before):
            if pre is not None:
                pre()
            e0.record(cur)
            fn()
            e1.record(cur)
    torch.cuda.synchronize()
    return [np.array([row[k][0].elapsed_time(row[k][1]) * 1e3 for row in ev]) for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
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
    plain, cond = pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)
    call_plain, call_cond = pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)
    cur = torch.cuda.Stream()                                     # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (bc, plain, cond):
        k.set_stream(cur.cuda_stream)
    bc.process_batch_device(iq, left, right, bb, pc)              # the sinks' input: a station's L and R
    lo = np.where(np.arange(ns) % 2 == 1, 32768, 1024).astype(np.uint16)
    hi = np.where(np.arange(ns) % 2 == 1, 1024, 32768).astype(np.uint16)

    def running(sink, sync):
        """what runs ahead of a timed call, outside its events: wait for the queue, and before every third call turn the ramps round — up three
        calls (14 400 units), down three, the last step on a call's last sample — so that h moves at every sample of every timed call"""
        assert lib.sdrfm_pcm_stereo_sink_set_hicut(sink._h, lo.ctypes.data, 32768) == 0
        sink.reset()                                              # (completes the jump: every stream stands at its end of the range)
        count = [0]

        def go():
            sync()
            if count[0] % 3 == 0:
                q = hi if count[0] % 6 == 0 else lo
                st = lib.sdrfm_pcm_stereo_sink_set_hicut(sink._h, q.ctypes.data, 1)
                assert st == 0, st
            count[0] += 1
            now, target, slew = sink.hicut_state()
            assert slew == 1 and np.all(now != target), "a timed call would start on a finished ramp"
        return go

    def f_a():
        plain.process_batch_device(left, right, pcm, na)

    def f_b():
        cond.process_batch_device(left, right, pcm, na)

    def f_c():
        bc.process_batch_pcm_device(call_plain, iq, left, right, pcm, bb, pc)

    def f_d():
        bc.process_batch_pcm_device(call_cond, iq, left, right, pcm, bb, pc)

    pre_b, pre_d = running(cond, cur.synchronize), running(call_cond, bc.synchronize)
    for _ in range(a.warmup):
        f_a(); pre_b(); f_b(); f_c(); pre_d(); f_d()
    torch.cuda.synchronize()
    t_a, t_b = _timed(cur, calls, (f_a, f_b), (cur.synchronize, pre_b))   # (every timed call starts on an empty queue, (a) and (c) too)
    t_c, t_d = _timed(cur, calls, (f_c, f_d), (bc.synchronize, pre_d))
    med = lambda t: float(np.median(t))
    out = dict(metric="stereo_sink_hicut_us", shape="256x4800 (sink), 256x240000 T64 D10 P101 Ta32 Da5 Tr255 Dr25 (bcast)", calls=calls,
               bcast_kernel=bc.kernel_name,
               a_plain_sink_us_median=med(t_a), a_p10=float(np.percentile(t_a, 10)), a_p90=float(np.percentile(t_a, 90)),
               b_hicut_sink_us_median=med(t_b), b_p10=float(np.percentile(t_b, 10)), b_p90=float(np.percentile(t_b, 90)),
               c_bcast_pcm_plain_us_median=med(t_c), c_p10=float(np.percentile(t_c, 10)), c_p90=float(np.percentile(t_c, 90)),
               d_bcast_pcm_hicut_us_median=med(t_d), d_p10=float(np.percentile(t_d, 10)), d_p90=float(np.percentile(t_d, 90)),
               b_over_a=med(t_b) / med(t_a), d_minus_c_us=med(t_d) - med(t_c))
    for k in (plain, cond, call_plain, call_cond, bc):
        k.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
