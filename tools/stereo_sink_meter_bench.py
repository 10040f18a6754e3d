#!/usr/bin/env python3
"""The cost of the stereo PCM sink's audio meter at 256 streams x 4800 samples per call, device-resident, one process, no
retries, the two cases of every pair alternating in one loop:
  (a) the stereo sink's default form on an unmetered sink — the yardstick of (b), from the same run;
  (b) the same call on a metered sink: the sink's launch and the meter kernel behind it;
  (c) sdrfm_bcast_process_batch_pcm with an unmetered sink (256 x 240 000 samples, T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25);
  (d) the same call with a metered sink.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers, so that no call finds its input where the one before left it.  Prints one JSON line; --out writes the same line to a file
(profiles/stereo_sink_meter_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/stereo_sink_meter_bench.py, in a run of its own."""
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
    ap.add_argument("--quiet-lsb", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, nsamp = 256, 240000
    lib = pkg.load_library()
    alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    h, g = pkg.default_config(64)
    iq0 = torch.from_numpy(pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 75e3, first_id=1)).cuda()
    iq = [iq0] + [torch.roll(iq0, r, 0).contiguous() for r in range(1, ROT)]
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), pilot_min=0.05, diff_gain=pkg.stereo_diff_gain(10, 2.4e6),
                                                rds_gain=pkg.rds_gain(10, 2.4e6), n_streams=ns, max_bytes_per_call=2 * nsamp))
    na, nr = bc.counts(2 * nsamp)
    assert na == 4800, na
    left = [torch.zeros((ns, na), dtype=torch.float32, device="cuda") for _ in range(ROT)]
    right = [torch.zeros_like(left[0]) for _ in range(ROT)]
    bb = torch.zeros((ns, 2 * nr), dtype=torch.float32, device="cuda")
    pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
    pcm = [torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda") for _ in range(ROT)]
    plain, metered = pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)
    call_plain, call_metered = pkg.StereoPcmSink(ns, alpha, gain), pkg.StereoPcmSink(ns, alpha, gain)     # the one-call forms'
    cur = torch.cuda.Stream()                                     # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (bc, plain, metered):
        k.set_stream(cur.cuda_stream)
    for k in (metered, call_metered):
        k.enable_meter(a.quiet_lsb)
    for r in range(ROT):                                          # the sinks' inputs: four stations' L and R
        bc.process_batch_device(iq[r], left[r], right[r], bb, pc)
    bc.synchronize()
    bc.reset()

    def f_a(k):
        plain.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], na)

    def f_b(k):
        metered.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], na)

    def f_c(k):
        bc.process_batch_pcm_device(call_plain, iq[k % ROT], left[0], right[0], pcm[k % ROT], bb, pc)

    def f_d(k):
        bc.process_batch_pcm_device(call_metered, iq[k % ROT], left[0], right[0], pcm[k % ROT], bb, pc)

    for k in range(a.warmup):
        f_a(k); f_b(k); f_c(k); f_d(k)
    torch.cuda.synchronize()
    t_a, t_b = _pairs(cur, calls, f_a, f_b)
    t_c, t_d = _pairs(cur, calls, f_c, f_d)
    bc.synchronize()
    # the records are what the host routine makes of the PCM the last metered call left
    rec = metered.read_meters()
    metered.process_batch_device(left[0], right[0], pcm[0], na)
    metered.synchronize()
    want = pkg.pcm_audio_meter_host(pcm[0].cpu().numpy(), a.quiet_lsb)
    assert metered.read_meters().tobytes() == want.tobytes() and int(rec["n"][0]) == (a.warmup + calls) * na, "the records differ from the host routine's"
    med = lambda t: float(np.median(t))
    out = dict(metric="stereo_sink_meter_us", shape="256x4800 (sink), 256x240000 T64 D10 P101 Ta32 Da5 Tr255 Dr25 (bcast)", calls=calls, rotate=ROT,
               quiet_lsb=a.quiet_lsb, bcast_kernel=bc.kernel_name,
               a_sink_us_median=med(t_a), a_p10=float(np.percentile(t_a, 10)), a_p90=float(np.percentile(t_a, 90)),
               b_sink_metered_us_median=med(t_b), b_p10=float(np.percentile(t_b, 10)), b_p90=float(np.percentile(t_b, 90)),
               c_bcast_pcm_us_median=med(t_c), c_p10=float(np.percentile(t_c, 10)), c_p90=float(np.percentile(t_c, 90)),
               d_bcast_pcm_metered_us_median=med(t_d), d_p10=float(np.percentile(t_d, 10)), d_p90=float(np.percentile(t_d, 90)),
               b_over_a=med(t_b) / med(t_a), b_minus_a_us=med(t_b) - med(t_a), d_over_c=med(t_d) / med(t_c), d_minus_c_us=med(t_d) - med(t_c))
    for k in (plain, metered, call_plain, call_metered, bc):
        k.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
