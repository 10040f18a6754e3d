#!/usr/bin/env python3
"""The cost of the stereo PCM sink's loudness meter at 256 streams x 4800 samples per call, device-resident, one process, no
retries, the kinds of a group alternating in one loop:
  (a) the stereo sink's default form on a plain sink — the yardstick, from the same run;
  (m) the same call on a sink with the audio meter (§4.20) alone — what the loudness add-on is compared with;
  (b) the same call with loudness enabled (block_len 4800, 64 slots): the sink's launch and k_pcm_loudness behind it;
  (c) the same call with the audio meter and loudness enabled;
  (d) sdrfm_bcast_process_batch_pcm with a plain sink (256 x 240 000 samples, T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25);
  (e), (f) the same call with a loudness sink and with a meter + loudness sink.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers, so that no call finds its input where the one before left it.  The last loudness call's energies are checked against the host
routine on the PCM it left.  Prints one JSON line; --out writes the same line to a file (profiles/stereo_sink_loudness_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/stereo_sink_loudness_bench.py, in a run of its own."""
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
    ap.add_argument("--block-len", type=int, default=4800)
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
    new = lambda: pkg.StereoPcmSink(ns, alpha, gain)
    plain, meter, loud, both = new(), new(), new(), new()
    call_plain, call_loud, call_both = new(), new(), new()                       # the one-call forms'
    cur = torch.cuda.Stream()                                     # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (bc, plain, meter, loud, both):
        k.set_stream(cur.cuda_stream)
    for k in (meter, both, call_both):
        k.enable_meter(8)
    for k in (loud, both, call_loud, call_both):
        k.enable_loudness(a.block_len, 64)
    for r in range(ROT):                                          # the sinks' inputs: four stations' L and R
        bc.process_batch_device(iq[r], left[r], right[r], bb, pc)
    bc.synchronize()
    bc.reset()
    sink_call = lambda s: (lambda k: s.process_batch_device(left[k % ROT], right[k % ROT], pcm[k % ROT], na))
    bcast_call = lambda s: (lambda k: bc.process_batch_pcm_device(s, iq[k % ROT], left[0], right[0], pcm[k % ROT], bb, pc))
    sink_fns = [sink_call(s) for s in (plain, meter, loud, both)]
    bcast_fns = [bcast_call(s) for s in (call_plain, call_loud, call_both)]
    for k in range(a.warmup):
        for f in sink_fns + bcast_fns:
            f(k)
    torch.cuda.synchronize()
    t_a, t_m, t_b, t_c = _group(cur, calls, sink_fns)
    t_d, t_e, t_f = _group(cur, calls, bcast_fns)
    bc.synchronize()
    # the energies are what the host routine makes of the PCM the last loudness call left, its state carried from the device
    loud.synchronize()
    first, _ = loud.read_loudness()
    st = loud.loudness_state()
    assert int(st["pos"][0]) == (a.warmup + calls) * na, "pos"
    loud.process_batch_device(left[0], right[0], pcm[0], na)
    f2, got = loud.read_loudness()
    want, _ = pkg.pcm_loudness_host(pcm[0].cpu().numpy(), a.block_len, state=st)
    assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-9 * want + 1e-3 * a.block_len), "the energies differ from the host routine's"
    med = lambda t: float(np.median(t))
    out = dict(metric="stereo_sink_loudness_us", shape="256x4800 (sink), 256x240000 T64 D10 P101 Ta32 Da5 Tr255 Dr25 (bcast)", calls=calls, rotate=ROT,
               block_len=a.block_len, bcast_kernel=bc.kernel_name)
    for name, t in (("a_sink", t_a), ("m_sink_meter", t_m), ("b_sink_loudness", t_b), ("c_sink_meter_loudness", t_c), ("d_bcast_pcm", t_d),
                    ("e_bcast_pcm_loudness", t_e), ("f_bcast_pcm_meter_loudness", t_f)):
        out[name + "_us_median"], out[name + "_p10"], out[name + "_p90"] = med(t), float(np.percentile(t, 10)), float(np.percentile(t, 90))
    out.update(b_over_a=med(t_b) / med(t_a), b_minus_a_us=med(t_b) - med(t_a), m_minus_a_us=med(t_m) - med(t_a), c_minus_a_us=med(t_c) - med(t_a),
               loudness_over_meter_addon=(med(t_b) - med(t_a)) / (med(t_m) - med(t_a)), e_over_d=med(t_e) / med(t_d), e_minus_d_us=med(t_e) - med(t_d),
               f_minus_d_us=med(t_f) - med(t_d))
    for k in (plain, meter, loud, both, call_plain, call_loud, call_both, bc):
        k.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
