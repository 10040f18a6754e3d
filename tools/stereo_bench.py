#!/usr/bin/env python3
"""The stereo call against the bit-exact mono call at the BASELINE configs[2] shape (256 streams x 240 000 samples, T = 64, D = 10,
Ta = 32, Da = 5; stereo: P = 101), device-resident, alternating in one run.  One process, no retries.  Prints one JSON line.

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/stereo_bench.py; counters in a run of their own (--pmc)."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

pkg = importlib.import_module("stm32f7-rtlsdr_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    iq = torch.from_numpy(pkg.make_iq_stereo(ns, nsamp, 1e3, 3.1e3, 75e3, first_id=1)).cuda()
    st = pkg.StereoDemod(pkg.StereoConfig(fir_coeffs=h, audio_coeffs=g, pilot_coeffs=b, pilot_min=0.05,
                                          diff_gain=pkg.stereo_diff_gain(10, 2.4e6), n_streams=ns, max_bytes_per_call=2 * nsamp))
    mono = pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, bit_exact=True, max_bytes_per_call=2 * nsamp))
    na = st.audio_count(2 * nsamp) + 8
    left = torch.zeros((ns, na), dtype=torch.float32, device="cuda")
    right = torch.zeros_like(left)
    audio = torch.zeros_like(left)
    pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
    cur = torch.cuda.Stream()                                     # both handles and the events on one stream of our own
    torch.cuda.synchronize()
    st.set_stream(cur.cuda_stream)
    mono.set_stream(cur.cuda_stream)
    for _ in range(a.warmup):
        st.process_batch_device(iq, left, right, pc)
        mono.process_batch_device(iq, audio)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    for e in ev:
        e[0].record(cur)
        st.process_batch_device(iq, left, right, pc)
        e[1].record(cur)
        e[2].record(cur)
        mono.process_batch_device(iq, audio)
        e[3].record(cur)
    torch.cuda.synchronize()
    t_st = np.array([e[0].elapsed_time(e[1]) * 1e3 for e in ev])
    t_mo = np.array([e[2].elapsed_time(e[3]) * 1e3 for e in ev])
    counts = pc.cpu().numpy()
    out = dict(metric="stereo_call_us", shape="256x240000 T64 D10 P101 Ta32 Da5", calls=calls, stereo_kernel=st.kernel_name,
               mono_kernel=mono.kernel_name, stereo_us_median=float(np.median(t_st)), stereo_us_p10=float(np.percentile(t_st, 10)),
               stereo_us_p90=float(np.percentile(t_st, 90)), mono_us_median=float(np.median(t_mo)),
               mono_us_p10=float(np.percentile(t_mo, 10)), mono_us_p90=float(np.percentile(t_mo, 90)),
               ratio_median=float(np.median(t_st) / np.median(t_mo)), pilot_count_min=int(counts.min()),
               new_d_per_stream=nsamp // 10)
    st.close()
    mono.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
