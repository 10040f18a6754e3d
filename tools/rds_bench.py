#!/usr/bin/env python3
"""The RDS call, the stereo call and the bit-exact mono call at the BASELINE configs[2] shape (256 streams x 240 000 samples, T = 64,
D = 10; RDS: P = 101, Tr = 255, Dr = 25; stereo: P = 101, Ta = 32, Da = 5), device-resident, in one run: each timed round makes the three
calls one after the other, every call on the next of a rotation of input buffers larger than the last-level cache (so no call finds
its input warm from the one before).  One process, no retries.  Prints one JSON line.

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/rds_bench.py; counters in a run of their own (--pmc)."""
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
    ap.add_argument("--buffers", type=int, default=4, help="input buffers in rotation (4 x 123 MB: past the 256 MB last-level cache)")
    ap.add_argument("--rds-taps", type=int, default=255, help="Tr (the default shape's 255; 1 takes the output chains and the long halo away)")
    ap.add_argument("--rds-decim", type=int, default=25)
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    gr = pkg.rds_lowpass_taps(a.rds_taps, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "rds_bench")
    base = pkg.make_iq_rds(8, nsamp, groups, first_id=1)
    iqs = []
    for k in range(a.buffers):
        rows = np.concatenate([np.roll(base, k + r, axis=0) for r in range(ns // 8)])
        iqs.append(torch.from_numpy(np.ascontiguousarray(np.roll(rows, 2 * 977 * k, axis=1))).cuda())
    rd = pkg.RdsDemod(pkg.RdsConfig(fir_coeffs=h, pilot_coeffs=b, rds_coeffs=gr, pilot_min=0.05, rds_gain=pkg.rds_gain(10, 2.4e6),
                                    rds_decim=a.rds_decim, n_streams=ns, max_bytes_per_call=2 * nsamp))
    st = pkg.StereoDemod(pkg.StereoConfig(fir_coeffs=h, audio_coeffs=g, pilot_coeffs=b, pilot_min=0.05,
                                          diff_gain=pkg.stereo_diff_gain(10, 2.4e6), n_streams=ns, max_bytes_per_call=2 * nsamp))
    mono = pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, bit_exact=True, max_bytes_per_call=2 * nsamp))
    na = st.audio_count(2 * nsamp) + 8
    left = torch.zeros((ns, na), dtype=torch.float32, device="cuda")
    right = torch.zeros_like(left)
    audio = torch.zeros_like(left)
    bb = torch.zeros((ns, 2 * rd.count(2 * nsamp) + 16), dtype=torch.float32, device="cuda")
    pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
    pc_r = torch.zeros(ns, dtype=torch.int32, device="cuda")
    cur = torch.cuda.Stream()                                     # the three handles and the events on one stream of our own
    torch.cuda.synchronize()
    for hnd in (rd, st, mono):
        hnd.set_stream(cur.cuda_stream)
    turn = [0]

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(e=None):
        if e: e[0].record(cur)
        rd.process_batch_device(nxt(), bb, pc_r)
        if e: e[1].record(cur); e[2].record(cur)
        st.process_batch_device(nxt(), left, right, pc)
        if e: e[3].record(cur); e[4].record(cur)
        mono.process_batch_device(nxt(), audio)
        if e: e[5].record(cur)

    for _ in range(a.warmup):
        one_round()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
    for e in ev:
        one_round(e)
    torch.cuda.synchronize()
    t = {k: np.array([e[2 * i].elapsed_time(e[2 * i + 1]) * 1e3 for e in ev]) for i, k in enumerate(("rds", "stereo", "mono"))}
    out = dict(metric="rds_call_us", shape="256x240000 T64 D10 P101 Tr%d Dr%d (stereo: Ta32 Da5)" % (a.rds_taps, a.rds_decim), calls=calls, input_buffers=len(iqs),
               rds_kernel=rd.kernel_name, stereo_kernel=st.kernel_name, mono_kernel=mono.kernel_name)
    for k, v in t.items():
        out["%s_us_median" % k] = float(np.median(v))
        out["%s_us_p10" % k] = float(np.percentile(v, 10))
        out["%s_us_p90" % k] = float(np.percentile(v, 90))
    out["rds_over_stereo_median"] = float(np.median(t["rds"]) / np.median(t["stereo"]))
    out["target_rds_over_stereo"] = 1.15
    out["rds_pilot_count_min"] = int(pc_r.cpu().numpy().min())
    out["new_d_per_stream"] = nsamp // 10
    for hnd in (rd, st, mono):
        hnd.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
