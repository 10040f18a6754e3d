#!/usr/bin/env python3
"""The broadcast receiver call against the two calls it stands for, at the BASELINE configs[2] shape (256 streams x 240 000 samples,
T = 64, D = 10, P = 101; stereo: Ta = 32, Da = 5; RDS: Tr = 255, Dr = 25), device-resident, in one run: each timed round makes the combined
call, then the stereo call, then the RDS call, every call on the next of a rotation of input buffers larger than the last-level cache
(so no call finds its input warm from the one before).  One process, no retries.  Prints one JSON line.

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/bcast_bench.py; counters in a run of their own (--pmc)."""
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
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    gr = pkg.rds_lowpass_taps(255, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "bcast_bench")
    base = pkg.make_iq_rds(8, nsamp, groups, first_id=1)
    iqs = []
    for k in range(a.buffers):
        rows = np.concatenate([np.roll(base, k + r, axis=0) for r in range(ns // 8)])
        iqs.append(torch.from_numpy(np.ascontiguousarray(np.roll(rows, 2 * 977 * k, axis=1))).cuda())
    common = dict(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=ns, max_bytes_per_call=2 * nsamp)
    dg, rg = pkg.stereo_diff_gain(10, 2.4e6), pkg.rds_gain(10, 2.4e6)
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(audio_coeffs=g, rds_coeffs=gr, diff_gain=dg, rds_gain=rg, **common))
    st = pkg.StereoDemod(pkg.StereoConfig(audio_coeffs=g, diff_gain=dg, **common))
    rd = pkg.RdsDemod(pkg.RdsConfig(rds_coeffs=gr, rds_gain=rg, **common))
    na, nr = bc.counts(2 * nsamp)
    left, right = (torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda") for _ in range(2))
    left_s, right_s = torch.zeros_like(left), torch.zeros_like(right)
    bb = torch.zeros((ns, 2 * nr + 16), dtype=torch.float32, device="cuda")
    bb_r = torch.zeros_like(bb)
    pc, pc_s, pc_r = (torch.zeros(ns, dtype=torch.int32, device="cuda") for _ in range(3))
    cur = torch.cuda.Stream()                                     # the three handles and the events on one stream of our own
    torch.cuda.synchronize()
    for hnd in (bc, st, rd):
        hnd.set_stream(cur.cuda_stream)
    turn = [0]

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(e=None):
        if e: e[0].record(cur)
        bc.process_batch_device(nxt(), left, right, bb, pc)
        if e: e[1].record(cur); e[2].record(cur)
        st.process_batch_device(nxt(), left_s, right_s, pc_s)
        if e: e[3].record(cur); e[4].record(cur)
        rd.process_batch_device(nxt(), bb_r, pc_r)
        if e: e[5].record(cur)

    for _ in range(a.warmup):
        one_round()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
    for e in ev:
        one_round(e)
    torch.cuda.synchronize()
    t = {k: np.array([e[2 * i].elapsed_time(e[2 * i + 1]) * 1e3 for e in ev]) for i, k in enumerate(("bcast", "stereo", "rds"))}
    out = dict(metric="bcast_call_us", shape="256x240000 T64 D10 P101 Ta32 Da5 Tr255 Dr25", calls=calls, input_buffers=len(iqs),
               bcast_kernel=bc.kernel_name, stereo_kernel=st.kernel_name, rds_kernel=rd.kernel_name)
    for k, v in t.items():
        out["%s_us_median" % k] = float(np.median(v))
        out["%s_us_p10" % k] = float(np.percentile(v, 10))
        out["%s_us_p90" % k] = float(np.percentile(v, 90))
    out["bcast_over_stereo_plus_rds_median"] = float(np.median(t["bcast"]) / (np.median(t["stereo"]) + np.median(t["rds"])))
    out["target_bcast_over_stereo_plus_rds"] = 0.70
    out["bcast_pilot_count_min"] = int(pc.cpu().numpy().min())
    out["new_d_per_stream"] = nsamp // 10
    for hnd in (bc, st, rd):
        hnd.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
