#!/usr/bin/env python3
"""The scan call (sdrfm_scan_process_batch) against the tuned broadcast call, at 256 streams x 480 000 B (T = 64, D = 10,
P = 101; the broadcast handle with Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one run: each timed round makes the scan call
on one shared row, the scan call on separate rows and the tuned broadcast call on separate rows, on three handles, every call on the next
of a rotation of input buffers larger than the last-level cache (the shared call reads row 0 of its buffer).  Device time between events.
One process, no retries.  Prints one JSON line and writes it to profiles/r14_scan_bench.json.  The yardstick is the tuned broadcast call of
the same run: the scan call walks the same K2, K3 and pilot filter, drops both sets of output chains and adds five conversions per d, so a
scan call slower than the tuned broadcast call would be a defect."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

pkg = importlib.import_module("stm32f7-rtlsdr_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=4, help="input buffers in rotation (4 x 123 MB: past the 256 MB last-level cache)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_scan_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "scan_bench")
    base = pkg.make_iq_rds(8, nsamp, groups, first_id=1)
    iqs = []
    for k in range(a.buffers):
        rows = np.concatenate([np.roll(base, k + r, axis=0) for r in range(ns // 8)])
        iqs.append(torch.from_numpy(np.ascontiguousarray(np.roll(rows, 2 * 977 * k, axis=1))).cuda())
    offsets = np.linspace(-1.0e6, 1.0e6, ns)
    scan_cfg = dict(pilot_coeffs=b, offsets_hz=offsets, h=h, fs=2.4e6, pilot_min=0.05, max_bytes_per_call=2 * nsamp)
    hnd = dict(scan_shared=pkg.ScanDemod(pkg.ScanConfig(shared_input=True, **scan_cfg)), scan=pkg.ScanDemod(pkg.ScanConfig(**scan_cfg)),
               bcast_tuned=pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=ns, max_bytes_per_call=2 * nsamp,
                                                                  audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                                  diff_gain=pkg.stereo_diff_gain(10, 2.4e6), rds_gain=pkg.rds_gain(10, 2.4e6))))
    kinds = tuple(hnd)
    hnd["bcast_tuned"].tune(offsets_hz=offsets, fs=2.4e6)
    na, nr = hnd["bcast_tuned"].counts(2 * nsamp)
    bc_out = (torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"),
              torch.zeros((ns, 2 * nr + 16), dtype=torch.float32, device="cuda"), torch.zeros(ns, dtype=torch.int32, device="cuda"))
    meters = {k: torch.zeros((ns, 8), dtype=torch.int64, device="cuda") for k in ("scan_shared", "scan")}
    cur = torch.cuda.Stream()                                     # the three handles and the events on one stream of our own
    torch.cuda.synchronize()
    for k in kinds:
        hnd[k].set_stream(cur.cuda_stream)
    turn = [0]

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(e=None):
        for i, k in enumerate(kinds):
            if e: e[2 * i].record(cur)
            if k == "bcast_tuned":
                hnd[k].process_batch_device(nxt(), *bc_out)
            else:
                hnd[k].process_batch_device(nxt(), meters[k])
            if e: e[2 * i + 1].record(cur)

    for _ in range(a.warmup):
        one_round()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
    for e in ev:
        one_round(e)
    torch.cuda.synchronize()
    t = {k: np.array([e[2 * i].elapsed_time(e[2 * i + 1]) * 1e3 for e in ev]) for i, k in enumerate(kinds)}
    out = dict(metric="scan_call_us", shape="256x480000B T64 D10 P101 (bcast: Ta32 Da5 Tr255 Dr25)", calls=calls, input_buffers=len(iqs),
               kernels={k: hnd[k].kernel_name for k in kinds})
    for k, v in t.items():
        out["%s_us_median" % k] = float(np.median(v))
        out["%s_us_p10" % k] = float(np.percentile(v, 10))
        out["%s_us_p90" % k] = float(np.percentile(v, 90))
    out["scan_over_bcast_tuned_median"] = float(np.median(t["scan"]) / np.median(t["bcast_tuned"]))
    out["scan_shared_over_scan_median"] = float(np.median(t["scan_shared"]) / np.median(t["scan"]))
    out["bound_scan_over_bcast_tuned"] = 1.0
    # the records of the last round, summed over the streams: a run whose kernels did no work shows here
    out["n_sum"] = {k: int(meters[k][:, 0].sum().item()) for k in meters}
    for k in kinds:
        hnd[k].close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
