#!/usr/bin/env python3
"""The metered broadcast call (sdrfm_bcast_process_batch_metered) against the two calls it replaces, at 256 streams tuned on
one shared row x 480 000 B (T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one run: each timed round
makes (a) the plain tuned broadcast call, (b) the metered call and (c) the scan call of the same 256 tunings, on three handles, every call
on the next of a rotation of input rows.  Device time between events.  One process, no retries.  Prints one JSON line and writes it to
profiles/bcast_meter_bench.json.
The condition is (b) < (a) + (c) of the same run: a metered call that is not cheaper than the two handles it replaces would be a defect.
(b) / (a) is reported beside (a)'s own p10 - p90 spread, the noise floor it is to be read against."""
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
    ap.add_argument("--buffers", type=int, default=4, help="input rows in rotation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcast_meter_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "meter_bench")
    base = pkg.make_iq_rds(a.buffers, nsamp, groups, first_id=1)
    iqs = [torch.from_numpy(np.ascontiguousarray(base[k:k + 1])).cuda() for k in range(a.buffers)]
    offsets = np.linspace(-1.0e6, 1.0e6, ns)

    def bcast():
        bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=ns, max_bytes_per_call=2 * nsamp,
                                                    audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                    diff_gain=pkg.stereo_diff_gain(10, 2.4e6), rds_gain=pkg.rds_gain(10, 2.4e6)))
        bc.tune(offsets_hz=offsets, fs=2.4e6, shared_input=True)
        return bc

    hnd = dict(plain=bcast(), metered=bcast(),
               scan=pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=b, offsets_hz=offsets, h=h, fs=2.4e6, pilot_min=0.05, max_bytes_per_call=2 * nsamp,
                                                 shared_input=True)))
    kinds = tuple(hnd)
    na, nr = hnd["plain"].counts(2 * nsamp)
    outs = {k: (torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"),
                torch.zeros((ns, 2 * nr + 16), dtype=torch.float32, device="cuda")) for k in ("plain", "metered")}
    pcs = {k: torch.zeros(ns, dtype=torch.int32, device="cuda") for k in ("plain", "metered")}
    meters = {k: torch.zeros((ns, 8), dtype=torch.int64, device="cuda") for k in ("metered", "scan")}
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
            if k == "plain":
                hnd[k].process_batch_device(nxt(), *outs[k], pcs[k])
            elif k == "metered":
                hnd[k].process_batch_metered_device(nxt(), *outs[k], meters[k], pcs[k])
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
    out = dict(metric="bcast_metered_call_us", shape="256 streams on one shared row x 480000B T64 D10 P101 Ta32 Da5 Tr255 Dr25", calls=calls,
               input_buffers=len(iqs), kernels={k: hnd[k].kernel_name for k in kinds})
    for k, v in t.items():
        out["%s_us_median" % k] = float(np.median(v))
        out["%s_us_p10" % k] = float(np.percentile(v, 10))
        out["%s_us_p90" % k] = float(np.percentile(v, 90))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out["metered_over_plain_median"] = med["metered"] / med["plain"]
    out["plain_spread_p10_p90_over_median"] = [out["plain_us_p10"] / med["plain"], out["plain_us_p90"] / med["plain"]]
    out["plain_plus_scan_us_median"] = med["plain"] + med["scan"]
    out["metered_below_plain_plus_scan"] = bool(med["metered"] < med["plain"] + med["scan"])
    # the last round's work: the metered call's records against the scan call's (other rows of the rotation: the counts alone agree), and
    # its pilot counts against its own records
    torch.cuda.synchronize()
    out["n_sum"] = {k: int(meters[k][:, 0].sum().item()) for k in meters}
    out["metered_n_pilot_is_pilot_count"] = bool((meters["metered"][:, 1] == pcs["metered"].to(torch.int64)).all().item())
    for k in kinds:
        hnd[k].close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
