#!/usr/bin/env python3
"""The broadcast handle's hist call (sdrfm_bcast_process_batch_metered_hist) against the two calls it replaces, at 256 streams
tuned on one shared row x 480 000 B (T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one process: each
timed round makes (a) the metered tuned broadcast call, (b) the hist call and (c) the scan handle's hist call of the same 256 tunings, on
three handles, every call on the next of a rotation of four input rows.  Device time between events, 200 timed calls of each kind, no
retries.  Three input classes, one after the other on the same handles and buffers:
  programme   a make_iq_stations capture of eight stations on the eight tuned offsets
  carrier     eight unmodulated, noise-free carriers on the eight tuned offsets: every d of a wave falls into one or two bins, the worst
              case for the same-address LDS atomics of the hist kernels
  noise       random bytes: d uniform in +-pi, 404 bins in use
Prints one JSON line and writes it to profiles/bcast_hist_bench.json, medians and p10 - p90 per kind and class.
The condition is (b) < (a) + (c) of the same run, in every class: a hist call that is not cheaper than the second handle it replaces would
be a defect.  (b) / (a) is reported beside (a)'s own p10 - p90 spread and nothing is promised about it.
--parent-check FILE puts the content of FILE (the metered call of this build against the parent commit's, alternating runs of
tools/bcast_meter_bench.py) into the result under "parent_check"."""
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

NS, NSAMP, FS, D = 256, 240000, 2.4e6, 10
OFFSETS = np.array([-900e3, -600e3, -400e3, -100e3, 100e3, 300e3, 600e3, 800e3])     # the eight tunings, stream s takes OFFSETS[s % 8]
CLASSES = ("programme", "carrier", "noise")


def base_rows(cls, n):
    """n rows [n, 2 NSAMP] of a class, every one a capture all the streams share"""
    if cls == "programme":
        rows = []
        for r in range(n):
            sts = [dict(offset_hz=float(f), amplitude=14.0, left_hz=400.0 + 300.0 * k + 37.0 * r, right_hz=1.1e3 + 500.0 * k, rds_phase=0.5 * k,
                        groups=pkg.rds_encode_groups(0xD400 + k, "HIST %03d" % k, "bcast_hist_bench")) for k, f in enumerate(OFFSETS)]
            rows.append(pkg.make_iq_stations(NSAMP, sts, fs=FS, seed=80 + r)[0])
        return np.stack(rows)
    if cls == "carrier":
        t = np.arange(NSAMP)
        rows = np.empty((n, 2 * NSAMP), np.uint8)
        for r in range(n):
            z = sum(14.0 * np.exp(1j * (0.3 * k + 0.7 * r + 2.0 * np.pi * f / FS * t)) for k, f in enumerate(OFFSETS))
            rows[r, 0::2] = np.clip(np.rint(127.5 + z.real), 0, 255)
            rows[r, 1::2] = np.clip(np.rint(127.5 + z.imag), 0, 255)
        return rows
    return pkg.make_iq(n, NSAMP, mode="random", fs=FS, first_id=90)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind and class (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=4, help="input rows in rotation")
    ap.add_argument("--parent-check", default=None, help="a JSON file to embed under \"parent_check\"")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcast_hist_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, FS / D)
    offsets = OFFSETS[np.arange(NS) % 8]

    def bcast():
        bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=NS, max_bytes_per_call=2 * NSAMP,
                                                    audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, FS / D),
                                                    diff_gain=pkg.stereo_diff_gain(D, FS), rds_gain=pkg.rds_gain(D, FS)))
        bc.tune(offsets_hz=offsets, fs=FS, shared_input=True)
        return bc

    hnd = dict(metered=bcast(), hist=bcast(),
               scan_hist=pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=b, offsets_hz=offsets, h=h, fs=FS, pilot_min=0.05, max_bytes_per_call=2 * NSAMP,
                                                      shared_input=True)))
    kinds = tuple(hnd)
    na, nr = hnd["metered"].counts(2 * NSAMP)
    outs = {k: (torch.zeros((NS, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((NS, na + 8), dtype=torch.float32, device="cuda"),
                torch.zeros((NS, 2 * nr + 16), dtype=torch.float32, device="cuda")) for k in ("metered", "hist")}
    pcs = {k: torch.zeros(NS, dtype=torch.int32, device="cuda") for k in ("metered", "hist")}
    meters = {k: torch.zeros((NS, 8), dtype=torch.int64, device="cuda") for k in kinds}
    rows = {k: torch.zeros((NS, pkg.HIST_BINS), dtype=torch.int32, device="cuda") for k in ("hist", "scan_hist")}
    iqs = [torch.zeros((1, 2 * NSAMP), dtype=torch.uint8, device="cuda") for _ in range(a.buffers)]
    cur = torch.cuda.Stream()                                     # the three handles and the events on one stream of our own
    torch.cuda.synchronize()
    for k in kinds:
        hnd[k].set_stream(cur.cuda_stream)
    turn = [0]

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(e=None, same=None):
        for i, k in enumerate(kinds):
            iq = nxt() if same is None else same
            if e: e[2 * i].record(cur)
            if k == "metered":
                hnd[k].process_batch_metered_device(iq, *outs[k], meters[k], pcs[k])
            elif k == "hist":
                hnd[k].process_batch_metered_hist_device(iq, *outs[k], meters[k], rows[k], pcs[k])
            else:
                hnd[k].process_batch_hist_device(iq, meters[k], rows[k])
            if e: e[2 * i + 1].record(cur)

    out = dict(metric="bcast_hist_call_us", shape="256 streams on one shared row x 480000B T64 D10 P101 Ta32 Da5 Tr255 Dr25", calls=calls,
               input_buffers=len(iqs), kernels=dict(metered=hnd["metered"].kernel_name, hist=hnd["hist"].hist_kernel_name()), classes={})
    for cls in CLASSES:
        base = base_rows(cls, len(iqs))
        for k, buf in enumerate(iqs):
            buf.copy_(torch.from_numpy(np.ascontiguousarray(base[k:k + 1])))
        torch.cuda.synchronize()
        for k in kinds:
            hnd[k].reset()
        for _ in range(a.warmup):
            one_round()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(kinds))] for _ in range(calls)]
        for e in ev:
            one_round(e)
        torch.cuda.synchronize()
        t = {k: np.array([e[2 * i].elapsed_time(e[2 * i + 1]) * 1e3 for e in ev]) for i, k in enumerate(kinds)}
        med = {k: float(np.median(v)) for k, v in t.items()}
        res = {}
        for k, v in t.items():
            res["%s_us_median" % k] = med[k]
            res["%s_us_p10" % k] = float(np.percentile(v, 10))
            res["%s_us_p90" % k] = float(np.percentile(v, 90))
        res["hist_over_metered_median"] = med["hist"] / med["metered"]
        res["metered_spread_p10_p90_over_median"] = [res["metered_us_p10"] / med["metered"], res["metered_us_p90"] / med["metered"]]
        res["metered_plus_scan_hist_us_median"] = med["metered"] + med["scan_hist"]
        res["hist_below_metered_plus_scan_hist"] = bool(med["hist"] < med["metered"] + med["scan_hist"])
        # one more round from a restart, all three on one row: a run whose kernels did no work shows here, and so does a class that does not
        # fill the bins it is meant to
        for k in kinds:
            hnd[k].reset()
        one_round(same=iqs[0])
        torch.cuda.synchronize()
        hh = rows["hist"].cpu().numpy().view(np.uint32)
        res["n_sum"] = {k: int(meters[k][:, 0].sum().item()) for k in kinds}
        res["hist_sum"] = int(hh.sum(dtype=np.uint64))
        res["bins_in_use_median"] = float(np.median((hh > 0).sum(1)))
        res["rows_equal_scan_rows"] = bool(torch.equal(rows["hist"], rows["scan_hist"]))
        res["records_equal_metered_records"] = bool(torch.equal(meters["hist"], meters["metered"]))
        out["classes"][cls] = res
    out["hist_below_metered_plus_scan_hist"] = all(r["hist_below_metered_plus_scan_hist"] for r in out["classes"].values())
    out["worst_hist_over_metered_median"] = max(r["hist_over_metered_median"] for r in out["classes"].values())
    if a.parent_check:
        with open(a.parent_check) as fh:
            out["parent_check"] = json.load(fh)
    for k in kinds:
        hnd[k].close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
