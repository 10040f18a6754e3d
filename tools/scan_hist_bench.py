#!/usr/bin/env python3
"""The scan handle's hist call (sdrfm_scan_process_batch_hist) against the plain scan call and the tuned broadcast call, at
256 streams x 480 000 B (T = 64, D = 10, P = 101; the broadcast handle with Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one
process: each timed round makes the plain scan call, the hist call and the tuned broadcast call on three handles, every call on the next of
a rotation of input buffers larger than the last-level cache.  Device time between events, 200 timed calls of each kind, no retries.  Three
input classes, one after the other on the same handles and buffers:
  programme   every stream tuned to a station of a make_iq_stations capture (eight captures, eight offsets, in turn)
  carrier     an unmodulated, noise-free carrier on every stream's tuned offset: every d of a wave falls into one or two bins, the worst
              case for the same-address LDS atomics of the hist kernel
  noise       random bytes: d uniform in +-pi, 404 bins in use
Prints one JSON line and writes it to profiles/scan_hist_bench.json, medians and p10 - p90 per kind and class.  The yardsticks are the same
run's other calls: the hist call walks what the tuned broadcast call walks, less both output chains, so a hist-call median above the tuned
broadcast call's in any class is a defect (yardstick 1); the ratio to the plain scan call is reported per class (yardstick 2).
--parent-check FILE puts the content of FILE (the plain scan call of this build against the parent commit's, alternating runs of
tools/scan_bench.py) into the result under "parent_check"."""
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


def base_rows(cls):
    """eight rows [8, 2 NSAMP] of a class, row k for the streams tuned to OFFSETS[k]"""
    if cls == "programme":
        rows = []
        for k, f in enumerate(OFFSETS):
            st = dict(offset_hz=float(f), amplitude=100.0, left_hz=400.0 + 300.0 * k, right_hz=1.1e3 + 500.0 * k, rds_phase=0.5 * k,
                      groups=pkg.rds_encode_groups(0xD300 + k, "HIST %03d" % k, "scan_hist_bench"))
            rows.append(pkg.make_iq_stations(NSAMP, [st], fs=FS, seed=60 + k)[0])
        return np.stack(rows)
    if cls == "carrier":
        n = np.arange(NSAMP)
        rows = np.empty((8, 2 * NSAMP), np.uint8)
        for k, f in enumerate(OFFSETS):
            z = 100.0 * np.exp(1j * (0.3 * k + 2.0 * np.pi * f / FS * n))
            rows[k, 0::2] = np.clip(np.rint(127.5 + z.real), 0, 255)
            rows[k, 1::2] = np.clip(np.rint(127.5 + z.imag), 0, 255)
        return rows
    return pkg.make_iq(8, NSAMP, mode="random", fs=FS, first_id=70)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind and class (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=4, help="input buffers in rotation (4 x 123 MB: past the 256 MB last-level cache)")
    ap.add_argument("--parent-check", default=None, help="a JSON file to embed under \"parent_check\"")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_hist_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, FS / D)
    offsets = OFFSETS[np.arange(NS) % 8]
    scan_cfg = dict(pilot_coeffs=b, offsets_hz=offsets, h=h, fs=FS, pilot_min=0.05, max_bytes_per_call=2 * NSAMP)
    hnd = dict(scan=pkg.ScanDemod(pkg.ScanConfig(**scan_cfg)), scan_hist=pkg.ScanDemod(pkg.ScanConfig(**scan_cfg)),
               bcast_tuned=pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=NS, max_bytes_per_call=2 * NSAMP,
                                                                  audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, FS / D),
                                                                  diff_gain=pkg.stereo_diff_gain(D, FS), rds_gain=pkg.rds_gain(D, FS))))
    kinds = tuple(hnd)
    hnd["bcast_tuned"].tune(offsets_hz=offsets, fs=FS)
    na, nr = hnd["bcast_tuned"].counts(2 * NSAMP)
    bc_out = (torch.zeros((NS, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((NS, na + 8), dtype=torch.float32, device="cuda"),
              torch.zeros((NS, 2 * nr + 16), dtype=torch.float32, device="cuda"), torch.zeros(NS, dtype=torch.int32, device="cuda"))
    meters = {k: torch.zeros((NS, 8), dtype=torch.int64, device="cuda") for k in ("scan", "scan_hist")}
    hist = torch.zeros((NS, pkg.HIST_BINS), dtype=torch.int32, device="cuda")
    iqs = [torch.zeros((NS, 2 * NSAMP), dtype=torch.uint8, device="cuda") for _ in range(a.buffers)]
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
            elif k == "scan_hist":
                hnd[k].process_batch_hist_device(nxt(), meters[k], hist)
            else:
                hnd[k].process_batch_device(nxt(), meters[k])
            if e: e[2 * i + 1].record(cur)

    out = dict(metric="scan_hist_call_us", shape="256x480000B T64 D10 P101 (bcast: Ta32 Da5 Tr255 Dr25)", calls=calls, input_buffers=len(iqs), classes={},
               bound_scan_hist_over_bcast_tuned=1.0)
    for cls in CLASSES:
        base = base_rows(cls)
        for k, buf in enumerate(iqs):                             # stream s reads row s % 8, every buffer rolled on in time
            rows = np.roll(base, 2 * 977 * k, axis=1)[np.arange(NS) % 8]
            buf.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
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
        res = dict(kernels={k: hnd[k].kernel_name for k in kinds})
        for k, v in t.items():
            res["%s_us_median" % k] = float(np.median(v))
            res["%s_us_p10" % k] = float(np.percentile(v, 10))
            res["%s_us_p90" % k] = float(np.percentile(v, 90))
        res["scan_hist_over_bcast_tuned_median"] = float(np.median(t["scan_hist"]) / np.median(t["bcast_tuned"]))
        res["scan_hist_over_scan_median"] = float(np.median(t["scan_hist"]) / np.median(t["scan"]))
        # the last round's outputs: a run whose kernels did no work shows here, and so does a class that does not fill the bins it is meant to
        hh = hist.cpu().numpy().view(np.uint32)
        res["n_sum"] = {k: int(meters[k][:, 0].sum().item()) for k in meters}
        res["hist_sum"] = int(hh.sum(dtype=np.uint64))
        res["bins_in_use_median"] = float(np.median((hh > 0).sum(1)))
        res["n_equal"] = bool(torch.equal(meters["scan"][:, 0], meters["scan_hist"][:, 0]))
        out["classes"][cls] = res
    out["worst_scan_hist_over_bcast_tuned_median"] = max(r["scan_hist_over_bcast_tuned_median"] for r in out["classes"].values())
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
