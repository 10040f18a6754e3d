#!/usr/bin/env python3
"""The re-tune of a running broadcast receiver (sdrfm_bcast_retune) against the restart it replaces, at 256 streams tuned on
one shared row x 480 000 B (T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one run: each timed round
makes (a) sdrfm_bcast_tune and one plain call, (b) sdrfm_bcast_retune and one plain call and (c) the plain call alone, on three handles,
every call on the next of a rotation of input rows; (a) and (b) move all 256 streams by 5 kHz, back and forth, with precomputed taps.
Per kind: the host time of the tune / retune call itself, the device time between two events round the plain call, and the device time
from an event before the tune / retune call to the one behind the plain call.  One process, no retries.  Prints one JSON line and writes
it to profiles/bcast_retune_bench.json.
The yardstick is (a) of the same run: (b) uploads the same taps and replaces three memsets by one small kernel, so a median of (b) above
(a)'s by more than (a)'s own p10 - p90 width would be a defect; the plain call behind a re-tune is the kernel (c) launches."""
import argparse
import importlib
import json
import os
import sys
import time

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcast_retune_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp, fs = 256, 240000, 2.4e6
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "retune_bench")
    base = pkg.make_iq_rds(a.buffers, nsamp, groups, first_id=1)
    iqs = [torch.from_numpy(np.ascontiguousarray(base[k:k + 1])).cuda() for k in range(a.buffers)]
    offsets = [np.linspace(-1.0e6, 1.0e6, ns), np.linspace(-1.0e6, 1.0e6, ns) + 5e3]
    ctaps = [np.ascontiguousarray(np.stack([pkg.tuned_channel_taps(h, f, fs) for f in off])) for off in offsets]
    rots = [np.array([pkg.tuned_rotation(f, fs, 10) for f in off], np.float32) for off in offsets]
    carries = [np.ascontiguousarray(np.stack([pkg.retune_carry(o, n, 64, fs) for o, n in zip(offsets[1 - k], offsets[k])])) for k in (0, 1)]
    lib = pkg.load_library()

    def bcast():
        bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=ns, max_bytes_per_call=2 * nsamp,
                                                    audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                    diff_gain=pkg.stereo_diff_gain(10, fs), rds_gain=pkg.rds_gain(10, fs)))
        bc.tune(ctaps=ctaps[0], rot=rots[0], shared_input=True)
        return bc

    kinds = ("tune", "retune", "plain")
    hnd = {k: bcast() for k in kinds}
    na, nr = hnd["plain"].counts(2 * nsamp)
    outs = {k: (torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"),
                torch.zeros((ns, 2 * nr + 16), dtype=torch.float32, device="cuda")) for k in kinds}
    pcs = {k: torch.zeros(ns, dtype=torch.int32, device="cuda") for k in kinds}
    cur = torch.cuda.Stream()                                     # the three handles and the events on one stream of our own
    torch.cuda.synchronize()
    for k in kinds:
        hnd[k].set_stream(cur.cuda_stream)
    turn, host = [0], {"tune": [], "retune": []}

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(n, e=None):
        w = n % 2                                                 # the tuning this round moves to
        for i, k in enumerate(kinds):
            cur.synchronize()                                     # (tune and retune wait for the stream: the host times are theirs alone)
            if e: e[3 * i].record(cur)
            t0 = time.perf_counter()
            if k == "tune":
                rc = lib.sdrfm_bcast_tune(hnd[k]._h, ctaps[w].ctypes.data, rots[w].ctypes.data, pkg.lib.TUNE_SHARED_INPUT)
            elif k == "retune":
                rc = lib.sdrfm_bcast_retune(hnd[k]._h, ctaps[w].ctypes.data, rots[w].ctypes.data, carries[w].ctypes.data, None, pkg.lib.TUNE_SHARED_INPUT)
            else:
                rc = pkg.lib.OK
            t1 = time.perf_counter()
            assert rc == pkg.lib.OK, (k, rc)
            if e and k in host:
                host[k].append((t1 - t0) * 1e6)
            if e: e[3 * i + 1].record(cur)
            hnd[k].process_batch_device(nxt(), *outs[k], pcs[k])
            if e: e[3 * i + 2].record(cur)

    for n in range(a.warmup):
        one_round(n)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(9)] for _ in range(calls)]
    for n, e in enumerate(ev):
        one_round(a.warmup + n, e)
    torch.cuda.synchronize()
    call = {k: np.array([e[3 * i + 1].elapsed_time(e[3 * i + 2]) * 1e3 for e in ev]) for i, k in enumerate(kinds)}
    whole = {k: np.array([e[3 * i].elapsed_time(e[3 * i + 2]) * 1e3 for e in ev]) for i, k in enumerate(kinds)}
    out = dict(metric="bcast_retune_us", shape="256 streams on one shared row x 480000B T64 D10 P101 Ta32 Da5 Tr255 Dr25", calls=calls,
               input_buffers=len(iqs), moved_hz=5e3, kernels={k: hnd[k].kernel_name for k in kinds})
    for name, t in (("call", call), ("turn", whole), ("host", {k: np.array(v) for k, v in host.items()})):
        for k, v in t.items():
            out["%s_%s_us_median" % (k, name)] = float(np.median(v))
            out["%s_%s_us_p10" % (k, name)] = float(np.percentile(v, 10))
            out["%s_%s_us_p90" % (k, name)] = float(np.percentile(v, 90))
    for name in ("host", "turn"):
        width = out["tune_%s_us_p90" % name] - out["tune_%s_us_p10" % name]
        out["retune_minus_tune_%s_us_median" % name] = out["retune_%s_us_median" % name] - out["tune_%s_us_median" % name]
        out["tune_%s_us_p10_p90_width" % name] = width
        out["retune_%s_within_tunes_width" % name] = bool(out["retune_%s_us_median" % name] - out["tune_%s_us_median" % name] <= width)
    out["call_behind_retune_over_plain_median"] = out["retune_call_us_median"] / out["plain_call_us_median"]
    out["plain_call_spread_p10_p90_over_median"] = [out["plain_call_us_p10"] / out["plain_call_us_median"], out["plain_call_us_p90"] / out["plain_call_us_median"]]
    out["pilot_count_sum"] = {k: int(pcs[k].sum().item()) for k in kinds}
    for k in kinds:
        hnd[k].close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
