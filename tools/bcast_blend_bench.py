#!/usr/bin/env python3
"""What the audio conditioning of the broadcast receiver costs (sdrfm_bcast_set_audio), at 256 streams tuned on one shared
row x 480 000 B (T = 64, D = 10, P = 101, Ta = 32, Da = 5, Tr = 255, Dr = 25), device-resident, in one run: each timed round makes (a) the
plain tuned broadcast call and (b) the same call on a conditioned handle in mid-ramp — every stream's blend and gain on their way, the
ramps set again before they end — on two handles, every call on the next of a rotation of input rows.  Device time between events.  One
process, no retries.  Prints one JSON line and writes it to profiles/bcast_blend_bench.json.
The yardstick is (a) of the same run.  The blended stage works per audio output, 1 / Da of what the meter stage touches, in 32-bit integers
and five fp32 operations: (b) / (a) above the metered call's 1.058 (profiles/bcast_meter_bench.json) would be a defect to explain.  The ratio
is reported beside (a)'s own p10 - p90 spread, the noise floor it is to be read against."""
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
METERED_RATIO = 1.058


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 200)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=4, help="input rows in rotation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcast_blend_bench.json"))
    a = ap.parse_args()
    calls = max(a.calls, 200)
    ns, nsamp = 256, 240000
    h, g = pkg.default_config(64)
    b = pkg.stereo_pilot_taps(101, 240e3)
    groups = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "blend_bench")
    base = pkg.make_iq_rds(a.buffers, nsamp, groups, first_id=1)
    iqs = [torch.from_numpy(np.ascontiguousarray(base[k:k + 1])).cuda() for k in range(a.buffers)]
    offsets = np.linspace(-1.0e6, 1.0e6, ns)

    def bcast():
        bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, pilot_coeffs=b, pilot_min=0.05, n_streams=ns, max_bytes_per_call=2 * nsamp,
                                                    audio_coeffs=g, rds_coeffs=pkg.rds_lowpass_taps(255, 240e3),
                                                    diff_gain=pkg.stereo_diff_gain(10, 2.4e6), rds_gain=pkg.rds_gain(10, 2.4e6)))
        bc.tune(offsets_hz=offsets, fs=2.4e6, shared_input=True)
        return bc

    hnd = dict(plain=bcast(), blend=bcast())
    kinds = tuple(hnd)
    na, nr = hnd["plain"].counts(2 * nsamp)
    outs = {k: (torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"), torch.zeros((ns, na + 8), dtype=torch.float32, device="cuda"),
                torch.zeros((ns, 2 * nr + 16), dtype=torch.float32, device="cuda")) for k in kinds}
    pcs = {k: torch.zeros(ns, dtype=torch.int32, device="cuda") for k in kinds}
    cur = torch.cuda.Stream()                                     # both handles and the events on one stream of our own
    torch.cuda.synchronize()
    for k in kinds:
        hnd[k].set_stream(cur.cuda_stream)
    # the ramps: both start at one half (a jump, and one call to make it); at slew 1 a call of 4800 outputs moves them 4800 units, and the
    # targets swap ends every 2 calls, outside the timed span of a call: 16384 -> 6784 -> 16384 -> ... and 16384 -> 25984 -> 16384 -> ...,
    # never at a target (those lie below 4096 and above 28672), so every timed call finds every stream's blend and gain on their way
    hnd["blend"].set_audio(blend=0.5, gain=0.5, ramp_ms=0)
    hnd["blend"].process_batch_device(iqs[0], *outs["blend"], pcs["blend"])
    lo = (np.arange(ns) * 97 % 4096).astype(np.uint16)
    hi = (32768 - np.arange(ns) * 61 % 4096).astype(np.uint16)
    turn, sets = [0], [0]

    def nxt():
        turn[0] += 1
        return iqs[turn[0] % len(iqs)]

    def one_round(r, e=None):
        if r % 2 == 0:
            up = (r // 2) % 2 == 0
            hnd["blend"].set_audio(blend=lo if up else hi, gain=hi if up else lo, ramp_ms=1e9)
            sets[0] += 1
        for i, k in enumerate(kinds):
            if e: e[2 * i].record(cur)
            hnd[k].process_batch_device(nxt(), *outs[k], pcs[k])
            if e: e[2 * i + 1].record(cur)

    for r in range(a.warmup):
        one_round(r)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    moving = 0
    for r, e in enumerate(ev):
        one_round(a.warmup + r, e)
        st = hnd["blend"].audio_state()
        moving += int(((st["blend"] != st["blend_target"]) & (st["gain"] != st["gain_target"])).all())
    torch.cuda.synchronize()
    t = {k: np.array([e[2 * i].elapsed_time(e[2 * i + 1]) * 1e3 for e in ev]) for i, k in enumerate(kinds)}
    out = dict(metric="bcast_blend_call_us", state="measured on an MI355X", shape="256 streams on one shared row x 480000B T64 D10 P101 Ta32 Da5 Tr255 Dr25",
               calls=calls, input_buffers=len(iqs), kernels={k: hnd[k].kernel_name for k in kinds}, sets=sets[0],
               calls_that_ended_in_mid_ramp=moving)
    for k, v in t.items():
        out["%s_us_median" % k] = float(np.median(v))
        out["%s_us_p10" % k] = float(np.percentile(v, 10))
        out["%s_us_p90" % k] = float(np.percentile(v, 90))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out["blend_over_plain_median"] = med["blend"] / med["plain"]
    out["plain_spread_p10_p90_over_median"] = [out["plain_us_p10"] / med["plain"], out["plain_us_p90"] / med["plain"]]
    out["blend_ratio_inside_plain_spread"] = bool(out["plain_spread_p10_p90_over_median"][0] <= out["blend_over_plain_median"] <= out["plain_spread_p10_p90_over_median"][1])
    out["metered_over_plain_reference"] = METERED_RATIO
    out["blend_ratio_at_most_metered_ratio"] = bool(out["blend_over_plain_median"] <= METERED_RATIO)
    # the last round's work: bb and the pilot counts are the plain call's on the same tunings (other rows of the rotation: the shapes alone)
    torch.cuda.synchronize()
    out["pilot_count_sum"] = {k: int(pcs[k].sum().item()) for k in kinds}
    for k in kinds:
        hnd[k].set_stream(None)
        hnd[k].close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
