#!/usr/bin/env python3
"""The cost of the raw-capture IQ meter at 256 streams x 480 000 bytes per call (0.1 s at 2.4 MS/s), device-resident, one
process, no retries, the five kinds alternating in one loop:
  (a) the record-only call on carrier rows;
  (b) the hist call on the same rows;
  (c) the hist call on constant rows (every byte 128): the one-bin case;
  (d) the FM handle's default call on the same rows — the yardstick of the same run: it reads the same bytes and does far more with them;
  (e) a copy of the same rows to pinned host memory — what metering on the host would have to pay first.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers of 123 MB, more than the Infinity Cache holds, so every call reads cold.  Behind the timed loop the last call's records and rows of
(a), (b) and (c) are held to the host routine.  The read rate is the call's bytes over its median time.
Prints one JSON line; --out writes the same line to a file (profiles/iq_meter_bench.json).

Kernel statistics: rocprofv3 --kernel-trace --stats -- python tools/iq_meter_bench.py, in a run of its own."""
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
KINDS = ("a_record", "b_hist_carrier", "c_hist_constant", "d_fm_default", "e_copy_to_host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, nsamp = 256, 240000
    nbytes = 2 * nsamp
    rows = pkg.make_iq(ns, nsamp, mode="fm", first_id=1200)
    iq = [torch.from_numpy(np.roll(rows, r, axis=0)).cuda() for r in range(ROT)]           # the same rows on other streams: other addresses
    flat = [torch.full((ns, nbytes), 128, dtype=torch.uint8, device="cuda") for _ in range(ROT)]
    pinned = torch.zeros((ns, nbytes), dtype=torch.uint8).pin_memory()
    h, g = pkg.default_config(fir_taps=64)
    dm = pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, n_streams=ns, max_bytes_per_call=nbytes))
    audio = torch.zeros((ns, nsamp // 50 + 8), dtype=torch.float32, device="cuda")
    meters = [pkg.IqMeter(ns, nbytes) for _ in range(3)]
    rec = [torch.zeros(8 * ns, dtype=torch.int64, device="cuda") for _ in range(3)]
    hist = [None] + [torch.zeros(512 * ns, dtype=torch.int32, device="cuda") for _ in range(2)]
    cur = torch.cuda.Stream()                                             # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in meters + [dm]:
        k.set_stream(cur.cuda_stream)

    def f_a(k):
        meters[0].process_batch_device(iq[k % ROT], rec[0])

    def f_b(k):
        meters[1].process_batch_device(iq[k % ROT], rec[1], hist[1])

    def f_c(k):
        meters[2].process_batch_device(flat[k % ROT], rec[2], hist[2])

    def f_d(k):
        dm.process_batch_device(iq[k % ROT], audio)

    def f_e(k):
        with torch.cuda.stream(cur):
            pinned.copy_(iq[k % ROT], non_blocking=True)

    fs = (f_a, f_b, f_c, f_d, f_e)
    for k in range(a.warmup):
        for f in fs:
            f(k)
    torch.cuda.synchronize()
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in fs] for _ in range(calls)]
    for k in range(calls):
        for j, f in enumerate(fs):
            ev[k][j][0].record(cur)
            f(k)
            ev[k][j][1].record(cur)
    torch.cuda.synchronize()
    times = [np.array([ev[k][j][0].elapsed_time(ev[k][j][1]) * 1e3 for k in range(calls)]) for j in range(len(fs))]
    # the last timed call of every meter kind against the host routine
    last = np.roll(rows, (calls - 1) % ROT, axis=0)
    want, want_rows = pkg.iq_meter_host(last, with_hist=True)
    got = [r.cpu().numpy().view(pkg.IQ_METER_DTYPE) for r in rec]
    got_rows = [None] + [x.cpu().numpy().view(np.uint32).reshape(ns, 512) for x in hist[1:]]
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want.tobytes(), "the records differ from the host routine's"
    assert np.array_equal(got_rows[1].astype(np.uint64), want_rows), "the rows differ from the host routine's"
    flat_want, flat_rows = pkg.iq_meter_host(np.full((1, nbytes), 128, np.uint8), with_hist=True)
    assert all(got[2][s].tobytes() == flat_want[0].tobytes() for s in range(ns)) and (got_rows[2].astype(np.uint64) == flat_rows[0]).all(), "the constant rows"
    rep = pkg.iq_meter_report(got[0])
    med = lambda v: float(np.median(v))
    res = dict(metric="iq_meter_us", shape="256x480000 bytes", bytes_per_call=ns * nbytes, calls=calls, warmup=a.warmup, rotate=ROT,
               kernels=[meters[0].kernel_name, meters[1].kernel_name], fm_kernel=dm.kernel_name, geometry=list(pkg.iqmeter.iq_meter_geometry(ns, nbytes)),
               rms_dbfs_stream0=float(rep["rms_dbfs"][0]))
    for tag, v in zip(KINDS, times):
        res.update({tag + "_us_median": med(v), tag + "_p10": float(np.percentile(v, 10)), tag + "_p90": float(np.percentile(v, 90)),
                    tag + "_read_tb_per_s": ns * nbytes / (med(v) * 1e-6) / 1e12})
    res.update(a_over_fm=med(times[0]) / med(times[3]), b_over_a=med(times[1]) / med(times[0]), c_over_b=med(times[2]) / med(times[1]),
               a_over_copy=med(times[0]) / med(times[4]))
    for k in meters + [dm]:
        k.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
