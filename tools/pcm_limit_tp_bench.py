#!/usr/bin/env python3
"""The cost of the limiter's true-peak form at 256 streams x 4800 pairs per call, LW = 6, the BS.1770 table, device-resident,
one process, no retries, the five kinds alternating in one loop:
  (a) the sample limiter on a programme that limits — the yardstick: k_pcm_limit, the parent's kernel, in the same run;
  (b) the true-peak limiter on quiet input: nothing over the ceiling, unity gain — the transparent case;
  (c) the true-peak limiter on the programme of (a), under the same + 12 dB of make-up gain;
  (d) the rate matcher's call (default table, + 100 ppm) on the same rows;
  (e) a copy of the same rows to pinned host memory.
Each figure is the median (and p10 - p90) over the timed calls of the device time between two events around one call.  The inputs rotate over
four buffers.  Behind the timed loop: the last call's rows, state and records of (c) are held to the host routine sdrfm_pcm_tplimit_s16, and the
true peak of either form's output under a ceiling of - 2 dB is recorded from pcm_truepeak_host.
Prints one JSON line; --out writes the same line to a file (profiles/pcm_limit_tp_bench.json)."""
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
KINDS = ("a_sample_active", "b_tp_quiet", "c_tp_active", "d_rate_matcher", "e_copy_to_host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls of each kind (>= 50)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    calls = max(a.calls, 50)
    ns, n, lw, slew = 256, 4800, 6, 4
    rng = np.random.default_rng(7)
    t = np.arange(n) / 48000.0
    # four programmes of two tones per channel at about - 12 dBFS: under the ceiling as they are, over it under + 12 dB
    rows = []
    for _ in range(ROT):
        f = rng.uniform(100.0, 12e3, (ns, 2, 2, 1))
        ph = rng.uniform(0, 6.28, (ns, 2, 2, 1))
        x = (4000.0 * np.sin(2 * np.pi * f * t + ph)).sum(axis=2)               # [ns, 2, n]
        rows.append(np.ascontiguousarray(np.rint(x).astype(np.int16).transpose(0, 2, 1).reshape(ns, 2 * n)))
    pcm = [torch.from_numpy(r).cuda() for r in rows]
    out = torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda")
    out_tp = torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda")
    out_r = torch.zeros((ns, 2 * (n + 2)), dtype=torch.int16, device="cuda")
    pinned = torch.zeros((ns, 2 * n), dtype=torch.int16).pin_memory()
    boost = int(pkg.normalise_gain_q12(-35.0)[0])                          # + 12 dB
    sample = pkg.PcmLimiter(ns, lw, slew)
    quiet, active = (pkg.PcmLimiter(ns, lw, slew, detect="truepeak") for _ in range(2))
    for k in (sample, active):
        k.set_gain(boost, jump=True)
    step = pkg.step_for(48000, 48000, 100.0)
    rm = pkg.PcmRateMatcher(ns, pkg.rate_coef(step=step))
    rm.set_step(step)
    cur = torch.cuda.Stream()                                             # every handle and the events on one stream of our own
    torch.cuda.synchronize()
    for k in (sample, quiet, active, rm):
        k.set_stream(cur.cuda_stream)

    def f_a(k):
        sample.process_batch_device(pcm[k % ROT], out, n)

    def f_b(k):
        quiet.process_batch_device(pcm[k % ROT], out_tp, n)

    def f_c(k):
        active.process_batch_device(pcm[k % ROT], out_tp, n)

    def f_d(k):
        rm.process_batch_device(pcm[k % ROT], out_r, n)

    def f_e(k):
        with torch.cuda.stream(cur):
            pinned.copy_(pcm[k % ROT], non_blocking=True)

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
    # the last timed call of (c) against the host routine: the whole history of that handle from reset, on three streams
    total = a.warmup + calls
    active.synchronize()
    got, st, rec = out_tp.cpu().numpy(), active.state(), active.read()
    assert sample.kernel_name == "pcm-limit" and active.kernel_name == "pcm-limit-tp"
    assert quiet.read()["limited"].sum() == 0, "the quiet programme was limited"
    assert (rec["limited"] > 0).sum() > ns // 2 and int(np.abs(got.astype(np.int64)).max()) <= 29204, "the active programme was not limited, or not held"
    par = np.array([(29204, 874, boost, boost)], dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
    for s in (0, ns // 2, ns - 1):
        h_st, h_rec, J = None, None, 0
        for k in range(total):
            kk = k if k < a.warmup else k - a.warmup
            want, h_st, h_rec = pkg.pcm_limit_tp_host(rows[kk % ROT][s], lw, slew, J, par, h_st, h_rec)
            J = min(65536, J + n)
        assert np.array_equal(got[s], want) and np.array_equal(st[s], h_st[0]) and rec[s].tobytes() == h_rec[0].tobytes(), \
            "the true-peak limiter's row %d differs from the host routine's" % s
    # the true peak of what comes out of either form under a ceiling of - 2 dB: measured with the meter's host routine, not bounded
    c2 = pkg.limit_ceiling(-2.0)
    peaks = {}
    for tag, kw in (("sample", {}), ("truepeak", dict(detect="truepeak"))):
        with pkg.PcmLimiter(ns, lw, slew, **kw) as lim:
            lim.set_params(c2, None)
            lim.set_gain(boost, jump=True)
            y = np.concatenate([lim.process_batch(rows[r]) for r in range(2)], axis=1)
        assert int(np.abs(y.astype(np.int64)).max()) <= c2
        peaks[tag] = float(np.max(pkg.truepeak_report(pkg.pcm_truepeak_host(y[:16])[0])["dbtp"]))
    med = lambda v: float(np.median(v))
    res = dict(metric="pcm_limit_tp_us", shape="256x4800 pairs", log2_window=lw, detector=list(active.detector), latency=active.latency, calls=calls,
               warmup=a.warmup, rotate=ROT, kernel=active.kernel_name, yardstick=sample.kernel_name, boost_q12=boost,
               limited_frac_active=float(rec["limited"].sum() / rec["n"].sum()), min_gain_active=int(rec["min_gain"].min()), ceiling_minus2_db=c2,
               ceiling_dbtp=float(20 * np.log10(c2 / 32768.0)), true_peak_dbtp_max_sample_form=peaks["sample"],
               true_peak_dbtp_max_truepeak_form=peaks["truepeak"], true_peak_streams=16)
    for tag, v in zip(KINDS, times):
        res.update({tag + "_us_median": med(v), tag + "_p10": float(np.percentile(v, 10)), tag + "_p90": float(np.percentile(v, 90))})
    res.update(c_over_a=med(times[2]) / med(times[0]), c_over_rate=med(times[2]) / med(times[3]), c_over_copy=med(times[2]) / med(times[4]),
               c_over_b=med(times[2]) / med(times[1]))
    for k in (sample, quiet, active, rm):
        k.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
