#!/usr/bin/env python3
"""Where a weak stereo station is better off in mono: the ladder behind scan.audio_policy's two defaults.  CPU only, the
project's references alone: for each station amplitude a 0.1 s capture of an L-only 1 kHz tone at 50 kHz deviation (siggen.make_iq_stereo's
multiplex and N(0, 4) byte noise, the station's amplitude varied), the definition's d and record (tests/scan_ref.py at offset 0), the
stereo stages on that d (tests/stereo_ref.py), and per rung
  - pilot_steadiness of the record and scan.pilot_snr_db of it,
  - the SNR of L, the stereo decoder's output, and of am, the mono sum: the fitted tone's power over the residual's,
  - what scan.audio_policy makes of the record.
Prints the table and writes it to profiles/audio_ladder.txt."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

AMPLITUDES = (100.0, 10.0, 5.0, 3.0, 2.0)
FS, D, DA, N_SAMPLES, TONE_HZ, DEVIATION_HZ, PILOT_MIN = 2.4e6, 10, 5, 240000, 1e3, 50e3, 0.05


def capture(amplitude, seed=3):
    """one row of siggen.make_iq_stereo's signal — L = sin(2 pi 1 kHz t), R = 0, the pilot at 10 % — at `amplitude` byte units in place of
    its 100; the carrier offset, start phase and noise are drawn as it draws them"""
    t = np.arange(N_SAMPLES, dtype=np.float64) / FS
    ph = 2.0 * np.pi * 19e3 * t
    rng = np.random.default_rng(seed)
    fc = (rng.random() * 2.0 - 1.0) * 20000.0
    phi0 = rng.random() * 2.0 * np.pi
    L = np.sin(2.0 * np.pi * TONE_HZ * t)
    m = 0.9 * (L / 2 + L / 2 * np.sin(2.0 * ph)) + 0.1 * np.sin(ph)
    phase = phi0 + np.cumsum(2.0 * np.pi * (fc + DEVIATION_HZ * m) / FS)
    noise = rng.normal(0.0, 2.0, size=(2, N_SAMPLES))
    row = np.empty(2 * N_SAMPLES, np.uint8)
    row[0::2] = np.clip(np.rint(127.5 + amplitude * np.cos(phase) + noise[0]), 0, 255)
    row[1::2] = np.clip(np.rint(127.5 + amplitude * np.sin(phase) + noise[1]), 0, 255)
    return row


def tone_snr_db(x, fs=FS / D / DA, skip=600):
    """the power of the least-squares 1 kHz tone in x[skip:] over the power of what is left beside it and the DC term"""
    x = np.asarray(x, np.float64)[skip:]
    t = np.arange(x.size) / fs
    cols = np.stack([np.ones_like(t), np.sin(2 * np.pi * TONE_HZ * t), np.cos(2 * np.pi * TONE_HZ * t)], 1)
    coef, *_ = np.linalg.lstsq(cols, x, rcond=None)
    rest = x - cols @ coef
    return float(10.0 * np.log10((coef[1] ** 2 + coef[2] ** 2) / 2.0 / np.mean(rest ** 2)))


def ladder(amplitudes=AMPLITUDES, **policy):
    """one dict per amplitude: amplitude, pilot_steadiness, pilot_snr_db, stereo_snr_db, mono_snr_db, present, stereo, blend, gain"""
    import scan_ref
    import stereo_ref
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    h = pkg.lowpass_taps(64, 120e3 / FS)
    g = pkg.default_config()[1]
    b = pkg.stereo_pilot_taps(101, FS / D)
    dg = pkg.stereo_diff_gain(D, FS)
    rows = []
    for amp in amplitudes:
        r = scan_ref.scan_ref(capture(amp), pkg.tuned_channel_taps(h, 0.0, FS), 0.0, D, b, PILOT_MIN)
        meters = np.zeros(1, pkg.METER_DTYPE)
        for k, v in r["rec"].items():
            meters[k][0] = v
        report = pkg.meter_report(meters, FS, D)
        status = pkg.stream_status(report, [0.0])
        blend, gain = pkg.audio_policy(report, status, **policy)
        st = stereo_ref.stereo_ref(r["d"], b, g, PILOT_MIN, dg, DA)
        rows.append(dict(amplitude=float(amp), pilot_steadiness=float(report["pilot_steadiness"][0]), pilot_snr_db=float(pkg.pilot_snr_db(report)[0]),
                         stereo_snr_db=tone_snr_db(st["L"]), mono_snr_db=tone_snr_db(st["am"]), present=bool(status[0]["present"]),
                         stereo=bool(status[0]["stereo"]), blend=int(blend[0]), gain=int(gain[0])))
    return rows


def table(rows):
    lines = ["amplitude  pilot_steadiness  pilot SNR (dB)  stereo L SNR (dB)  mono SNR (dB)  present  stereo  blend_q15  gain_q15"]
    for r in rows:
        lines.append("%9g  %16.4f  %14.1f  %17.1f  %13.1f  %7s  %6s  %9d  %8d" % (
            r["amplitude"], r["pilot_steadiness"], r["pilot_snr_db"], r["stereo_snr_db"], r["mono_snr_db"], r["present"], r["stereo"], r["blend"], r["gain"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_ladder.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    from importlib import import_module
    scan = import_module("stm32f7-rtlsdr_amd.scan")
    rows = ladder()
    lines = ["L-only 1 kHz tone, 50 kHz deviation, N(0, 4) byte noise, 0.1 s at 2.4 MS/s; T64 D10 P101 Ta%d Da5; pilot_min %.2f" % (
        pkg.default_config()[1].size, PILOT_MIN), ""] + table(rows) + [""]
    loss = [r for r in rows if r["stereo_snr_db"] < r["mono_snr_db"]]
    keep = [r for r in rows if r["stereo_snr_db"] >= r["mono_snr_db"]]
    lines.append("stereo is no worse than mono down to amplitude %g (pilot SNR %.1f dB) and worse from amplitude %g (%.1f dB) down;" % (
        keep[-1]["amplitude"], keep[-1]["pilot_snr_db"], loss[0]["amplitude"], loss[0]["pilot_snr_db"]))
    lines.append("audio_policy's defaults: full stereo from %.1f dB up, mono from %.1f dB down." % (scan.STEREO_FULL_DB, scan.STEREO_OFF_DB))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
