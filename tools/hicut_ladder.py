#!/usr/bin/env python3
"""What a high-cut buys a weak station once the blend has reached mono: the ladder behind scan.hicut_policy's two
defaults.  CPU only, the project's references alone, in the manner of tools/audio_ladder.py and on its signal and amplitudes: per
amplitude the definition's record and stereo stages, L and R as scan.audio_policy's blend of that record leaves them (tests/audio_ref.py),
then the host high-cut routine sdrfm_pcm_deemph_stereo_hicut_s16 at 75 us over them with h held flat at 32768, 16384, 8192 and 4096, and of
the PCM's L slots
  - the SNR of the fitted 1 kHz tone: its power over the residual's,
  - the tone's own loss: its fitted amplitude against the one at h = 32768, in dB.
Prints the table and the rule by which the defaults are picked from it, and writes both to profiles/hicut_ladder.txt."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import audio_ladder as al

HICUTS = (32768, 16384, 8192, 4096)
MAX_TONE_LOSS_DB = 6.0      # the rule's bound on what the high-cut may take from a 1 kHz tone
MIN_GAIN_DB = 1.0           # the rule's bound on what a rung must still win over the one above it


def tone_fit(x, fs=al.FS / al.D / al.DA, skip=600):
    """(SNR in dB, amplitude) of the least-squares 1 kHz tone in x[skip:]: audio_ladder.tone_snr_db's fit, the amplitude beside it"""
    x = np.asarray(x, np.float64)[skip:]
    t = np.arange(x.size) / fs
    cols = np.stack([np.ones_like(t), np.sin(2 * np.pi * al.TONE_HZ * t), np.cos(2 * np.pi * al.TONE_HZ * t)], 1)
    coef, *_ = np.linalg.lstsq(cols, x, rcond=None)
    rest = x - cols @ coef
    p = (coef[1] ** 2 + coef[2] ** 2) / 2.0
    return float(10.0 * np.log10(p / np.mean(rest ** 2))), float(np.sqrt(2.0 * p))


def ladder(amplitudes=al.AMPLITUDES, hicuts=HICUTS):
    """one dict per amplitude: amplitude, pilot_snr_db, blend and, per h of hicuts, snr_db[h] and loss_db[h]"""
    import audio_ref
    import scan_ref
    import stereo_ref
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    h = pkg.lowpass_taps(64, 120e3 / al.FS)
    g = pkg.default_config()[1]
    b = pkg.stereo_pilot_taps(101, al.FS / al.D)
    dg = pkg.stereo_diff_gain(al.D, al.FS)
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    gain = float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    rows = []
    for amp in amplitudes:
        r = scan_ref.scan_ref(al.capture(amp), pkg.tuned_channel_taps(h, 0.0, al.FS), 0.0, al.D, b, al.PILOT_MIN)
        meters = np.zeros(1, pkg.METER_DTYPE)
        for k, v in r["rec"].items():
            meters[k][0] = v
        report = pkg.meter_report(meters, al.FS, al.D)
        status = pkg.stream_status(report, [0.0])
        blend, _ = pkg.audio_policy(report, status)
        st = stereo_ref.stereo_ref(r["d"], b, g, al.PILOT_MIN, dg, al.DA)
        left, right = audio_ref.blend(st["am"], st["as_"], int(blend[0]), 32768)
        row = dict(amplitude=float(amp), pilot_snr_db=float(pkg.pilot_snr_db(report)[0]), blend=int(blend[0]), snr_db={}, loss_db={})
        ref_amp = None
        for hq in hicuts:
            pcm, _ = pkg.pcm_deemph_stereo_hicut_s16_host(left, right, alpha, gain, hq, hq, 32768)
            snr, a = tone_fit(pcm[0::2])
            ref_amp = a if ref_amp is None else ref_amp
            row["snr_db"][hq], row["loss_db"][hq] = snr, float(20.0 * np.log10(a / ref_amp))
        rows.append(row)
    return rows


def pick(rows, hicuts=HICUTS):
    """The rule.  floor_q15: walking h down from 32768 on the WEAKEST rung, the last h that still wins at least MIN_GAIN_DB of SNR over the
    h above it and takes at most MAX_TONE_LOSS_DB from the tone.  floor_db: that rung's pilot SNR, rounded to a whole dB — the weakest
    station the ladder has measured is where the policy stops cutting further."""
    weakest = min(rows, key=lambda r: r["amplitude"])
    floor_q15 = hicuts[0]
    for above, hq in zip(hicuts, hicuts[1:]):
        if weakest["snr_db"][hq] - weakest["snr_db"][above] < MIN_GAIN_DB or -weakest["loss_db"][hq] > MAX_TONE_LOSS_DB:
            break
        floor_q15 = hq
    return float(np.rint(weakest["pilot_snr_db"])), int(floor_q15)


def table(rows, hicuts=HICUTS):
    lines = ["amplitude  pilot SNR (dB)  blend_q15  " + "  ".join("SNR h=%-5d  loss h=%-5d" % (hq, hq) for hq in hicuts)]
    for r in rows:
        lines.append("%9g  %14.1f  %9d  " % (r["amplitude"], r["pilot_snr_db"], r["blend"]) +
                     "  ".join("%11.1f  %12.2f" % (r["snr_db"][hq], r["loss_db"][hq]) for hq in hicuts))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hicut_ladder.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("stm32f7-rtlsdr_amd")
    scan = importlib.import_module("stm32f7-rtlsdr_amd.scan")
    alpha = float(pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6))
    rows = ladder()
    floor_db, floor_q15 = pick(rows)
    lines = ["L-only 1 kHz tone, 50 kHz deviation, N(0, 4) byte noise, 0.1 s at 2.4 MS/s; T64 D10 P101 Ta%d Da5; pilot_min %.2f;" % (
        pkg.default_config()[1].size, al.PILOT_MIN),
        "L and R under audio_policy's blend, then sdrfm_pcm_deemph_stereo_hicut_s16 at 75 us, 48 kHz, h held flat; the PCM's L slots:",
        "SNR (dB) of the fitted 1 kHz tone and the tone's own loss (dB) against h = 32768", ""] + table(rows) + [""]
    lines.append("corners (Hz) at 75 us: " + ", ".join("h=%d: %.0f" % (hq, float(pkg.hicut_corner_hz(alpha, hq, 48000.0))) for hq in HICUTS))
    lines.append("rule: on the weakest rung walk h down from 32768; floor_q15 is the last h that still wins >= %.1f dB of SNR over the h above it and" % MIN_GAIN_DB)
    lines.append("takes <= %.1f dB from the 1 kHz tone; floor_db is that rung's pilot SNR rounded to a whole dB." % MAX_TONE_LOSS_DB)
    lines.append("picked: floor_db %.1f, floor_q15 %d" % (floor_db, floor_q15))
    lines.append("hicut_policy's defaults: full_db %.1f (audio_policy's mono corner), floor_db %.1f, floor_q15 %d." % (
        scan.STEREO_OFF_DB, scan.HICUT_FLOOR_DB, scan.HICUT_FLOOR_Q15))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
