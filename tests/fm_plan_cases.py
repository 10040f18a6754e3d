"""The handles whose create-time plan tests/golden/fm_plan_mi355x.json records (printed by the library as it stood BEFORE sdrfm_fm_plan.h existed, on an
MI355X): which designs the handle owns, its FmGeom, its names.  tests/test_fm_plan_cpu.py holds the planning function to the record on the CPU,
tests/test_fm_plan_gpu.py holds sdrfm_kernel_name to it on the device."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm_plan_mi355x.json")
N_STREAMS = 2
FS = {10: 2.4e6, 8: 2.048e6, 4: 1.024e6, 16: 3.2e6, 5: 2.4e6}
# (T, D, Ta, Da): every shape one of designs Q, S, B has an instance of ...
WITH_INSTANCE = [(64, 10, 32, 5), (32, 10, 32, 5), (16, 10, 32, 5), (64, 8, 32, 8), (16, 8, 32, 8), (64, 4, 32, 8), (64, 16, 32, 5)]
# ... and shapes with none of design B: 48 channel taps (design Q alone), 16 audio taps, an odd decimation, and a generic tile that has to halve NA
WITHOUT = [(48, 10, 32, 5), (64, 10, 16, 5), (64, 5, 32, 5), (64, 16, 32, 8)]
FLAGS = {"default": 0, "bit-exact": 4, "force-generic": 1, "guard-worst-case": 8}


def cases():
    """[(id, T, D, Ta, Da, flags, tap kind)]"""
    out = [("T%d-D%d-Ta%d-Da%d-%s" % (T, D, Ta, Da, name), T, D, Ta, Da, flags, "lowpass")
           for T, D, Ta, Da in WITH_INSTANCE + WITHOUT for name, flags in FLAGS.items()]
    # a band-pass channel filter: sum|h| > 2 |sum h|, which the low-pass heuristic refuses design Q
    out.append(("T64-D10-Ta32-Da5-bandpass", 64, 10, 32, 5, 0, "bandpass"))
    return out


def taps(pkg, T, D, Ta, Da, kind):
    h, g = pkg.default_config(T, fs=FS[D], fir_decim=D, audio_taps=Ta, audio_decim=Da)
    if kind == "bandpass":
        h = (2.0 * h.astype(np.float64) * np.cos(0.5 * np.pi * np.arange(T))).astype(np.float32)
    return h, g


def call_nsamp(D, Da):
    return 8 * D * Da * 8


def load_record():
    with open(GOLDEN) as f:
        return {c["id"]: c for c in json.load(f)["cases"]}

