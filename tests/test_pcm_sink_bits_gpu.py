"""The device PCM sinks' bits, pinned: SHA-256 of the PCM bytes and of the carried states' bit patterns of PcmSink and StereoPcmSink, default form (the
blocked scan) and exact form, against tests/golden/pcm_sink_bits.json, which holds what the commit named in it left.  The other sink tests hold the default
forms to the exact form within 1 LSB and to each other bit for bit; this one holds all four kernels to their own past, so that a change of the shared bodies
(csrc/sdrfm_sink_kernels.h) which moves one bit of either sink shows here.  Inputs: tools/pcm_stereo_scan_emulate.py's mono_inputs / sink_inputs, two calls
with the state carried, at lengths below, at and above one chunk (19) and one segment (4864), two segments plus one, and stream counts that leave the exact
form a partial last block of 64.  A differing hash is a finding to explain: the hashes are regenerated (record()) only by a change that means to move bits."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
emu = importlib.import_module("pcm_stereo_scan_emulate")
pp = importlib.import_module("pcm_params")

GOLDEN = os.path.join(ROOT, "tests", "golden", "pcm_sink_bits.json")
SHAPES = [(3, 1), (2, 18), (1, 19), (3, 20), (5, 4863), (63, 4864), (65, 4865), (2, 9729), (256, 4800)]   # streams x samples per call
ALPHAS = ["75us", "0.05"]
SINKS = ["mono", "stereo"]
FORMS = ["default", "exact"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hashes(pkg, sink, form):
    """{"<alpha> <ns>x<n>": {"pcm": sha, "state": sha}} of one sink in one form"""
    lib = pkg.load_library()
    out = {}
    for name in ALPHAS:
        alpha = pp.alpha_of(lib, name)
        for ns, n in SHAPES:
            if sink == "mono":
                x = emu.mono_inputs(ns, n)
                with pkg.PcmSink(ns, alpha, pp.DEFAULT_GAIN, exact=form == "exact") as k:
                    pcm = [k.process_batch(x[:, :n]), k.process_batch(x[:, n:])]
                    st = k.state()
            else:
                left, right = emu.sink_inputs(ns, n)
                with pkg.StereoPcmSink(ns, alpha, pp.DEFAULT_GAIN, exact=form == "exact") as k:
                    pcm = [k.process_batch(left[:, :n], right[:, :n]), k.process_batch(left[:, n:], right[:, n:])]
                    st = k.state()
            pcm = np.concatenate(pcm, axis=1)
            assert pcm.dtype == np.int16 and pcm.shape == (ns, 4 * n) and st.dtype == np.float32, (pcm.dtype, pcm.shape, st.dtype)
            out["%s %dx%d" % (name, ns, n)] = {"pcm": _sha(pcm), "state": _sha(st.view(np.uint32))}
    return out


def record(pkg, commit):
    """the golden file's content, from the library `pkg` loads (built from `commit`)"""
    return {"commit": commit, "inputs": "tools/pcm_stereo_scan_emulate.py mono_inputs / sink_inputs, two calls of n, gain tests/pcm_params.py DEFAULT_GAIN",
            "hashes": {"%s %s" % (s, f): hashes(pkg, s, f) for s in SINKS for f in FORMS}}


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("sink", SINKS)
def test_pcm_and_state_bits_are_the_recorded_ones(pkg, sink, form):
    with open(GOLDEN) as f:
        want = json.load(f)["hashes"]["%s %s" % (sink, form)]
    got = hashes(pkg, sink, form)
    assert sorted(got) == sorted(want)
    bad = [(k, w) for k in sorted(got) for w in ("pcm", "state") if got[k][w] != want[k][w]]
    assert not bad, bad
