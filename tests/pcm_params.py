"""The sink parameters the PCM tests sweep (tests/test_pcm_sink_params_gpu.py on the device; tests/test_pcm_chain_cpu.py, tests/test_pcm_stereo_scan_cpu.py and
tests/test_pcm_mono_scan_cpu.py on the emulators): every alpha at which the library takes another path or builds other tables, and the gains that mirror, mute and
saturate the output.  An alpha is named here and resolved with the library (sdrfm_pcm_alpha is the library's own float arithmetic)."""
import numpy as np

F = np.float32
MIN_ALPHA = F(0.231)                                     # SDRFM_CHAIN_MIN_ALPHA (csrc/sdrfm_sink_chain.h)
ALPHAS = ["1", "0.99", "0.5", "50us", "75us", "0.231f", "below 0.231f", "0.05", "0.001"]
DEFAULT_GAIN = float(F(32767.0 / (2 * np.pi * 75e3 / 240e3)))   # 16 689: +-75 kHz deviation at 240 kS/s is full scale
GAINS = [DEFAULT_GAIN, -DEFAULT_GAIN, 0.0, 1e6]
# the chain inside design Q's launch serves alpha in [0.231f, 1 - 1.8e-5] (sdrfm_sink_chain_tables): of ALPHAS, these
CHAIN_ALPHAS = ["0.99", "0.5", "50us", "75us", "0.231f"]


def alpha_of(lib, name):
    if name.endswith("us"):
        return float(lib.sdrfm_pcm_alpha(48000.0, float(name[:-2]) * 1e-6))
    if name == "0.231f":
        return float(MIN_ALPHA)
    if name == "below 0.231f":
        return float(np.nextafter(MIN_ALPHA, F(0.0)))
    return float(F(float(name)))


def gain_id(g):
    return "gain%g" % g
