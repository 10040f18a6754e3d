"""CPU checks of the stereo definition (tests/stereo_ref.py on the oracle's d): it separates the channels, in the right order, and
stays L == R without a pilot."""
import numpy as np
import pytest

from stereo_ref import oracle_d, separation_db, stereo_ref

FS, D, DA = 2.4e6, 10, 5


@pytest.fixture(scope="module")
def stereo_setup(pkg):
    h = pkg.lowpass_taps(64, 120e3 / FS)
    g = pkg.default_config()[1]
    b = pkg.stereo_pilot_taps(101, FS / D)
    return h, g, b


@pytest.fixture(scope="module")
def decoded_d(pkg, oracle_mod, stereo_setup):
    h = stereo_setup[0]
    iq = pkg.make_iq_stereo(1, 240000, 1e3, 3.1e3, 50e3, first_id=3)[0]
    return oracle_d(oracle_mod, h, iq, D)


def test_diff_gain_compensates_the_discriminator_boxcar(pkg):
    gain = pkg.stereo_diff_gain(10, 2.4e6)
    x = np.pi * 38e3 / 2.4e6
    assert abs(gain - 2.0 * 10 * np.sin(x) / np.sin(10 * x)) <= 1e-6
    assert abs(2.0 / gain - 0.95967) <= 5e-6                   # H_D(38 kHz) at D = 10, 2.4 MS/s, to the 5 digits quoted in DESIGN.md
    assert abs(gain / (2.0 / 0.95967) - 1.0) <= 5.3e-6           # (the quoted 0.95967 is that value rounded: its relative error)


def test_pilot_taps_measure_the_pilot_amplitude(pkg, stereo_setup):
    b = stereo_setup[2]
    assert b.shape == (101,) and np.iscomplexobj(b)
    t = np.arange(4000)
    d = (0.2 * np.sin(2 * np.pi * 19e3 / 240e3 * t)).astype(np.float32)
    r = stereo_ref(d, b, np.ones(1, np.float32), 0.05, 2.0, Da=1)
    assert abs(np.sqrt(r["pw"][2000:]).mean() - 0.2) < 2e-3


@pytest.mark.parametrize("dg_name,min_db", [("compensated", 40.0), ("textbook", 30.0)])
def test_reference_separates_the_channels(pkg, stereo_setup, decoded_d, dg_name, min_db):
    h, g, b = stereo_setup
    dg = pkg.stereo_diff_gain(D, FS) if dg_name == "compensated" else 2.0
    r = stereo_ref(decoded_d, b, g, 0.05, dg, DA)
    sep_l, sep_r, amps = separation_db(r["L"], r["R"])
    print("diff_gain %.4f: separation L %.1f dB, R %.1f dB" % (dg, sep_l, sep_r))
    assert sep_l >= min_db and sep_r >= min_db, (sep_l, sep_r)
    l_l, l_r, r_l, r_r = amps
    assert l_l > 10 * r_l and r_r > 10 * l_r                  # not swapped
    assert r["count"] >= 0.99 * decoded_d.size


def test_reference_is_fp32_faithful_restatement(pkg, stereo_setup, decoded_d):
    h, g, b = stereo_setup
    dg = pkg.stereo_diff_gain(D, FS)
    r32 = stereo_ref(decoded_d, b, g, 0.05, dg, DA)
    r64 = stereo_ref(decoded_d, b, g, 0.05, dg, DA, exact64=True)
    ok = r32["on"] == r64["on"]
    assert ok.mean() > 0.999
    for ch in ("L", "R"):
        err = np.abs(r32[ch].astype(np.float64) - r64[ch]) / np.maximum(np.abs(r64[ch]), 1.0)
        assert err.max() <= 1e-6, (ch, err.max())


@pytest.mark.parametrize("source", ["no_pilot", "mono_fm"])
def test_mono_inputs_give_no_pilot_and_l_equals_r(pkg, oracle_mod, stereo_setup, source):
    h, g, b = stereo_setup
    if source == "no_pilot":
        iq = pkg.make_iq_stereo(1, 120000, 1e3, 3.1e3, 50e3, pilot=False, first_id=5)[0]
    else:
        iq = pkg.make_iq(1, 120000, mode="fm", first_id=5)[0]
    d = oracle_d(oracle_mod, h, iq, D)
    r = stereo_ref(d, b, g, 0.05, pkg.stereo_diff_gain(D, FS), DA)
    # the stream's first d's step from 0 to the carrier offset's DC: the pilot filter's ramp-up (its first 2P d's) may cross pilot_min
    # briefly; after it, no d of a mono input does, and every output whose windows hold no crossing has L == R bit for bit
    P, ramp = b.size, 2 * b.size
    on = r["on"]
    print("%s: %d crossings in the ramp-up, max |q| after it %.4f rad" % (source, int(on[:ramp].sum()), float(np.sqrt(r["pw"][ramp:].max()))))
    assert not on[ramp:].any()
    first = (ramp + g.size + P) // DA + 1
    assert np.array_equal(r["L"][first:], r["R"][first:])
    if not on.any():
        assert r["count"] == 0 and np.array_equal(r["L"], r["R"])
