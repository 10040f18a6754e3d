"""CPU checks of the RDS definition (tests/rds_ref.py on the oracle's d) with the C decoder behind it: a synthetic station's groups come
back block by block, at any phase of the subcarrier against the pilot's third harmonic and with the crystal 100 ppm off; the
fp32-faithful reference against its float64 restatement."""
import numpy as np
import pytest

from rds_ref import check_blocks, oracle_d, rds_ref, station_samples

FS, D, DR = 2.4e6, 10, 25
PI, PS, TEXT = 0xD3C2, "GRAFT FM", "RDS on the GPU.."
CASES = {"phase0": (0.0, 0.0, 12), "phase0.3": (0.3, 0.0, 12), "quadrature": (np.pi / 2, 0.0, 12),
         "plus100ppm": (0.6, 100.0, 40), "minus100ppm": (0.0, -100.0, 40)}


@pytest.fixture(scope="module")
def rds_setup(pkg):
    return pkg.lowpass_taps(64, 120e3 / FS), pkg.stereo_pilot_taps(101, FS / D), pkg.rds_lowpass_taps(255, FS / D), pkg.rds_gain(D, FS)


def test_rds_gain_compensates_the_discriminator_boxcar(pkg):
    gain = pkg.rds_gain(10, 2.4e6)
    x = np.pi * 57e3 / 2.4e6
    assert abs(gain - 2.0 * 10 * np.sin(x) / np.sin(10 * x)) <= 1e-6
    assert abs(2.0 / gain - 0.91061) <= 5e-6 and abs(gain - 2.1963) <= 5e-5      # the figures quoted in DESIGN.md §4.9
    g = pkg.rds_lowpass_taps(255, 240e3)
    assert g.shape == (255,) and np.array_equal(g, pkg.lowpass_taps(255, 3e3 / 240e3))


@pytest.mark.parametrize("case", sorted(CASES))
def test_station_groups_come_back_block_by_block(pkg, oracle_mod, rds_setup, case):
    """100 of 127.5 amplitude, N(0, 4) noise, 75 kHz deviation, RDS at 3 kHz, programme tones present, carrier offset drawn per stream"""
    h, b, g, gain = rds_setup
    phase, ppm, n_groups = CASES[case]
    sent = pkg.rds_encode_groups(PI, PS, TEXT, pty=10)
    iq = pkg.make_iq_rds(1, station_samples(n_groups), sent, rds_phase=phase, clock_ppm=ppm, first_id=40 + sorted(CASES).index(case))[0]
    r = rds_ref(oracle_d(oracle_mod, h, iq, D), b, g, 0.05, gain, DR)
    with pkg.RdsSync(FS / D / DR) as sync:
        got = sync.push(r["w"])
        st = sync.stats()
    first, n_ok = check_blocks(sent, got, n_groups, case)
    info = pkg.rds_parse(got)
    print("%s: |q| %.3f rad, RMS |w| %.3g, first reported group %d, %d blocks ok of %d groups sent, stats %s" % (
        case, float(np.sqrt(r["pw"][2000:].mean())), float(np.sqrt(np.mean(np.abs(r["w"][50:]) ** 2))), first, n_ok, n_groups, st))
    assert info == dict(pi=PI, pty=10, ps=PS, text=TEXT), info
    assert st["in_sync"] and st["blocks_failed"] == 0


def test_reference_is_fp32_faithful_restatement(pkg, oracle_mod, rds_setup):
    h, b, g, gain = rds_setup
    sent = pkg.rds_encode_groups(PI, PS, TEXT)
    worst_abs, worst_rel = 0.0, 0.0
    for s in range(2):
        iq = pkg.make_iq_rds(1, 600000, sent, rds_phase=0.7 * s, first_id=60 + s)[0]
        d = oracle_d(oracle_mod, h, iq, D)
        r32 = rds_ref(d, b, g, 0.05, gain, DR)
        r64 = rds_ref(d, b, g, 0.05, gain, DR, exact64=True)
        near = np.abs(r64["pw"] - float(r32["pmin2"])) <= 1e-3 * float(r32["pmin2"])
        assert np.array_equal(r32["on"], r64["on"]) or near.any()
        assert np.array_equal(r32["on"][~near], r64["on"][~near])
        rms = float(np.sqrt(np.mean(np.abs(r64["w"][50:]) ** 2)))
        err = float(np.abs(r32["w"].astype(np.complex128) - r64["w"]).max()) if not near.any() else float(
            np.abs(r32["w"].astype(np.complex128) - r64["w"])[50:].max())
        first_on = int(np.argmax(r32["on"]))
        print("stream %d: fp32 against exact64 worst %.3g absolute, %.3g of RMS |w| = %.3g; %d d's within 1e-3 of the gate, gate on from d[%d]" % (
            s, err, err / rms, rms, int(near.sum()), first_on))
        worst_abs, worst_rel = max(worst_abs, err), max(worst_rel, err / rms)
    # 255 fmaf's over |g z| <= 0.01 each and the roundings of z (4 of 6e-8 relative on |z| <= 0.6, summed over sum|g| = 1.3) stay below 1e-6
    assert worst_abs <= 1e-6, worst_abs


def test_mono_station_gives_no_baseband_and_no_groups(pkg, oracle_mod, rds_setup):
    h, b, g, gain = rds_setup
    sent = pkg.rds_encode_groups(PI, PS, TEXT)
    iq = pkg.make_iq_rds(1, int(2.05 * FS), sent, pilot=False, first_id=70)[0]
    r = rds_ref(oracle_d(oracle_mod, h, iq, D), b, g, 0.05, gain, DR)
    ramp = 2 * b.size
    assert not r["on"][ramp:].any()
    behind = (ramp + g.size) // DR + 1
    assert not r["w"][behind:].any()
    with pkg.RdsSync(FS / D / DR) as sync:
        assert sync.push(r["w"]) == []
        assert sync.stats()["groups"] == 0
