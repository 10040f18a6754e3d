"""CPU checks of the tuned definition (tests/native/tuned_ref.c through tests/tuned_ref.py): the identities that tie it to
the frozen real-tap definition — offset 0 and offset fs / 2 bit for bit, offset fs / 4 within 1e-6 on well-conditioned inputs —, three
stations received from one capture, and how many outputs of every case of tests/test_bcast_tuned_gpu.py sit at the pilot gate."""
import numpy as np
import pytest

import tuned_cases as tc
import tuned_ref as tr
from conftest import scaled_err
from stereo_ref import oracle_d, separation_db

NSAMP = 40000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(pkg, fs):
    return {"random": pkg.make_iq(1, NSAMP, mode="random", fs=fs, first_id=11)[0], "carrier": pkg.make_iq(1, NSAMP, mode="fm", fs=fs, first_id=12)[0],
            "station": pkg.make_iq_rds(1, NSAMP, tc.GROUPS, fs=fs, first_id=13)[0]}


def test_tap_helpers(pkg):
    h = pkg.lowpass_taps(64, 0.05)
    z = pkg.tuned_channel_taps(h, 0.0, 2.4e6)
    assert z.dtype == np.float32 and np.array_equal(z[0::2], h) and not z[1::2].any()
    z = pkg.tuned_channel_taps(h, 600e3, 2.4e6)                     # a quarter of the rate: h[k] j^k up to the rounding of exp
    k = np.arange(64)
    want = h.astype(np.float64) * np.exp(1j * 2 * np.pi * 600e3 * k / 2.4e6)
    assert np.array_equal(z[0::2], want.real.astype(np.float32)) and np.array_equal(z[1::2], want.imag.astype(np.float32))
    assert np.abs((z[0::2] + 1j * z[1::2]) - h * (1j ** (k % 4))).max() <= 1e-9
    assert pkg.tuned_rotation(0.0, 2.4e6, 10) == 0.0
    assert abs(float(pkg.tuned_rotation(100e3, 2.4e6, 10)) - 2 * np.pi * 100e3 * 10 / 2.4e6) <= 3e-7
    assert abs(float(pkg.tuned_rotation(400e3, 2.4e6, 10)) - (2 * np.pi * 400e3 * 10 / 2.4e6 - 4 * np.pi)) <= 3e-7
    for f in (600e3, -600e3, 1.2e6, 123456.7, -1.19e6):
        r = pkg.tuned_rotation(f, 2.4e6, 10)
        assert r.dtype == np.float32 and abs(r) <= tr.PI_F, (f, r)
        assert abs(np.angle(np.exp(1j * (float(r) - 2 * np.pi * f * 10 / 2.4e6)))) <= 1e-6, (f, r)


@pytest.mark.parametrize("T,D", [(64, 10), (64, 8), (64, 7), (16, 8), (7, 3)])
def test_zero_offset_is_the_real_tap_definition_bitwise(pkg, oracle_mod, T, D):
    h = pkg.lowpass_taps(T, 0.05)
    for name, iq in _inputs(pkg, 2.4e6).items():
        want = tr.real_d(iq, h, D)
        got = tr.tuned_d(iq, tr.pairs(h), 0.0, D)
        assert np.array_equal(_bits(got), _bits(want)), (name, T, D)
        e = scaled_err(want, oracle_d(oracle_mod, h, iq, D))
        assert e <= 1e-5, (name, T, D, e)                            # the project's parity bound on d


@pytest.mark.parametrize("T,D", [(64, 10), (64, 8), (16, 8), (7, 4)])
def test_half_rate_is_the_untuned_d_bitwise(pkg, T, D):
    """taps (-1)^k h[k] and bytes x (-1)^n (odd-indexed samples 255 - byte, exact): every product keeps its magnitude and every chain its
    order, y is the untuned y times (-1)^n, and an even D leaves d alone"""
    h = pkg.lowpass_taps(T, 0.05)
    sign = np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for name, iq in _inputs(pkg, 2.4e6).items():
        flipped = iq.copy().reshape(-1, 2)
        flipped[1::2] = 255 - flipped[1::2]
        got = tr.tuned_d(flipped.reshape(-1), tr.pairs(h * sign), 0.0, D)
        assert np.array_equal(_bits(got), _bits(tr.real_d(iq, h, D))), (name, T, D)


@pytest.mark.parametrize("D,rot", [(8, 0.0), (10, -float(tr.PI_F))])
def test_quarter_rate_agrees_within_1e_6_on_signals(pkg, D, rot):
    """taps h[k] j^k and bytes x j^n: y is the untuned y times j^n, d the untuned d plus D pi / 2 — 0 at D = 8, pi at D = 10, which the
    rotation -pi takes off.  The two chains associate differently from the one, so this is no bitwise identity; carrier and station only
    (random bytes give ill-conditioned y's)"""
    h = pkg.lowpass_taps(64, 0.05)
    k = np.arange(64) % 4
    hr = h * np.array([1, 0, -1, 0], np.float32)[k]
    hi = h * np.array([0, 1, 0, -1], np.float32)[k]
    ins = _inputs(pkg, 2.4e6)
    for name in ("carrier", "station"):
        x = ins[name].reshape(-1, 2).astype(np.int32)
        I, Q = x[:, 0], x[:, 1]
        n = np.arange(I.size) % 4
        rI = np.choose(n, [I, 255 - Q, 255 - I, Q])
        rQ = np.choose(n, [Q, I, 255 - Q, 255 - I])
        rotated = np.stack([rI, rQ], 1).astype(np.uint8).reshape(-1)
        got = tr.tuned_d(rotated, tr.pairs(hr, hi), rot, D)
        want = tr.real_d(ins[name], h, D)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("quarter rate, D = %d, %s: worst |d - d untuned| = %.3g" % (D, name, err))
        assert err <= 1e-6, (name, D, err)


def test_three_stations_from_one_capture(pkg):
    """stations at -400, +100 and +600 kHz of one 2.4 MS/s capture, amplitude 40 each: every station's PI and PS exactly, its L/R separation
    measured (tuned_cases.STATIONS_SEPARATION_DB records it; the GPU test asserts that figure minus 1 dB)"""
    iq, sts = tc.three_stations(pkg)
    h, ga, gr, b, dg, rg = tc.shape_taps(pkg, tc.SHAPES["default"])
    seps = []
    for k, st in enumerate(sts):
        d = tr.tuned_d(iq[0], pkg.tuned_channel_taps(h, st["offset_hz"], 2.4e6), pkg.tuned_rotation(st["offset_hz"], 2.4e6, 10), 10)
        r = tr.bcast_ref(d, b, ga, gr, 0.05, dg, rg, 5, 25)
        with pkg.RdsSync(9600.0) as sync:
            info = pkg.rds_parse(sync.push(r["bb"]))
        assert info["pi"] == st["pi"] and info["ps"] == st["ps"], (k, info)
        sl, sr, amps = separation_db(r["L"], r["R"], st["left_hz"], st["right_hz"])
        print("station %d at %+.0f kHz: PI %04X, PS %r, separation %.2f dB in L, %.2f dB in R" % (k, st["offset_hz"] / 1e3, info["pi"], info["ps"], sl, sr))
        seps.append(min(sl, sr))
    for k, v in enumerate(seps):                                    # (deterministic: the record and the measurement agree to the printed digits)
        assert abs(v - tc.STATIONS_SEPARATION_DB[k]) <= 0.05, (seps, "tuned_cases.STATIONS_SEPARATION_DB is out of date")


@pytest.mark.parametrize("case", tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_gate_distance_of_the_gpu_cases(pkg, case):
    """the share of a case's outputs whose window holds a d with its pilot power within 1e-3 pmin2 of the gate stays under the cap the GPU
    test excludes under"""
    su, refs = tc.case_reference(pkg, case)
    frac, _, _, n_amb = tc.case_keeps(su, refs)
    on = [int(r["rds"]["count"]) for r in refs]
    print("%s: %s; d's at the gate %s, gate on for %s of %d d's, %.3f %% of the outputs excluded" % (
        tc.case_id(case), "/".join(su["names"]), n_amb, on, refs[0]["d"].size, 100 * frac))
    assert frac <= tc.EXCLUDED_CAP, frac
    if su["pilot_min"] < 1.0:
        assert any(c > 0 for c, nm in zip(on, su["names"]) if nm == "station") or "station" not in su["names"], "no station opens the gate"
    else:
        assert not any(on), "the shut gate is open"
