"""CPU tests of the spectrum-view oracle (oracle/sdrfm_spectrum_oracle.c): it is the build-defined spec of the FFT view
(the reference has no FFT code: parity unpinned), so it is pinned against an independent float64 FFT and against the
committed golden vectors."""
import glob
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ref(iq, nfft, window):
    x = (iq[0::2].astype(np.float64) - 127.5) + 1j * (iq[1::2].astype(np.float64) - 127.5)
    frames = x.size // nfft
    acc = np.zeros(nfft)
    for f in range(frames):
        acc += np.abs(np.fft.fft(x[f * nfft:(f + 1) * nfft] * window.astype(np.float64))) ** 2
    return np.fft.fftshift(acc / max(frames, 1)), frames


@pytest.mark.parametrize("nfft", [64, 256, 1024, 4096])
def test_oracle_matches_float64_fft(pkg, oracle_mod, nfft):
    iq = pkg.make_iq(1, 5 * nfft + 17, mode="fm", first_id=3)[0]
    hann = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)
    got, frames = oracle_mod.SpectrumOracle(nfft).process(iq)
    want, wf = _ref(iq, nfft, hann)
    assert frames == wf == 5
    assert np.max(np.abs(got - want)) <= 2e-6 * want.max()            # fp32 FFT against float64: ~log2(N) * 2^-24 relative
    got_w, _ = oracle_mod.SpectrumOracle(nfft, hann).process(iq)      # explicit window == default window
    assert np.array_equal(got_w.view(np.uint32), got.view(np.uint32))


def test_tone_lands_in_its_bin_dc_in_the_middle(oracle_mod):
    nfft, k = 1024, 100                                                # +100 bins above DC
    n = np.arange(4 * nfft)
    ph = 2 * np.pi * k * n / nfft
    iq = np.empty(2 * n.size, np.uint8)
    iq[0::2] = np.clip(np.rint(127.5 + 100 * np.cos(ph)), 0, 255)
    iq[1::2] = np.clip(np.rint(127.5 + 100 * np.sin(ph)), 0, 255)
    p, frames = oracle_mod.SpectrumOracle(nfft).process(iq)
    assert frames == 4 and int(p.argmax()) == nfft // 2 + k
    # Hann: coherent gain 0.5 -> peak power (100 * N/2)^2, and the two neighbours are 6 dB down
    assert abs(p[nfft // 2 + k] / (100 * nfft / 2) ** 2 - 1) < 0.02
    assert abs(p[nfft // 2 + k + 1] / p[nfft // 2 + k] - 0.25) < 0.02
    neg = np.empty_like(iq)                                            # conjugate signal -> mirrored bin
    neg[0::2], neg[1::2] = iq[0::2], 255 - iq[1::2]
    assert int(oracle_mod.SpectrumOracle(nfft).process(neg)[0].argmax()) == nfft // 2 - k


def test_edge_cases(oracle_mod):
    o = oracle_mod.SpectrumOracle(256)
    p, frames = o.process(np.zeros(2 * 255, np.uint8))                 # shorter than one frame
    assert frames == 0 and np.all(p == 0)
    p, frames = o.process(np.zeros(0, np.uint8))
    assert frames == 0 and np.all(p == 0)
    with pytest.raises(ValueError):
        o.process(np.zeros(7, np.uint8))                               # odd byte count
    with pytest.raises(ValueError):
        oracle_mod.SpectrumOracle(1000)                                # not a power of two
    mid = np.full(2 * 256 * 3, 128, np.uint8)                          # +0.5 DC on both rails -> only the DC bin (+ Hann skirts)
    p, _ = o.process(mid)
    assert int(p.argmax()) == 128 and p[128 + 2:].max() < 1e-6 * p[128]


def test_golden_vectors(oracle_mod):
    files = sorted(glob.glob(os.path.join(GOLD, "spectrum_*.npz")))
    assert len(files) >= 4
    for fn in files:
        z = np.load(fn)
        win = z["window"] if z["window"].size else None
        got, frames = oracle_mod.SpectrumOracle(int(z["nfft"]), win).process(z["iq"])
        assert frames == int(z["frames"])
        assert np.array_equal(got.view(np.uint32), z["power"].view(np.uint32)), fn


# ---- the oracle against float64 at every size, input class, window and frame-count class of the GPU sweep -------------------------------
from test_spectrum_shapes_gpu import (SIZES, TAIL_FILLS, WINDOWS, case_counts, case_rows, fpr, fpw, hann, make_window, oracle_rows,  # noqa: E402
                                      tail_case, tail_frames, tiled_rows)


def _ref_fast(iq, nfft, window):
    """_ref with the frames transformed in one numpy.fft call; the frame sum in float64"""
    x = (iq[0::2].astype(np.float64) - 127.5) + 1j * (iq[1::2].astype(np.float64) - 127.5)
    frames = x.size // nfft
    p = np.abs(np.fft.fft(x[:frames * nfft].reshape(frames, nfft) * window.astype(np.float64)[None, :], axis=1)) ** 2
    return np.fft.fftshift(p.sum(axis=0) / max(frames, 1)), frames


def _frame_classes(nfft):
    return (1, 5, 2 * fpr(nfft) + 1, 3 * fpr(nfft) + 5, 1000 if nfft <= 1024 else 200)


def _bound(nfft, F):
    """relative to the largest bin of the float64 result.  F <= 100: this file's 2e-6.  Longer averages: the spec's frame sum is a
    sequential fp32 sum of F non-negative terms, relative error at most (F - 1) 2^-24, on top of a per-frame FFT error of the order
    log2(N) 2^-24 in each of the two squared rails: (F + 2 log2 N) 2^-24.  Derived, not measured."""
    return 2e-6 if F <= 100 else (F + 2 * np.log2(nfft)) * 2.0 ** -24


@pytest.mark.parametrize("mode", ["fm", "random", "const", "counter"])
@pytest.mark.parametrize("nfft", SIZES)
def test_oracle_matches_float64_fft_every_size_class_window_and_count(pkg, oracle_mod, nfft, mode):
    """All seven sizes x four input classes x (Hann and the six windows of the GPU sweep) x F in {1, 5, 2 FPR + 1, 3 FPR + 5, 1000 (N <= 1024)
    / 200}.  Observed worst |oracle - float64| / max bin over all of them: 7.4e-7 for F <= 100 (bound 2e-6; 512 points, const input, Hann x
    1e-20, F = 53) and 1.34e-5 for F > 100 (128 points, const input, the signed-noise window, F = 1000: 0.22 of its bound
    (F + 2 log2 N) 2^-24 = 6.0e-5; no case came nearer to its bound than that)."""
    counts = _frame_classes(nfft)
    iq = pkg.make_iq(1, max(counts) * nfft + 17, mode=mode, first_id=31 + nfft)[0]
    worst = {}
    for name in ("hann",) + WINDOWS:
        win = hann(nfft) if name == "hann" else make_window(name, nfft)
        o = oracle_mod.SpectrumOracle(nfft, win)
        for F in counts:
            part = iq[:2 * (F * nfft + 8)]
            got, frames = o.process(part)
            want, wf = _ref_fast(part, nfft, win)
            assert frames == wf == F
            assert np.all(np.isfinite(got))
            err = float(np.max(np.abs(got - want)) / want.max())
            key = "F<=100" if F <= 100 else "F>100"
            if err / _bound(nfft, F) > worst.get(key, (0, 0, 0))[0]:
                worst[key] = (err / _bound(nfft, F), err, (name, F))
            assert err <= _bound(nfft, F), (nfft, mode, name, F, err, _bound(nfft, F))
        o.close()
    print("nfft %d %s: worst error / bound %s" % (nfft, mode, {k: "%.3g (%.3g of the bound) at %s" % (v[1], v[0], v[2]) for k, v in worst.items()}))


@pytest.mark.parametrize("byte", [0, 255])
@pytest.mark.parametrize("nfft", SIZES)
def test_oracle_on_constant_rails_matches_float64(oracle_mod, nfft, byte):
    """all-0 and all-255 bytes: -127.5 / +127.5 on both rails, the largest inputs there are"""
    for F in (1, 5):
        iq = np.full(2 * F * nfft, byte, np.uint8)
        for name in ("hann",) + WINDOWS:
            win = hann(nfft) if name == "hann" else make_window(name, nfft)
            got, frames = oracle_mod.SpectrumOracle(nfft, win).process(iq)
            want, _ = _ref_fast(iq, nfft, win)
            assert frames == F and np.max(np.abs(got - want)) <= 2e-6 * want.max(), (nfft, byte, name, F)


@pytest.mark.parametrize("mode", ["fm", "random", "counter"])
@pytest.mark.parametrize("wname", ["hann", "ramp", "noise"])
def test_oracle_matches_the_dft_definition(pkg, oracle_mod, mode, wname):
    """64 points, one frame, against X[k] = sum_n x[n] exp(-2 pi j k n / N) written out as an O(N^2) sum in float64: the bin order (DC in
    the middle: out[i] = |X[(i + N/2) mod N]|^2) and the sign of the exponent are pinned by something that shares no code with an FFT."""
    nfft = 64
    win = hann(nfft) if wname == "hann" else make_window(wname, nfft)
    iq = pkg.make_iq(1, nfft, mode=mode, first_id=77)[0]
    x = ((iq[0::2].astype(np.float64) - 127.5) + 1j * (iq[1::2].astype(np.float64) - 127.5)) * win.astype(np.float64)
    want = np.zeros(nfft)
    for i in range(nfft):
        k = (i + nfft // 2) % nfft
        acc = 0j
        for n in range(nfft):
            acc += x[n] * complex(np.cos(2 * np.pi * k * n / nfft), -np.sin(2 * np.pi * k * n / nfft))
        want[i] = acc.real ** 2 + acc.imag ** 2
    got, frames = oracle_mod.SpectrumOracle(nfft, win).process(iq)
    assert frames == 1
    assert np.max(np.abs(got - want)) <= 2e-6 * want.max()
    if mode != "counter" or wname != "hann":
        mirrored = np.roll(want[::-1], 1)                              # what the other sign of the exponent would give
        assert np.max(np.abs(got - mirrored)) > 1e-3 * want.max()    # (the inputs tell the two conventions apart)


@pytest.mark.parametrize("nfft", SIZES)
def test_case_builders_of_the_gpu_sweep_against_the_oracle_alone(pkg, oracle_mod, nfft):
    """tests/test_spectrum_shapes_gpu.py builds its cases without a device: frame counts as expected, finite non-zero spectra for every
    window, the three tail fills differ only outside the rows, tiled rows repeat"""
    counts = case_counts(nfft)
    assert counts[0] == 1 and counts[-1] == 3 * fpr(nfft) + 5 and all(c > 0 for c in counts) and len(set(counts)) == len(counts)
    assert fpr(nfft) % fpw(nfft) == 0 and fpw(nfft) == max(1, 1024 // nfft)
    for F in (counts[0], counts[len(counts) // 2], counts[-1]):
        iq = case_rows(pkg, nfft, F, 3, 2000 + 7 * F)
        assert iq.shape == (3, 2 * (F * nfft + 7))
        assert not np.array_equal(iq[0], iq[1]) and not np.array_equal(iq[1], iq[2])
        oracle_rows(oracle_mod, nfft, iq, frames=F)
    iq = case_rows(pkg, nfft, 3 * fpw(nfft) + 1, 2, 6000 + nfft)
    for name in WINDOWS:
        win = make_window(name, nfft)
        assert win.dtype == np.float32 and win.shape == (nfft,) and np.all(np.isfinite(win))
        p = oracle_rows(oracle_mod, nfft, iq, win, frames=3 * fpw(nfft) + 1)
        assert np.all(np.isfinite(p)) and np.all(p >= 0) and p.max() > 0, name
    assert np.any(make_window("ramp", nfft) != make_window("ramp", nfft)[::-1]) and np.any(make_window("noise", nfft) < 0)
    assert int((make_window("hann_holes", nfft) == 0).sum()) >= nfft // 2
    F, seen = tail_frames(nfft), []
    assert F % fpw(nfft) == 1 % fpw(nfft) and F % 2 == 1 and F >= 2 * fpw(nfft) + 1
    for fill in TAIL_FILLS:
        for offset in (0, 1, 2):
            buf, at, stride, nbytes, rows = tail_case(pkg, nfft, offset, 0, fill)
            assert nbytes == 2 * F * nfft and stride - nbytes > 2048 and at % 4 == offset
            mask = np.ones(buf.size, bool)
            for s in range(rows.shape[0]):
                assert np.array_equal(buf[at + s * stride:at + s * stride + nbytes], rows[s])
                mask[at + s * stride:at + s * stride + nbytes] = False
            if fill != "random":
                assert np.all(buf[mask] == (0 if fill == "zeros" else 255))
            else:
                assert np.unique(buf[mask]).size > 200
        seen.append(rows)
    assert all(np.array_equal(r, seen[0]) for r in seen)
    tiled, rows = tiled_rows(pkg, nfft, 2, 30, 8000 + nfft)
    assert tiled.shape == (30, 4 * nfft) and np.array_equal(tiled[12:24], rows) and np.array_equal(tiled[24:], rows[:6])
    assert len({r.tobytes() for r in rows}) == 12
