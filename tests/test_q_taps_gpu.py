"""Design Q (csrc/sdrfm_q.hip: k_mfir, k_mfir_pcm, k_mix) held to the oracle at the channel-tap counts sdrfm_create offers it but no other test ran.

sdrfm_create offers design Q to every low-pass channel filter of T <= 64 taps at (D, Da) = (10, 5), (8, 8), (16, 5); the rest of the suite runs it at
T in {16, 32, 48, 64}.  The tap count is no harmless parameter of this kernel:
  * the template argument C0 skips the first 128-byte K-chunk of a block's window when no tap lies there: first chunk = floor((9 D - T) / 64), clamped to 1 —
    1 for T <= 26 at D = 10, T <= 8 at D = 8, always at D = 16.  k_mfir<1,4,8,8>, k_mfir_pcm<1,4,8,8> and k_mix<1,4,8,8,16,4> ran in no test before this file,
    and the 26 / 27 switch at D = 10 was met at 16 and 32 only.  The chunk follows the taps' DIGITS (csrc/qtaps.c), so 32 taps whose outer ones quantise
    to zero land on C0 = 1 as well (tests/q_tap_sets.py: the value-dependent sets; tests/test_q_tables.py holds the tables themselves on the CPU);
  * T - 1 sizes the carried input (the stream's first run loads T - 1 byte pairs per stream, the last run hands T - 1 over from the ring; T = 1: nothing),
    the repair path's taps are h padded to 64, the first call's fix-up covers (T + D - 1) / D + 1 outputs;
  * design B exists for T in {16, 32, 64} only: for every other T the bit-exact side of a design-Q handle — calls design Q cannot take, the first call's
    fix-up, routed streams — is the generic kernel.
Every test prints its figures (pytest -s)."""
import functools
import importlib

import numpy as np
import pytest

import pcm_params as pp
import q_tap_sets as qt
import test_pcm_oracle_gpu as og
import test_route_gpu as rg
from conftest import scaled_err, TOL

pytestmark = pytest.mark.gpu

NS, ND = 264, 12                                                    # streams; distinct rows, tiled
Q_STEP_OUT, Q_TA = 128, 32                                          # decimated outputs per wave step; audio taps (csrc/sdrfm_q.h)
NSLOT = {10: 5, 8: 4, 16: 8}                                        # the ring size in KiB the library launches per rate (sdrfm_q_default_nslot)

PLAIN = ([(T, 10) for T in (1, 2, 9, 10, 11, 17, 25, 26, 27, 28, 33, 47, 63)] +
         [(T, 8) for T in (1, 2, 7, 8, 9, 10, 17, 33, 63)] +
         [(T, 16) for T in (1, 2, 15, 16, 17, 18, 31, 33, 63)])
CASES = [("T%d-D%d" % td, td) for td in PLAIN] + [(name, name) for name in qt.VALUE_SETS]


def _pkg():
    return importlib.import_module("stm32f7-rtlsdr_amd")


def _case(pkg, case):
    """-> h, g, D, Da, the first chunk sdrfm_q_build reports"""
    if isinstance(case, str):
        h, g, D, _ = qt.value_taps(pkg, case)
        rc, _, _, _, c0 = qt.q_build(pkg, h, D)                      # (tests/test_q_tables.py: it is the chunk the digits imply)
        assert rc == 0
    else:
        T, D = case
        h, g = qt.plain_taps(pkg, T, D)
        c0 = qt.first_chunk_by_count(T, D)
    assert qt.create_offers_design_q(pkg, h, g, D)                   # sdrfm_create's conditions on the taps hold: a default handle has design Q
    return h, g, D, qt.RATES[D][0], c0


def _symbol(c0, D, Da):
    c0 = min(1, c0)                                                  # (sdrfm_create and q_find clamp: D = 16 has no tap in chunk 1 either below T = 17)
    return "k_mfir<%d,5>" % c0 if D == 10 else "k_mfir<%d,%d,%d,%d>" % (c0, NSLOT[D], D, Da)


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _first_call_units(T, D, Da):
    """the smallest whole number of U = 8 D Da samples that gives every stream two steps and that design Q takes on a zero history (csrc/sdrfm_fm_call.h:
    fm_q_fit — M >= fm_y_aff + Ta, and n_streams x steps >= 2 x CUs, which must then hold with two steps: checked, not assumed)"""
    y_aff = (T + D - 1) // D + 1
    k = 1
    while not (-(-(8 * Da * k) // Q_STEP_OUT) >= 2 and 8 * Da * k >= max(Q_TA, y_aff + Q_TA)):
        k += 1
    steps = -(-(8 * Da * k) // Q_STEP_OUT)
    assert NS * steps >= 2 * _n_cu(), "the first call (%d steps per stream x %d streams) does not fill this device's %d CUs twice" % (steps, NS, _n_cu())
    return k


def _plan(T, D, Da):
    """call sizes in samples: a minimal first call, several runs per stream, two calls design Q cannot take (together whole audio periods again: the generic
    kernel takes over design Q's carried input and hands it back), design Q on the generic kernel's state, and a longer call"""
    unit = 8 * D * Da
    back = (1000 // unit + 1) * unit - 1000                          # (2 unit - 1000 at D = 8 and 16; 3 unit - 1000 at D = 10, where 2 unit < 1000)
    return [_first_call_units(T, D, Da) * unit, 60 * unit, 1000, back, 7 * unit, 30 * unit]


@functools.lru_cache(maxsize=None)
def _rows(D, nsamp):
    """twelve distinct rows (shared, read-only): six carriers at the rate's fs, three rows of noise, a constant, a counter, and alternating bytes 127 / 128 —
    x = (-0.5, +0.5) throughout, |y| components 0.5 |sum h|: below the guard's radius for every T >= 2, so every lane of every step is repaired and the
    repair list is as full as it gets.  (tests/test_q_guard_gpu.py's periodic class, tools/q_classes.py, holds random square waves and short sequences;
    no row of this kind.)"""
    pkg = _pkg()
    fs = qt.RATES[D][1]
    alt = np.tile(np.array([127, 128], np.uint8), nsamp)[None, :]
    rows = np.concatenate([pkg.make_iq(6, nsamp, mode="fm", fs=fs, first_id=600), pkg.make_iq(3, nsamp, mode="random", first_id=650),
                           pkg.make_iq(1, nsamp, mode="const", first_id=660), pkg.make_iq(1, nsamp, mode="counter", first_id=670), alt])
    assert rows.shape == (ND, 2 * nsamp)
    rows.setflags(write=False)
    return rows


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_matrix_pipe_kernel_at_every_tap_count_class(pkg, oracle_mod, case):
    """One (taps, rate): the call plan of _plan on a default handle and on a bit-exact twin, then three device-buffer runs of the same 120 units.
    (a) kernel_name starts with fast-q exactly on the calls design Q can take, names T and the k_mfir<C0,...> instance of the first chunk; the twin never does;
    (b) every distinct row's whole stream is the oracle's at TOL; (c) within 2e-6 of the twin (the figure of the two existing design-Q tests);
    (d) tiled copies bit-identical; (e) one call, three serial calls and three overlapped calls give the same bits; (f) after reset() the first call's bits again."""
    import torch
    h, g, D, Da, c0 = _case(pkg, case)
    T, unit = h.size, 8 * D * Da
    calls = _plan(T, D, Da)
    total, nb = sum(calls), 40 * unit
    rows = _rows(D, max(total, 3 * nb))
    iq = np.tile(rows, (NS // ND, 1))
    sym = _symbol(c0, D, Da)
    kw = dict(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=NS, max_bytes_per_call=2 * max(calls))
    with pkg.FmDemod(pkg.FmConfig(**kw)) as fast, pkg.FmDemod(pkg.FmConfig(bit_exact=True, **kw)) as exact:
        pos, names, a_fast, a_exact = 0, [], [], []
        for n in calls:
            a_fast.append(fast.process_batch(iq[:, 2 * pos:2 * (pos + n)]))
            names.append(fast.kernel_name)
            a_exact.append(exact.process_batch(iq[:, 2 * pos:2 * (pos + n)]))
            assert not exact.kernel_name.startswith("fast-q"), exact.kernel_name
            pos += n
        st = fast.q_guard()
        fast.reset()
        again = fast.process_batch(iq[:, :2 * calls[0]])
        name_again = fast.kernel_name
    a_fast, a_exact = np.concatenate(a_fast, axis=1), np.concatenate(a_exact, axis=1)
    assert a_fast.shape == (NS, total // (D * Da))
    # every figure printed before anything is asserted
    want = np.stack([oracle_mod.Oracle(h, g, D, Da).process(rows[s_]) for s_ in range(ND)])     # (streaming: a prefix of the capture gives a prefix of the audio)
    e_or = [scaled_err(a_fast[s_], want[s_, :a_fast.shape[1]]) for s_ in range(ND)]
    e_tw = scaled_err(a_fast, a_exact)
    print("%s: T %d D %d Da %d, %s, first call %d units; worst scaled error against the oracle %.3g (row %d), against the bit-exact twin %.3g; %d lanes repaired; %s" % (
        case if isinstance(case, str) else "plain", T, D, Da, sym, calls[0] // unit, max(e_or), int(np.argmax(e_or)), e_tw, st["lanes"],
        [n_.split()[0] for n_ in names]))
    # (a)
    for n, name in zip(calls, names):
        assert name.startswith("fast-q") == (n % unit == 0), (n, names)
        if n % unit == 0:
            assert name == "fast-q T%d D%d Ta%d Da%d %s" % (T, D, Q_TA, Da, sym), name
    assert name_again == names[0], name_again
    # (b), (c)
    assert max(e_or) <= TOL, e_or
    assert e_tw <= 2e-6, e_tw
    if T >= 2:
        assert st["lanes"] > 0, st                                   # (the alternating row: nothing but repairs)
    # (d)
    for rep in range(1, NS // ND):
        assert np.array_equal(_bits(a_fast[ND * rep:ND * rep + ND]), _bits(a_fast[:ND])), rep
    # (f)
    assert np.array_equal(_bits(again), _bits(a_fast[:, :calls[0] // (D * Da)]))
    # (e) partition invariance and overlapped calls, on device-resident buffers
    dev = torch.from_numpy(np.ascontiguousarray(iq[:, :2 * 3 * nb])).cuda()
    outs = []
    for cuts, ovl in (([3 * nb], False), ([nb, nb, nb], False), ([nb, nb, nb], True)):
        bufs = [torch.zeros((NS, c // (D * Da)), dtype=torch.float32, device="cuda") for c in cuts]
        torch.cuda.synchronize()
        with pkg.FmDemod(pkg.FmConfig(**dict(kw, max_bytes_per_call=2 * 3 * nb))) as dm:
            p0 = 0
            for c, b in zip(cuts, bufs):
                assert dm.process_batch_device(dev[:, 2 * p0:], b, nbytes=2 * c, overlap=ovl) == c // (D * Da)
                assert dm.kernel_name.startswith("fast-q") and sym in dm.kernel_name, dm.kernel_name
                p0 += c
            if ovl:
                assert "overlapped" in dm.kernel_name, dm.kernel_name
            dm.synchronize()
        outs.append(torch.cat(bufs, dim=1).cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(outs[0]), _bits(outs[2]))
    # (the device-buffer runs start the same stream: the oracle's once more, so that (e) cannot pass on three equally wrong runs)
    assert scaled_err(outs[0][:ND], want[:, :3 * nb // (D * Da)]) <= TOL


@pytest.mark.parametrize("T,D", [(7, 8), (9, 8), (26, 10), (27, 10), (17, 16)])
def test_pcm_chain_inside_the_launch_at_one_tap_count_per_instance(pkg, oracle_mod, T, D):
    """k_mfir_pcm<C0,...>, one T per (rate, C0) instance — (7, 8) is k_mfir_pcm<1,4,8,8>, which no other test runs: two host-buffer calls, of >= 13 quads and of two runs, with a
    mono sink at the default alpha and gain.  The second call holds the sink's chain in the launch (the stream's first call never does: csrc/sdrfm_fm_call.h
    fm_chain_fits; the sink's own kernel follows it).  The PCM and the carried state against the host routine over the handle's OWN float audio, at the chain
    case's caps of tests/test_pcm_sink_params_gpu.py: 1 LSB, state within 1e-6 max(|st|, 0.25); that audio against the oracle at TOL.
    (The second call is cut into two runs of csrc/sdrfm_fm_call.h's fm_chain_run_quads.  While the host counted 13 quads per run at every rate, the 832 outputs this
    test first gave the D = 8 cases went out as two runs of 52 audio outputs — fewer than the 64 a predecessor's state reaches — and the carried state was 1.13e-6
    off, over the cap: tests/test_pcm_chain_cpu.py holds the run length on the CPU now.)"""
    h, g, D, Da, c0 = _case(pkg, (T, D))
    unit = 8 * D * Da
    run_quads = 1 + max(12, -(-(64 + 2) * Da // 32))                            # csrc/sdrfm_fm_call.h fm_chain_run_quads: 13 at Da = 5, 18 at Da = 8
    calls = [(400 // (8 * Da) + 2) * unit, -(-64 * run_quads // (8 * Da)) * unit]  # 480 and 840 outputs at Da = 5, 512 and 1152 at Da = 8
    quads = [((n // D + 7) // 8 + 3) // 4 for n in calls]                        # fm_q_quads
    assert quads[0] >= 13 and quads[1] >= 2 * run_quads                          # (two runs per stream: the second finishes its first outputs with the first's state)
    alpha, gain = og._params(pkg)
    assert gain == pp.DEFAULT_GAIN
    rows = _rows(D, 120 * unit)
    iq = np.tile(rows, (NS // ND, 1))
    pos, pcm, aud, names = 0, [], [], []
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=NS, max_bytes_per_call=2 * max(calls))) as dm, \
            pkg.PcmSink(NS, alpha, gain) as sink:
        for n in calls:
            p, a = dm.process_batch_pcm(sink, iq[:, 2 * pos:2 * (pos + n)], want_audio=True)
            pcm.append(p); aud.append(a); names.append(dm.kernel_name)
            pos += n
        assert sink.synchronize_status() == 0
        st_dev = sink.state().astype(np.float64)
    sym = _symbol(c0, D, Da)
    assert names[0] == "fast-q T%d D%d Ta%d Da%d %s" % (T, D, Q_TA, Da, sym), names
    assert names[1] == names[0] + " + pcm", names                                # k_mfir_pcm of the same instance
    for k, n in enumerate(calls):
        assert aud[k].shape == (NS, n // (D * Da)) and pcm[k].shape == (NS, 2 * aud[k].shape[1])
        assert np.array_equal(_bits(np.tile(aud[k][:ND], (NS // ND, 1))), _bits(aud[k])), k
    want_a = np.stack([oracle_mod.Oracle(h, g, D, Da).process(rows[s_, :2 * sum(calls)]) for s_ in range(ND)])
    e_or = scaled_err(np.concatenate([a[:ND] for a in aud], axis=1), want_a)
    want, st = og.host_pcm(pkg, [a[:ND] for a in aud], alpha, gain)
    rows_of = np.arange(NS) % ND
    worst = max(int(np.abs(pcm[k].astype(np.int32) - want[k][rows_of].astype(np.int32)).max()) for k in range(2))
    rel = float(np.max(np.abs(st_dev - st[rows_of]) / np.maximum(np.abs(st[rows_of]), 0.25)))
    print("T %d D %d Da %d: %s, then %s; audio %.3g off the oracle; worst PCM %d LSB, state %.3g relative (largest |PCM| %d)" % (
        T, D, Da, names[0], names[1], e_or, worst, rel, max(int(np.abs(w).max()) for w in want)))
    assert e_or <= TOL, e_or
    assert max(int(np.abs(w).max()) for w in want) > 1000                        # (the carriers' audio is not silence)
    for k in range(2):
        assert np.array_equal(pcm[k][:, 0::2], pcm[k][:, 1::2]), k               # L = R
    assert worst <= 1, worst
    assert rel <= 1e-6, rel


@pytest.mark.parametrize("case", ["16-tail-zero", (27, 10), (9, 8)], ids=["16-tail-zero", "T27-D10", "T9-D8"])
def test_routed_streams_at_tap_counts_without_a_design_b_tile_and_the_unreached_one_launch_instance(pkg, oracle_mod, case):
    """tests/test_route_gpu.py's test_the_one_launch_kernel_at_the_other_front_end_rates at three more tap sets: every third stream routed by the test hook from
    the second call on, serial and overlapped calls.  16 taps at D = 8 whose last eight are zero: design B has a tile, the first chunk is 1 — one launch, of
    k_mix<1,4,8,8,16,4>, an instance reachable only with such taps.  27 taps at D = 10 and 9 at D = 8: no design-B tile, the generic kernel serves the routed
    streams in a launch of its own.  Routed streams carry a bit-exact handle's bits, the others an all-design-Q handle's from the call after the change on;
    a carrier and a row of noise on either side against the oracle at TOL."""
    import torch
    h, g, D, Da, c0 = _case(pkg, case)
    T, one_launch = h.size, isinstance(case, str)
    ns, nsamp, ncalls = 192, D * Da * 8 * 60, 5
    iq, _, _, _, _ = rg._mixed_rows(pkg, ns, ncalls * nsamp, 7, first_id=3400 + T + D)
    dev = torch.from_numpy(iq).cuda()
    mask = np.array([1 if s % 3 == 1 else 0 for s in range(ns)], dtype=np.uint8)
    na = nsamp // (D * Da)
    q_name = "fast-q T%d D%d Ta%d Da%d %s" % (T, D, Q_TA, Da, _symbol(c0, D, Da))
    outs = {}
    for tag, cfg, ovl in (("q", {}, False), ("x", {"bit_exact": True}, False), ("serial", {}, False), ("overlapped", {}, True)):
        out = torch.zeros((ncalls, ns, na), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=ns, max_bytes_per_call=2 * nsamp, **cfg)) as dm:
            for k in range(ncalls):
                if tag in ("serial", "overlapped") and k == 1:
                    assert np.array_equal(dm.route(mask), mask)
                assert dm.process_batch_device(dev[:, 2 * k * nsamp:], out[k], nbytes=2 * nsamp, overlap=ovl) == na
                name = dm.kernel_name
                if tag == "x":
                    assert not name.startswith("fast-q"), name
                elif tag == "q" or k == 0:
                    assert name == q_name + (" overlapped" if ovl and k else ""), name
                else:
                    want = "%s%s + %s (64 streams)%s" % (q_name, " overlapped" if ovl else "", "fast-b" if one_launch else "generic", " in one launch" if one_launch else "")
                    assert name == want, (name, want)
            dm.synchronize()
        outs[tag] = out.cpu().numpy()
    on_q = mask == 0
    for tag in ("serial", "overlapped"):
        m = _bits(outs[tag])
        assert np.array_equal(m[:1], _bits(outs["q"])[:1]), tag                  # before the change: design Q for all
        assert np.array_equal(m[2:][:, ~on_q], _bits(outs["x"])[2:][:, ~on_q]), tag
        assert np.array_equal(m[2:][:, on_q], _bits(outs["q"])[2:][:, on_q]), tag
    worst = 0.0
    for s in (0, 4, 1, 8):                                                       # a carrier on design Q, a routed carrier, routed noise, noise on design Q
        assert (bool(mask[s]), s % 7 == 1) == {0: (False, False), 4: (True, False), 1: (True, True), 8: (False, True)}[s]
        want = oracle_mod.Oracle(h, g, D=D, Da=Da).process(iq[s])
        for tag in ("serial", "overlapped"):
            e = scaled_err(np.concatenate([outs[tag][k, s] for k in range(ncalls)]), want)
            worst = max(worst, e)
            assert e <= TOL, (tag, s, e)
    print("%s: T %d D %d Da %d: %s + %s (64 of %d streams)%s; worst scaled error against the oracle %.3g" % (
        case, T, D, Da, q_name, "fast-b" if one_launch else "generic", ns, " in one launch" if one_launch else ", two launches", worst))
