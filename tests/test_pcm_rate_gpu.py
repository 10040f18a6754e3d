"""The PCM rate matcher on the device, against tests/pcm_rate_ref.py — the int64 numpy restatement of the definition — and the host
routine sdrfm_pcm_rate_s16.  Every comparison of samples, counts and pos is integer equality; hist is held through the outputs of the call
that follows.  Nothing here has a tolerance."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_rate_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32
ROWS, ROW_PAIRS = 5, 2 * 4800


def _ns(nt):
    return (1, nt - 2, nt - 1, nt, 63, 64, 65, 1023, 1024, 1025, 4800)


@pytest.fixture(scope="module")
def rows():
    """five rows of full-range pairs, shared and never changed: stream s reads row s % 5 at step STEPS[s % 7]"""
    x = ref.random_full_range(np.random.default_rng(31), (ROWS, 2 * ROW_PAIRS))
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def tables(pkg):
    out = {}
    for nt in (4, 32, 64):
        for logph in (4, 8):
            out[nt, logph] = pkg.rate_coef(nt, logph, 0.9) if nt >= 32 else ref.small_table(nt, logph)
    return out


_want = {}


def _ref_calls(rows, coef, key, row, step, cuts):
    """the reference's outputs and pos after every call of the row cut into `cuts`, computed once per (table, row, step, cuts)"""
    k = (key, row, step, tuple(cuts))
    if k not in _want:
        _want[k] = ref.run(rows[row], coef, step, cuts)[:2]
    return _want[k]


def _steps(ns):
    return [ref.STEPS[s % len(ref.STEPS)] for s in range(ns)]


def _input(rows, ns, a, b):
    return np.stack([rows[s % ROWS, 2 * a:2 * b] for s in range(ns)])


@pytest.mark.parametrize("ns", [1, 3, 65])
@pytest.mark.parametrize("nt,logph", [(4, 4), (4, 8), (32, 4), (32, 8), (64, 4), (64, 8)])
def test_every_shape_against_the_reference(pkg, rows, tables, ns, nt, logph):
    """two calls of n pairs from reset, per-stream steps mixed in the batch: outputs, counts and pos after either call"""
    coef = tables[nt, logph]
    steps = _steps(ns)
    with pkg.PcmRateMatcher(ns, coef) as rm:
        assert rm.kernel_name == "pcm-rate"
        rm.set_step(steps)
        assert [int(v) for v in rm.steps] == steps
        for n in _ns(nt):
            rm.reset()
            for c in range(2):
                cnt, mx = rm.count(n)
                got = rm.process_batch(_input(rows, ns, c * n, (c + 1) * n))
                _, pos = rm.state()
                for s in range(ns):
                    outs, poss = _ref_calls(rows, coef, (nt, logph), s % ROWS, steps[s], (n, n))
                    assert int(cnt[s]) == outs[c].size // 2 == got[s].size // 2 and mx >= int(cnt[s]), (n, c, s)
                    assert np.array_equal(got[s], outs[c]), (n, c, s, steps[s])
                    assert int(pos[s]) == poss[c], (n, c, s)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_a_stream_spreads_over_workgroups(pkg, rows, tables, tmp_path):
    """n = 4800 at step 2^30 is 19200 outputs: rate_span cuts them into at least three workgroups, beside a stream at 2^34 that fits one"""
    exe = str(tmp_path / "pcm_rate_spans")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests/native/pcm_rate_spans.cpp")], check=True, cwd=ROOT, capture_output=True, text=True)
    for (nt, logph) in ((32, 8), (64, 8)):
        span, busy, cnt = (int(v) for v in subprocess.run([exe, "0", str(1 << 30), "4800", str(nt), str(logph), str(1 << 34)], capture_output=True, text=True,
                                                          check=True).stdout.split())
        assert cnt == 19200 and busy >= 3 and busy == -(-cnt // span), (span, busy, cnt)
        coef = tables[nt, logph]
        with pkg.PcmRateMatcher(2, coef) as rm:
            rm.set_step([1 << 30, 1 << 34])
            got = rm.process_batch(_input(rows, 2, 0, 4800))
            for s, step in enumerate((1 << 30, 1 << 34)):
                want = _ref_calls(rows, coef, (nt, logph), s, step, (4800,))[0][0]
                assert np.array_equal(got[s], want), (nt, s)
            assert got[0].size == 2 * 19200 and got[1].size == 2 * 1200


CUTS = (1, 0, 2, 30, 31, 32, 257, 64, 4799)


def test_ragged_calls_equal_one_call_and_the_c_routine(pkg, rows, tables):
    coef = tables[32, 8]
    ns, total = 7, sum(CUTS)
    steps = _steps(ns)
    with pkg.PcmRateMatcher(ns, coef) as rm, pkg.PcmRateMatcher(ns, coef) as whole:
        rm.set_step(steps)
        whole.set_step(steps)
        one = whole.process_batch(_input(rows, ns, 0, total))
        pieces, at = [[] for _ in range(ns)], 0
        host = [(0, None) for _ in range(ns)]
        for k, c in enumerate(CUTS):
            x = _input(rows, ns, at, at + c)
            got = rm.process_batch(x)
            _, pos = rm.state()
            for s in range(ns):
                outs, poss = _ref_calls(rows, coef, (32, 8), s % ROWS, steps[s], CUTS)
                o, p, h = pkg.pcm_rate_host(x[s], coef, steps[s], *host[s])
                host[s] = (p, h)
                assert np.array_equal(got[s], outs[k]) and np.array_equal(got[s], o), (k, s)
                assert int(pos[s]) == poss[k] == p, (k, s)
                pieces[s].append(got[s])
            at += c
        _, pos_whole = whole.state()
        for s in range(ns):
            assert np.array_equal(np.concatenate(pieces[s]), one[s]) and int(pos_whole[s]) == host[s][0], s


def test_set_step_takes_effect_at_the_next_call(pkg, rows, tables):
    coef = tables[32, 8]
    a, b = [ONE, ref.STEPS[4], 1 << 30], [ONE + 429497, 1 << 34, ref.STEPS[4]]
    with pkg.PcmRateMatcher(3, coef) as rm:
        rm.set_step(a)
        got_a = rm.process_batch(_input(rows, 3, 0, 1000))
        rm.set_step(b)
        assert [int(v) for v in rm.count(700)[0]] == [ref.count(ref.process(rows[s, :2000], coef, a[s])[1], b[s], 700) for s in range(3)]
        got_b = rm.process_batch(_input(rows, 3, 1000, 1700))
        _, pos = rm.state()
        for s in range(3):
            o1, p1, h1 = ref.process(rows[s, :2000], coef, a[s])
            o2, p2, _ = ref.process(rows[s, 2000:3400], coef, b[s], p1, h1)
            assert np.array_equal(got_a[s], o1) and np.array_equal(got_b[s], o2) and int(pos[s]) == p2, s


def test_a_call_that_yields_nothing(pkg, rows, tables):
    """step 2^34 and n = 1: the first call's output leaves pos three pairs ahead, the next three calls yield nothing and only move pos and hist —
    beside a stream that goes on producing, and alone in a handle of its own (a launch whose largest count is 0)"""
    coef = tables[32, 4]
    for ns in (2, 1):
        steps = [1 << 34, ONE][:ns]
        with pkg.PcmRateMatcher(ns, coef) as rm:
            rm.set_step(steps)
            state = [(0, None) for _ in range(ns)]
            for k in range(6):
                x = _input(rows, ns, k, k + 1)
                cnt = rm.count(1)[0]
                got = rm.process_batch(x)
                _, pos = rm.state()
                for s in range(ns):
                    o, p, h = ref.process(x[s], coef, steps[s], *state[s])
                    state[s] = (p, h)
                    assert np.array_equal(got[s], o) and int(pos[s]) == p and int(cnt[s]) == o.size // 2, (ns, k, s)
                assert got[0].size == (2 if k % 4 == 0 else 0)
            got = rm.process_batch(_input(rows, ns, 6, 300))       # the history those calls left is the row's
            for s in range(ns):
                assert np.array_equal(got[s], ref.process(rows[s, 12:600], coef, steps[s], *state[s])[0]), (ns, s)


def test_device_rows_strides_padding_and_the_callers_stream(pkg, rows, tables):
    """device rows 4 bytes into their allocations, in_stride 2n + 2 and out_stride 2 max + 6: the padding and a canary row of -32768 are neither read
    (the outputs are the reference's) nor changed; the call runs on the caller's HIP stream and n_out is known at return"""
    import torch
    coef = tables[32, 8]
    ns, n = 5, 1025
    steps = _steps(ns)
    stream = torch.cuda.Stream()
    with pkg.PcmRateMatcher(ns, coef) as rm:
        rm.set_step(steps)
        rm.set_stream(stream.cuda_stream)
        for c in range(2):
            mx = rm.count(n)[1]
            si, so = 2 * n + 2, 2 * mx + 6
            flat_in = torch.full((2 + (ns + 1) * si,), -32768, dtype=torch.int16)
            d_in_host = flat_in[2:].view(ns + 1, si)
            d_in_host[:ns, :2 * n] = torch.from_numpy(_input(rows, ns, c * n, (c + 1) * n))
            flat_in = flat_in.cuda()
            flat_out = torch.full((2 + (ns + 1) * so,), -32768, dtype=torch.int16, device="cuda")
            d_in, d_out = flat_in[2:].view(ns + 1, si), flat_out[2:].view(ns + 1, so)
            assert d_in.data_ptr() % 8 == 4 and d_out.data_ptr() % 8 == 4
            torch.cuda.synchronize()
            cnt = rm.process_batch_device(d_in[:ns], d_out[:ns], n)
            stream.synchronize()
            out = flat_out.cpu().numpy()
            assert (out[:2] == -32768).all()
            out = out[2:].reshape(ns + 1, so)
            assert (out[ns] == -32768).all()                        # the canary row
            for s in range(ns):
                want = _ref_calls(rows, coef, (32, 8), s % ROWS, steps[s], (n, n))[0][c]
                assert int(cnt[s]) == want.size // 2 and np.array_equal(out[s, :want.size], want) and (out[s, want.size:] == -32768).all(), (c, s)
            assert np.array_equal(flat_in.cpu().numpy()[2:].reshape(ns + 1, si)[:ns, :2 * n], _input(rows, ns, c * n, (c + 1) * n))
        rm.synchronize()
    # one stream at stride 0
    with pkg.PcmRateMatcher(1, coef) as rm:
        rm.set_step(ref.STEPS[4])
        d_in = torch.from_numpy(rows[1, :2 * 700].copy()).cuda()
        d_out = torch.full((2 * 700,), -32768, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        n_out = C.c_uint32()
        st = pkg.load_library().sdrfm_pcm_rate_process_batch(rm._h, C.c_void_p(d_in.data_ptr()), 0, 700, C.c_void_p(d_out.data_ptr()), 0, C.byref(n_out), 1)
        assert st == 0
        rm.synchronize()
        want = ref.process(rows[1, :1400], coef, ref.STEPS[4])[0]
        got = d_out.cpu().numpy()
        assert n_out.value == want.size // 2 and np.array_equal(got[:want.size], want) and (got[want.size:] == -32768).all()


def test_host_staging_grows_and_is_reused_below_capacity(pkg, rows, tables):
    """host-buffer calls of 1000, 1025 and 3 pairs in that order on one handle of 3 streams at three steps (2^30, 2^32 and 2^32 (1 + 1e-4), so the
    counts differ from stream to stream and the first stream's are four times the input's): both sides of the staging are made, outgrown, and then used far below their
    capacity with the last call's pairs still behind the valid ones.  Every call's outputs, counts and pos are the reference's"""
    coef, steps, cuts = tables[32, 8], _steps(3), (1000, 1025, 3)
    with pkg.PcmRateMatcher(3, coef) as rm:
        rm.set_step(steps)
        a = 0
        for c, n in enumerate(cuts):
            cnt, _ = rm.count(n)
            got = rm.process_batch(_input(rows, 3, a, a + n))
            a += n
            _, pos = rm.state()
            for s in range(3):
                outs, poss = _ref_calls(rows, coef, (32, 8), s % ROWS, steps[s], cuts)
                assert int(cnt[s]) == outs[c].size // 2 == got[s].size // 2, (n, s)
                assert np.array_equal(got[s], outs[c]) and int(pos[s]) == poss[c], (n, s, steps[s])


def test_reset_and_reuse(pkg, rows, tables):
    coef = tables[64, 8]
    steps = _steps(3)
    with pkg.PcmRateMatcher(3, coef) as rm:
        rm.set_step(steps)
        first = rm.process_batch(_input(rows, 3, 0, 1023))
        rm.process_batch(_input(rows, 3, 1023, 1100))
        rm.reset()
        st, pos = rm.state()
        assert [int(v) for v in st] == steps and not pos.any()      # the steps stay
        again = rm.process_batch(_input(rows, 3, 0, 1023))
        for s in range(3):
            assert np.array_equal(first[s], again[s]) and np.array_equal(again[s], _ref_calls(rows, coef, (64, 8), s, steps[s], (1023, 1023))[0][0]), s


def test_refusals_leave_a_live_handle_as_it_was(pkg, rows, tables):
    import torch
    lib = pkg.load_library()
    coef = tables[32, 8]
    ns, n = 3, 500
    steps = _steps(ns)
    E, ECAP = pkg.lib.EINVAL, pkg.lib.ECAPACITY
    with pkg.PcmRateMatcher(ns, coef) as rm:
        rm.set_step(steps)
        first = rm.process_batch(_input(rows, ns, 0, n))
        _, pos0 = rm.state()
        mx = rm.count(n)[1]
        d_in = torch.from_numpy(_input(rows, ns, n, 2 * n)).cuda()
        d_out = torch.full((ns, 2 * mx + 2), 12345, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        pi, po = C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr())
        cnt = (C.c_uint32 * ns)(*([77] * ns))
        call = lambda i, is_, n_, o, os_, fl: lib.sdrfm_pcm_rate_process_batch(rm._h, i, is_, n_, o, os_, cnt, fl)
        assert call(pi, 2 * n, n, po, 2 * mx + 2, 3) == E                               # flags outside SDRFM_F_DEVICE_PTRS
        assert call(pi, 2 * n, n, po, 2 * mx + 2, 4) == E
        assert call(pi, 2 * n, (1 << 20) + 1, po, 2 * mx + 2, 1) == E                   # n > 2^20
        assert call(pi, 2 * n + 1, n, po, 2 * mx + 2, 1) == E                           # odd strides
        assert call(pi, 2 * n, n, po, 2 * mx + 3, 1) == E
        assert call(C.c_void_p(d_in.data_ptr() + 2), 2 * n, n, po, 2 * mx + 2, 1) == E  # device rows not 4-byte aligned
        assert call(pi, 2 * n, n, C.c_void_p(d_out.data_ptr() + 2), 2 * mx + 2, 1) == E
        assert call(None, 2 * n, n, po, 2 * mx + 2, 1) == E                             # NULL rows with n > 0
        assert call(pi, 2 * n, n, None, 2 * mx + 2, 1) == E
        assert call(pi, 2 * n - 2, n, po, 2 * mx + 2, 1) == ECAP                        # rows that do not hold the call
        assert call(pi, 2 * n, n, po, 2 * mx - 2, 1) == ECAP
        for bad in ((1 << 30) - 1, (1 << 34) + 1, 0):
            with pytest.raises(pkg.SdrfmError) as e:
                rm.set_step([ONE, bad, ONE])
            assert e.value.status == E
        assert lib.sdrfm_pcm_rate_count(rm._h, (1 << 20) + 1, None, None) == E
        assert list(cnt) == [77] * ns
        st, pos = rm.state()
        assert [int(v) for v in st] == steps and np.array_equal(pos, pos0)
        assert (d_out.cpu().numpy() == 12345).all()
        assert call(pi, 2 * n, 0, po, 2 * mx + 2, 1) == 0 and list(cnt) == [0] * ns     # n = 0: a no-op
        assert np.array_equal(rm.state()[1], pos0)
        got = rm.process_batch_device(d_in, d_out, n)
        rm.synchronize()
        out = d_out.cpu().numpy()
        for s in range(ns):
            outs, _ = _ref_calls(rows, coef, (32, 8), s, steps[s], (n, n))
            assert np.array_equal(first[s], outs[0]) and int(got[s]) == outs[1].size // 2 and np.array_equal(out[s, :outs[1].size], outs[1]), s


def test_broadcast_receiver_into_the_matcher(pkg, tables):
    """two stations through BroadcastDemod's one-call PCM form and, on the handle's stream, into the matcher: the matcher's rows equal pcm_rate_host of
    the PCM that call left, and that PCM is bit for bit a run's without the matcher"""
    import torch
    coef = tables[32, 8]
    nbytes, ns = 2 * 240000, 2
    h, g = pkg.default_config(fir_taps=64)
    sent = [pkg.rds_encode_groups(0x2200 + k, "RATE %02d" % k) for k in range(ns)]
    iq = np.stack([pkg.make_iq_rds(1, nbytes, sent[k], rds_phase=0.8 * k, first_id=720 + k)[0] for k in range(ns)])
    cfg = pkg.BroadcastConfig(fir_coeffs=pkg.lowpass_taps(64, 120e3 / 2.4e6), pilot_coeffs=pkg.stereo_pilot_taps(101, 240e3), audio_coeffs=g,
                              rds_coeffs=pkg.rds_lowpass_taps(255, 240e3), diff_gain=pkg.stereo_diff_gain(10, 2.4e6), rds_gain=pkg.rds_gain(10, 2.4e6),
                              n_streams=ns, max_bytes_per_call=nbytes)
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    steps = [ONE + 429497, ref.STEPS[4]]
    with pkg.BroadcastDemod(cfg) as bc, pkg.StereoPcmSink(ns, alpha, gain) as sink:
        plain = [bc.process_batch_pcm(sink, iq[:, c * nbytes:(c + 1) * nbytes])[2].copy() for c in range(2)]
    assert max(int(np.abs(p).max()) for p in plain) > 1000
    stream = torch.cuda.Stream()
    d_iq = torch.from_numpy(iq).cuda()
    with pkg.BroadcastDemod(cfg) as bc, pkg.StereoPcmSink(ns, alpha, gain) as sink, pkg.PcmRateMatcher(ns, coef) as rm:
        bc.set_stream(stream.cuda_stream)
        rm.set_stream(stream.cuda_stream)
        rm.set_step(steps)
        na, nr = bc.counts(nbytes)
        host = [(0, None) for _ in range(ns)]
        for c in range(2):
            d_pcm = torch.zeros((ns, 2 * na), dtype=torch.int16, device="cuda")
            d_bb = torch.zeros((ns, 2 * nr + 2), dtype=torch.float32, device="cuda")
            d_out = torch.zeros((ns, 2 * rm.count(na)[1]), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            assert bc.process_batch_pcm_device(sink, d_iq[:, c * nbytes:(c + 1) * nbytes], None, None, d_pcm, d_bb)[0] == na
            cnt = rm.process_batch_device(d_pcm, d_out, na)
            stream.synchronize()
            pcm, out = d_pcm.cpu().numpy(), d_out.cpu().numpy()
            assert np.array_equal(pcm, plain[c]), c
            for s in range(ns):
                o, p, hh = pkg.pcm_rate_host(pcm[s], coef, steps[s], *host[s])
                host[s] = (p, hh)
                assert int(cnt[s]) == o.size // 2 and np.array_equal(out[s, :o.size], o), (c, s)
        assert [int(v) for v in rm.state()[1]] == [host[s][0] for s in range(ns)]
        bc.synchronize()
