"""The PCM rate matcher on the device (csrc/sdrfm_pcm_rate.h) over the tables it accepts, where tests/test_pcm_rate_gpu.py runs
three tap counts, two phase counts and half rows of 30000: every tap count x every phase count with half rows at the bound of 65535, the
bound itself at either parity of the window index, the phase edges, calls of 2^20 pairs and of 2^20 outputs, 1025 streams.  The reference is
tests/pcm_rate_ref.py; every comparison of samples, counts and pos is integer equality, nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import pcm_rate_ref as ref

pytestmark = pytest.mark.gpu

ONE = 1 << 32
TAPS = tuple(range(4, 65, 4))
LOGPHS = (4, 5, 6, 7, 8)


def _hold(rm, x, want_outs, want_pos, tag):
    """one host-buffer call of the rows x [ns, 2n]: counts, outputs and the device's pos against the reference's, per stream"""
    cnt, mx = rm.count(x.shape[1] // 2)
    got = rm.process_batch(x)
    _, pos = rm.state()
    for s in range(x.shape[0]):
        assert int(cnt[s]) == want_outs[s].size // 2 == got[s].size // 2 and mx >= int(cnt[s]), (tag, s)
        assert np.array_equal(got[s], want_outs[s]), (tag, s, np.flatnonzero(got[s] != want_outs[s])[:8])
        assert int(pos[s]) == want_pos[s], (tag, s)
    return got


@pytest.mark.parametrize("nt", TAPS)
def test_every_table_shape(pkg, nt):
    """n_taps x log2_phases over all the library accepts — the inner loop's nt / 4 dwords leave every remainder of its unrolling by four —, tables
    with half rows at the bound of 65535, three streams at the smallest, a fractional and the largest step, calls of nt - 2 (shorter than the
    history), nt + 1 and 300 pairs from reset"""
    steps = [1 << 30, ref.STEPS[4], 1 << 34]
    cuts = (nt - 2, nt + 1, 300)
    x = ref.random_full_range(np.random.default_rng(4000 + nt), (3, 2 * sum(cuts)))
    low = high = False
    # (with two or four taps per half row small_table's clip to int16 leaves half rows short of the bound: there bound_table's tables run as well)
    tables = [(logph, ref.small_table(nt, logph, overshoot=True)) for logph in LOGPHS] + [(logph, ref.bound_table(nt, logph)) for logph in LOGPHS if nt < 12]
    for logph, coef in tables:
        halves = np.abs(coef.astype(np.int64)).reshape(-1, 2, nt // 2).sum(axis=2)
        assert halves.max() <= 65535 and (nt < 8 or np.median(halves) == 65535)
        want = [ref.run(x[s], coef, steps[s], cuts)[:2] for s in range(3)]
        with pkg.PcmRateMatcher(3, coef) as rm:
            rm.set_step(steps)
            at = 0
            for k, c in enumerate(cuts):
                _hold(rm, x[:, 2 * at:2 * (at + c)], [want[s][0][k] for s in range(3)], [want[s][1][k] for s in range(3)], (nt, logph, k))
                at += c
        low = low or any((o == -32768).any() for w in want for o in w[0])
        high = high or any((o == 32767).any() for w in want for o in w[0])
    assert low and high, nt                                         # the reference itself reaches both rails: the sums pass +-2^38
    print("n_taps %2d: %d tables x 3 streams x 3 calls equal to the reference" % (nt, len(tables)))


def _bound_tables(nt):
    """(name, table) with every half row's sum of |coef| at exactly 65535: a random one, and one whose first dword of taps is -32768 | -32767,
    which pairs of (-32768, -32768) drive to 2^31 - 32768 in a single dot product"""
    one = ref.bound_table(nt, 4)
    one[:, :nt // 2] = 0
    one[:, 0], one[:, 1] = -32768, -32767
    return [("random", ref.bound_table(nt, 4)), ("one dword", one)]


@pytest.mark.parametrize("nt", [4, 16, 64])
def test_the_half_row_bound_at_either_parity(pkg, nt):
    """step 2^32 from reset: output j reads row 0 over pairs j - nt + 1 .. j, and the kernel forms its tap pairs with a shift of 16 when j is even
    and of 0 when it is odd.  Pairs of +-32768 sign(coef[0]) in front of output 100 and of output 201 drive L's half-row sums to
    65535 * 32768 less a little and R's, with the signs opposed, to the negative of that: the int32 accumulators' whole range, with both shifts.
    Then 2000 pairs of full-range noise at every step"""
    lib = pkg.load_library()
    noise = ref.random_full_range(np.random.default_rng(4100 + nt), (len(ref.STEPS), 2 * 2000))
    for name, coef in _bound_tables(nt):
        a = np.abs(coef.astype(np.int64))
        assert (a[:, :nt // 2].sum(axis=1) == 65535).all() and (a[:, nt // 2:].sum(axis=1) == 65535).all()
        assert lib.sdrfm_pcm_rate_check_coef(coef.ctypes.data, nt, 4) == 0
        x = np.zeros((400, 2), np.int16)
        sgn = np.where(coef[0] >= 0, 1, -1)
        for j in (100, 201):
            x[j - nt + 1:j + 1, 0] = np.where(sgn > 0, 32767, -32768)
            x[j - nt + 1:j + 1, 1] = np.where(sgn > 0, -32768, 32767)
        if name == "one dword":
            x[250:] = -32768                                        # ... and a stretch in which the first dot product alone adds 2^31 - 32768
        want = ref.process(x.reshape(-1), coef, ONE)
        half = coef[0].astype(np.int64)[:nt // 2]
        for j in (100, 201):
            assert want[0][2 * j] == 32767 and want[0][2 * j + 1] == -32768, (nt, name, j)
            taps = x[j - nt + 1:j + 1].astype(np.int64)[:nt // 2]
            assert int(half @ taps[:, 0]) >= 65535 * 32768 - 65535 and int(half @ taps[:, 1]) <= -(65535 * 32768 - 65535)
        if name == "one dword":
            assert int(half @ x[399 - nt + 1:400].astype(np.int64)[:nt // 2, 0]) == (1 << 31) - 32768
        with pkg.PcmRateMatcher(1, coef) as rm:
            _hold(rm, x.reshape(1, -1), [want[0]], [want[1]], (nt, name, "driven"))
        with pkg.PcmRateMatcher(len(ref.STEPS), coef) as rm:
            rm.set_step(list(ref.STEPS))
            w = [ref.process(noise[s], coef, step) for s, step in enumerate(ref.STEPS)]
            assert any((o[0] == 32767).any() for o in w) and any((o[0] == -32768).any() for o in w), (nt, name)
            _hold(rm, noise, [o[0] for o in w], [o[1] for o in w], (nt, name, "noise"))


def test_phase_edges_on_the_device(pkg):
    """f = 0 reads row 0 alone; p = NPH - 1 with mu = 255 reads rows NPH - 1 and NPH.  A row stride off by one dword moves every row but row 0"""
    nt, logph = 8, 4
    nph = 1 << logph
    x = ref.random_full_range(np.random.default_rng(4200), 2 * 300)
    base = ref.small_table(nt, logph, overshoot=True)
    other = ref.small_table(nt, logph, np.random.default_rng(4201), overshoot=True)

    def run(coef, step, n=300):
        with pkg.PcmRateMatcher(1, coef) as rm:
            rm.set_step(step)
            want = ref.process(x[:2 * n], coef, step)
            return _hold(rm, x[None, :2 * n], [want[0]], [want[1]], step)[0]

    # step 2^32 from reset: every f is 0 — rows 1 .. NPH may hold anything
    rest = base.copy()
    rest[1:] = other[1:]
    assert not np.array_equal(rest, base)
    assert np.array_equal(run(base, ONE), run(rest, ONE))
    # step 2^34 - 1: output 1 stands at pair 3 with f = 2^32 - 1, p = NPH - 1 and mu = 255
    step = (1 << 34) - 1
    assert step >> 32 == 3 and (step & 0xFFFFFFFF) >> (32 - logph) == nph - 1 and ((step & 0xFFFFFFFF) >> (24 - logph)) & 255 == 255
    last = base.copy()
    last[nph] = other[nph]
    a, b = run(base, step, 40), run(last, step, 40)                 # each equals its own reference (run holds it)
    assert not np.array_equal(a[2:4], b[2:4]) and np.array_equal(a[:2], b[:2])
    lower = base.copy()
    lower[:nph - 1] = other[:nph - 1]
    c = run(lower, step, 40)
    assert np.array_equal(c[2:4], a[2:4]) and not np.array_equal(c, a)


LONG = [(1 << 20, 1 << 34, 1 << 18, 256), (1 << 18, 1 << 30, 1 << 20, 1024)]     # pairs, step, outputs, spans


@pytest.fixture(scope="module")
def long_case():
    """one row of 2^20 + 65 full-range pairs and the table both long shapes use; the references are computed once, here"""
    coef = ref.small_table(4, 4, overshoot=True)
    x = ref.random_full_range(np.random.default_rng(4300), 2 * ((1 << 20) + 65))
    x.setflags(write=False)
    want = {}
    for n, step, outputs, _ in LONG:
        first = ref.process_fast(x[:2 * n], coef, step)
        assert first[0].size == 2 * outputs
        want[n] = (first, ref.process(x[2 * n:2 * (n + 65)], coef, step, first[1], first[2]))
    return coef, x, want


@pytest.mark.parametrize("n,step,outputs,spans", LONG)
def test_long_calls(pkg, long_case, n, step, outputs, spans):
    """the longest call the library takes, and the most outputs one call gives: 256 and 1024 workgroups for the one stream; the call of 65 pairs
    behind it carries pos and the history"""
    coef, x, want = long_case
    first, then = want[n]
    with pkg.PcmRateMatcher(1, coef) as rm:
        rm.set_step(step)
        assert rm.count(n)[1] == outputs == spans * 1024
        _hold(rm, x[None, :2 * n], [first[0]], [first[1]], (n, "long"))
        _hold(rm, x[None, 2 * n:2 * (n + 65)], [then[0]], [then[1]], (n, "behind"))


def test_most_outputs_through_device_buffers(pkg, long_case):
    """2^20 outputs into a device row with one canary pair behind the last output and one in front of the first"""
    import torch
    coef, x, want = long_case
    n, step, outputs, _ = LONG[1]
    first, then = want[n]
    d_in = torch.from_numpy(x[:2 * (n + 65)].copy()).cuda().view(1, -1)
    d_out = torch.full((1, 2 * outputs + 4), -21846, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with pkg.PcmRateMatcher(1, coef) as rm:
        rm.set_step(step)
        cnt = rm.process_batch_device(d_in[:, :2 * n], d_out[:, 2:], n)
        rm.synchronize()
        out = d_out.cpu().numpy()[0]
        assert int(cnt[0]) == outputs and (out[:2] == -21846).all() and (out[-2:] == -21846).all()
        assert np.array_equal(out[2:-2], first[0])
        d_out.fill_(-21846)
        torch.cuda.synchronize()
        cnt = rm.process_batch_device(d_in[:, 2 * n:], d_out[:, 2:], 65)
        rm.synchronize()
        out = d_out.cpu().numpy()[0]
        assert int(cnt[0]) == then[0].size // 2 == 260 and np.array_equal(out[2:2 + 520], then[0]) and (out[522:] == -21846).all() and (out[:2] == -21846).all()
        assert int(rm.state()[1][0]) == then[1]


def test_a_wide_batch_and_the_one_stream_host_form(pkg):
    """1025 streams — a grid of 1025 rows of workgroups — of 65 pairs, steps cycling over ref.STEPS, two calls; and one stream through the C ABI
    with host buffers and both strides 0"""
    ns, n = 1025, 65
    coef = ref.small_table(4, 4, overshoot=True)
    rows = ref.random_full_range(np.random.default_rng(4400), (5, 2 * 2 * n))
    steps = [ref.STEPS[s % len(ref.STEPS)] for s in range(ns)]
    want = {(r, k): ref.run(rows[r], coef, ref.STEPS[k], (n, n))[:2] for r in range(5) for k in range(len(ref.STEPS))}
    of = lambda s: want[s % 5, s % len(ref.STEPS)]
    with pkg.PcmRateMatcher(ns, coef) as rm:
        rm.set_step(steps)
        for c in range(2):
            x = np.stack([rows[s % 5, 2 * c * n:2 * (c + 1) * n] for s in range(ns)])
            _hold(rm, x, [of(s)[0][c] for s in range(ns)], [of(s)[1][c] for s in range(ns)], ("wide", c))
    lib = pkg.load_library()
    with pkg.PcmRateMatcher(1, coef) as rm:
        rm.set_step(ref.STEPS[4])
        outs, poss = want[1, 4]
        for c in range(2):
            x = np.ascontiguousarray(rows[1, 2 * c * n:2 * (c + 1) * n])
            out = np.full(2 * rm.count(n)[1] + 2, -21846, np.int16)
            n_out = C.c_uint32()
            assert lib.sdrfm_pcm_rate_process_batch(rm._h, x.ctypes.data, 0, n, out.ctypes.data, 0, C.byref(n_out), 0) == 0
            assert n_out.value == outs[c].size // 2 and np.array_equal(out[:outs[c].size], outs[c]) and (out[outs[c].size:] == -21846).all(), c
            assert int(rm.state()[1][0]) == poss[c]
