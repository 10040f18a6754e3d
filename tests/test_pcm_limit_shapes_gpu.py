"""Both look-ahead PCM limiter kernels (k_pcm_limit; k_pcm_limit_tp, §4.25) at every shape and call form they take, with the
cases of tests/limit_cases.py: every log2_window and every (log2_window, n_phases, n_taps) under skewed tables, the numpy definition directly,
gain ramps in flight across tile borders and across J's saturation with sound in the rows, the largest 64-bit sums a table allows, the largest
call, device calls enqueued back to back, and one stream under any stride.  Every comparison is integer equality of PCM, every state word, the
four record fields, the parameters and J; tests/test_limit_cases_cpu.py holds the host routine to the definition at the same cases."""
import ctypes as C

import numpy as np
import pytest

import limit_cases as cases
import limit_ref as ref
import limit_tp_ref as tpref

pytestmark = pytest.mark.gpu

ROWS, ROW_PAIRS = 5, 70400
FORMS = [("sample", 6, 0, 0, None), ("truepeak", 5, 4, 20, "skew")]      # the forms the call-form tests run: (form, lw, P, NT, table)


@pytest.fixture(scope="module")
def T(pkg):
    assert pkg.limit.TILE == cases.TILE and pkg.limit.N_MAX == 1 << 20
    return cases.TILE


@pytest.fixture(scope="module")
def rows():
    """five rows of full-range pairs, shared and never changed"""
    x = cases.random_full_range(np.random.default_rng(92), (ROWS, 2 * ROW_PAIRS))
    x.setflags(write=False)
    return x


def _input(rows, ns, a, b):
    assert b <= ROW_PAIRS
    return np.stack([rows[s % ROWS, 2 * a:2 * b] for s in range(ns)])


def _coef(form, P, NT, table):
    return cases.table_for(table, P, NT)[0] if form == "truepeak" else None


def _step(lim, host, x, tag):
    """one host-buffer call on the device and through the host routine: PCM, state, records, parameters, J and the ceiling"""
    got, want = lim.process_batch(x), host.call(x)
    assert np.array_equal(got, want), (tag, [s for s in range(x.shape[0]) if not np.array_equal(got[s], want[s])][:5])
    assert host.holds(lim), tag
    assert cases.under_ceiling(got, host), tag
    return got


def _every_length_then_the_cuts(pkg, rows, T, lw, P=0, NT=0, coef=None):
    ns, L = 3, cases.latency(lw, NT)
    lim, host = cases.pair(pkg, ns, lw, NT=NT, coef=coef)                  # one handle per shape: making one is what these tests' time goes into
    with lim:
        assert lim.kernel_name == ("pcm-limit-tp" if NT else "pcm-limit") and lim.latency == L
        assert lim.state_words == 4 * ((1 << lw) - 1) + NT and lim.detector == (P, NT)
        for n in reversed(cases.lengths(L, T)):                                    # the longest first: the handle's staging is made once
            lim.reset()
            host.reset()
            for c in range(2):
                _step(lim, host, _input(rows, ns, c * n, (c + 1) * n), (lw, P, NT, n, c))
        lim.reset()
        host.reset()
        x = _input(rows, ns, 0, sum(cases.CUTS))
        one = _step(lim, host, x, (lw, P, NT, "one call"))
        state, rec = lim.state(), lim.read()
        lim.reset()
        host.reset()
        at, parts = 0, []
        for c in cases.CUTS:
            parts.append(_step(lim, host, x[:, 2 * at:2 * (at + c)], (lw, P, NT, "cut", at, c)))
            at += c
        assert np.array_equal(np.concatenate(parts, axis=1), one), (lw, P, NT)
        assert np.array_equal(lim.state(), state) and lim.read().tobytes() == rec.tobytes(), (lw, P, NT)


# ---- a. every shape ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw", cases.sample_shapes())
def test_sample_form_at_every_window(pkg, rows, T, lw):
    """three streams from reset, two calls each of 1, D - 1, D, D + 1 and TILE + 1 pairs, then the ragged cuts against one call"""
    _every_length_then_the_cuts(pkg, rows, T, lw)


@pytest.mark.parametrize("NT", cases.TAPS)
def test_true_peak_form_at_every_window_and_phase_count(pkg, rows, T, NT):
    """every accepted (lw, P, NT) of this tap count under a skewed table of its own, every third triple of the whole list at the bound of
    sdrfm_truepeak_check_coef: LX, the window's first entry, the state offsets 2 LX + t, the table's row length and the instance of P"""
    shapes = cases.tp_shapes()
    mine = [(i, s) for i, s in enumerate(shapes) if s[2] == NT]
    assert len(mine) == 3 * sum(1 for lw in range(2, 9) if (1 << lw) >= NT // 2)
    for i, (lw, P, nt) in mine:
        coef = cases.skew_table(P, nt, 100 + lw, at_bound=i % 3 == 0)
        assert cases.table_is_skewed(coef)
        _every_length_then_the_cuts(pkg, rows, T, lw, P, nt, coef)


# ---- b. against the definition directly -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,lw,P,NT,table", cases.DEFINITION_CASES)
def test_against_the_numpy_definition(pkg, T, form, lw, P, NT, table):
    """the five corners as five streams, one call of TILE + L + 2 pairs with a rail burst straddling pair TILE, then 1500 from the carried state:
    limit_ref.process / limit_tp_ref.process, the records joined with ref.join — and the host routine beside it"""
    case = cases.definition_case(form, lw, P, NT, table, T)
    lim, host = cases.pair(pkg, len(cases.CORNERS), lw, NT=NT, coef=case["coef"])
    with lim:
        par = lim.get_params()[0]
        assert [tuple(int(v) for v in p) for p in par] == case["par"]
        at = 0
        for k, n in enumerate(case["cuts"]):
            x = case["x"][:, 2 * at:2 * (at + n)]
            got = _step(lim, host, x, (form, lw, P, NT, k))
            assert np.array_equal(got, case["out"][k]), (k, [s for s in range(5) if not np.array_equal(got[s], case["out"][k][s])])
            assert np.array_equal(lim.state(), case["state"][k]) and [ref.rec_tuple(r) for r in lim.read()] == case["rec"][k], k
            at += n
        if table == "bound":
            assert case["peak"] >= 0.999 * cases.SUM_MAX


# ---- c. ramps across tiles and across J's saturation, with sound in the rows ------------------------------------------------------------------------------
def _ramp_pair(pkg, form, lw, P, NT, table, slew):
    return cases.pair(pkg, 5, lw, slew, NT=NT, coef=_coef(form, P, NT, table))


def _ramp_step(lim, host, x, tag, moving):
    """a call during a ramp: the host routine's, and NOT what a ramp frozen at the call's first value gives on the streams named"""
    frozen = host.frozen(x)
    got = _step(lim, host, x, tag)
    for s in moving:
        assert not np.array_equal(got[s], frozen[s]), (tag, s)
    return got


@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_a_ramp_that_ends_where_j_saturates_across_thirteen_tile_borders(pkg, rows, T, form, lw, P, NT, table):
    """slew 1, gain 0 -> 65536 in one call of 70000 pairs: the ramp takes 65536 pairs, the kernel evaluates it at J + base + j + 1 in every tile"""
    lim, host = _ramp_pair(pkg, form, lw, P, NT, table, 1)
    with lim:
        for k in (lim, host):
            k.set_gain(0, jump=True)
            k.set_gain(65536)
        assert 70000 // T == 13
        _ramp_step(lim, host, _input(rows, 5, 0, 70000), (form, "70000"), (0, 2, 3))
        assert lim.get_params()[1] == 65536 and host.now() == [65536] * 5
        _step(lim, host, _input(rows, 5, 70000, 70300), (form, "behind the ramp"))


@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_a_ramp_across_calls_with_its_target_replaced(pkg, rows, T, form, lw, P, NT, table):
    """slew 3, 4096 -> 40000 (11968 pairs) in calls of TILE + 100, TILE and 300; after the first call every target is replaced without a jump, so
    the ramps restart from where they have got to (19756): up, down, to 0 and on"""
    lim, host = _ramp_pair(pkg, form, lw, P, NT, table, 3)
    with lim:
        for k in (lim, host):
            k.set_gain(4096, jump=True)
            k.set_gain(40000)
        _ramp_step(lim, host, _input(rows, 5, 0, T + 100), (form, 0), (0, 2, 3))
        assert host.now() == [4096 + 3 * (T + 100)] * 5
        for k in (lim, host):
            k.set_gain([65536, 9000, 65536, 0, 30000])
        assert [int(g) for g in host.par["gain0"]] == [19756] * 5 and lim.get_params()[1] == 0
        _ramp_step(lim, host, _input(rows, 5, T + 100, 2 * T + 100), (form, 1), (0, 2, 3))
        _ramp_step(lim, host, _input(rows, 5, 2 * T + 100, 2 * T + 400), (form, 2), (0, 2))     # 19756 -> 65536 takes 15260 pairs: still moving


@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_j_passes_65536_inside_a_call(pkg, rows, T, form, lw, P, NT, table):
    """slew 1, 65536 -> 0: a call of 60000 pairs and one of 10000, J saturating 5536 pairs into the second, where the ramp ends"""
    lim, host = _ramp_pair(pkg, form, lw, P, NT, table, 1)
    with lim:
        for k in (lim, host):
            k.set_gain(65536, jump=True)
            k.set_gain(0)
        _ramp_step(lim, host, _input(rows, 5, 0, 60000), (form, 0), (0, 2, 3))
        assert lim.get_params()[1] == 60000 and host.now() == [5536] * 5
        got = _ramp_step(lim, host, _input(rows, 5, 60000, 70000), (form, 1), (0, 2, 3))
        assert lim.get_params()[1] == 65536 and host.now() == [0] * 5
        assert not got[:, -2 * 4000:].any() and got[0, :2 * 4000].any()                          # the gain has reached 0 and stays there


@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_a_ramp_of_its_own_per_stream(pkg, rows, T, form, lw, P, NT, table):
    """slew 2, five streams from and to different gains in one batch, one of them down to 0 (32768 pairs) over three tiles and two calls"""
    lim, host = _ramp_pair(pkg, form, lw, P, NT, table, 2)
    with lim:
        for k in (lim, host):
            k.set_gain([4096, 65536, 0, 20000, 30000], jump=True)
            k.set_gain([65536, 0, 30000, 20000, 0])
        frozen = host.frozen(_input(rows, 5, 0, 2 * T + 1))
        got = _step(lim, host, _input(rows, 5, 0, 2 * T + 1), (form, 0))
        # stream 3 does not move; stream 1's ceiling of 1 hides its ramp from the PCM (not from the state's x' words)
        assert [not np.array_equal(got[s], frozen[s]) for s in (0, 2, 3, 4)] == [True, True, False, True]
        _step(lim, host, _input(rows, 5, 2 * T + 1, 3 * T + 8), (form, 1))
        assert host.now() == [4096 + 2 * (3 * T + 8), 65536 - 2 * (3 * T + 8), 30000, 20000, 0]


# ---- d. the largest sums on the device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NT", [4, 12, 64])
@pytest.mark.parametrize("P", cases.PHASES)
def test_the_largest_sums_a_table_allows(pkg, T, P, NT):
    """a table AT the bound, rail bursts repeated over a tile plus L under a gain of 65536, ceilings 1, 12000 and 32767: |A| comes within a
    thousandth of 2 x 65535 x 2^19 (the definition's own T says so), and the 64-bit sums are the host routine's and the definition's"""
    lw = {4: 2, 12: 6, 64: 8}[NT]
    L, ns = cases.latency(lw, NT), 3
    coef = cases.skew_table(P, NT, 7, True)
    n = T + L
    tiled = np.tile(cases.rail_burst(coef), n // NT + 2)
    x = np.stack([tiled[2 * s:2 * (s + n)] for s in range(ns)])                                   # stream s starts s pairs into the burst
    lim, host = cases.pair(pkg, ns, lw, NT=NT, coef=coef, pars=False)
    with lim:
        for k in (lim, host):
            k.set_params([1, 12000, 32767], [874, 1, 1 << 23])
            k.set_gain(65536, jump=True)
        got = _step(lim, host, x, (P, NT))
        for s in range(ns):
            y, _, _, _, peak = tpref.process(x[s, :2 * 2000], lw, 1, 0, tuple(int(v) for v in host.par[s]), coef=coef)
            assert np.array_equal(got[s, :2 * 2000], y), (P, NT, s)
            assert 0.999 * cases.SUM_MAX <= int(peak.max()) <= cases.SUM_MAX, (P, NT, s, int(peak.max()))
        assert (lim.read()["limited"] >= n - L).all()


# ---- e. the largest call ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sample", "truepeak"])
def test_the_largest_call(pkg, rows, T, form):
    """2^20 pairs in one call, 205 tiles: quiet noise with full-scale pairs at 3, TILE - 1, TILE, 2^19 and 2^20 - 70 under a gain that ramps from 1
    to 16 over the first 61440 pairs, so the smallest gain falls at 2^19 — and again, equal, three tiles on, where the row repeats the 800 pairs
    round 2^19: the earliest wins, with `at` past 2^19.  The second stream releases by 1 per pair: its release is still climbing at the end, the
    carry handed over 204 times."""
    lw, n, NT = 6, 1 << 20, 12 if form == "truepeak" else 0
    L, K = cases.latency(lw, NT), 400
    p, q = 1 << 19, (1 << 19) + 3 * T + 17
    assert pkg.limit.N_MAX == n and (n + T - 1) // T == 205 and p // T != q // T and q + K < n - 70 - K
    row = np.random.default_rng(93).integers(-100, 101, size=2 * n, dtype=np.int64).astype(np.int16)
    for i in (3, T - 1, T, n - 70):
        row[2 * i] = 32767
    row[2 * p:2 * p + 4] = [-32768, 32767, -32768, 32767]                                        # two pairs: between them the waveform passes the samples
    row[2 * (q - K):2 * (q + K)] = row[2 * (p - K):2 * (p + K)]
    x = np.stack([row, row])
    lim, host = cases.pair(pkg, 2, lw, 1, NT=NT, pars=False)
    with lim:
        for k in (lim, host):
            k.set_params([29204, 29204], [874, 1])
            k.set_gain(4096, jump=True)
            k.set_gain(65536)
        got = _step(lim, host, x, form)
        rec = lim.read()
        # stream 0 is released again long before 2^19: what comes out round p comes out again round q, so the smallest gain is reached twice
        assert np.array_equal(got[0, 2 * (p + L - 100):2 * (p + L + 100)], got[0, 2 * (q + L - 100):2 * (q + L + 100)])
        assert p <= int(rec["at"][0]) <= p + L + 1 and int(rec["min_gain"][0]) < 2000 and int(rec["limited"][0]) > 2 * 9000    # two releases from 1825: 9063 pairs each
        assert int(rec["at"][1]) >= p and int(rec["limited"][1]) >= n - 100 and int(host.state[1, -1]) < 1 << 23
        assert lim.get_params()[1] == 65536
        _step(lim, host, _input(rows, 2, 0, 100), (form, "100 more"))


# ---- f. device calls back to back -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regain", [False, True])
@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_device_calls_back_to_back(pkg, rows, T, form, lw, P, NT, table, regain):
    """eight in-place device calls of ragged lengths enqueued on the caller's stream with nothing between them but one read_device(reset=True)
    behind the fourth — launch c + 1 reads the state launch c writes, and J goes by value — then one synchronise.  With regain, a set_gain
    (which synchronises) behind the third call."""
    import torch
    ns, L = 3, cases.latency(lw, NT)
    cuts = (T + 3, 1, 17, L, 2 * T + 1, 5, T, 200)
    lim, host = cases.pair(pkg, ns, lw, 2, NT=NT, coef=_coef(form, P, NT, table))
    stream = torch.cuda.Stream()
    with lim:
        lim.set_stream(stream.cuda_stream)
        for k in (lim, host):
            k.set_gain(30000)                                                                    # 12952 pairs at slew 2: the ramp spans the first five calls
        at, xs = 0, []
        for c in cuts:
            xs.append(_input(rows, ns, at, at + c))
            at += c
        bufs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]
        d_rec = torch.zeros(4 * ns, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for c, b in enumerate(bufs):
            if regain and c == 3:
                lim.set_gain([0, 65536, 4096])
            lim.process_batch_device(b)
            if c == 3:
                lim.read_device(d_rec, reset=True)
        lim.synchronize()
        want, first = [], None
        for c, x in enumerate(xs):
            if regain and c == 3:
                host.set_gain([0, 65536, 4096])
            want.append(host.call(x))
            if c == 3:
                first = host.rec.copy()
        for c, b in enumerate(bufs):
            got = b.cpu().numpy()
            assert np.array_equal(got, want[c]), (c, cuts[c])
            assert cases.under_ceiling(got, host)
        par, J = lim.get_params()
        assert par.tobytes() == host.par.tobytes() and J == host.J == (sum(cuts[3:]) if regain else sum(cuts))
        assert np.array_equal(lim.state(), host.state)
        read = d_rec.cpu().numpy().view(pkg.LIMIT_DTYPE)
        assert read.tobytes() == first.tobytes() and (lim.read()["n"] == sum(cuts[4:])).all()
        assert pkg.limit_add(read.copy(), lim.read()).tobytes() == host.rec.tobytes()             # the two records join to the stream's


# ---- g. one stream, any stride ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,lw,P,NT,table", FORMS)
def test_one_stream_under_any_stride(pkg, rows, form, lw, P, NT, table):
    """a handle of one stream ignores the strides: 0 and 2 through the C entry point, host and device buffers, give the PCM of strides of 2 n, and
    the device form writes nothing beyond 2 n int16 of its output"""
    import torch
    lib = pkg.load_library()
    n, pad = 700, 64
    x = np.ascontiguousarray(_input(rows, 1, 0, n))
    lim, host = cases.pair(pkg, 1, lw, NT=NT, coef=_coef(form, P, NT, table))
    with lim:
        want = _step(lim, host, x, "strides of 2 n")
        state, rec = lim.state(), lim.read()
        assert cases.under_ceiling(want, host)
        for k, (si, so) in enumerate(((0, 0), (2, 2), (0, 2), (2 * n, 0))):
            lim.reset()
            y = np.full(2 * n + pad, 77, np.int16)
            assert lib.sdrfm_pcm_limit_process_batch(lim._h, x.ctypes.data, si, n, y.ctypes.data, so, 0) == 0, (si, so)
            assert np.array_equal(y[:2 * n], want[0]) and (y[2 * n:] == 77).all(), (si, so)
            assert np.array_equal(lim.state(), state) and lim.read().tobytes() == rec.tobytes()
            lim.reset()
            d_in = torch.from_numpy(x[0].copy()).cuda()
            d_out = torch.full((2 * n + pad,), 77, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            assert lib.sdrfm_pcm_limit_process_batch(lim._h, C.c_void_p(d_in.data_ptr()), si, n, C.c_void_p(d_out.data_ptr()), so, pkg.lib.F_DEVICE_PTRS) == 0
            lim.synchronize()
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:2 * n], want[0]) and (out[2 * n:] == 77).all(), (si, so)
            assert np.array_equal(d_in.cpu().numpy(), x[0])
            assert np.array_equal(lim.state(), state) and lim.read().tobytes() == rec.tobytes()
            par, J = lim.get_params()
            assert par.tobytes() == host.par.tobytes() and J == (2 * k + 3) * n                   # reset keeps J, and every call moves it
