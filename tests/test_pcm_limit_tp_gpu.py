"""The look-ahead PCM limiter's true-peak form on the device, against the host routine sdrfm_pcm_tplimit_s16 (which
tests/test_limit_tp_cpu.py holds to the numpy restatement of the definition).  Every comparison is integer equality of PCM, all 4 D + NT state
words and all four record fields.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import limit_tp_ref as ref

pytestmark = pytest.mark.gpu

ROWS = 5
# per-stream (ceiling, release, gain): the corners of the ranges and two ordinary settings; stream s takes entry s % 7 and row s % 5
PARS = [(29204, 874, 4096), (1, 1, 65536), (32767, 1 << 23, 65536), (12000, 5000, 20000), (29204, 874, 0), (9000, 300, 4096), (32767, 1, 4096)]
SHAPES = [(3, 4, 12), (6, 4, 12), (8, 4, 12), (2, 8, 4), (5, 2, 64)]


@pytest.fixture(scope="module")
def T(pkg):
    return pkg.limit.TILE


@pytest.fixture(scope="module")
def rows(T):
    """five rows of full-range pairs, shared and never changed"""
    x = ref.random_full_range(np.random.default_rng(71), (ROWS, 2 * (2 * (2 * T + 1))))
    x.setflags(write=False)
    return x


def _input(rows, ns, a, b):
    return np.stack([rows[s % ROWS, 2 * a:2 * b] for s in range(ns)])


def _table(pkg, P, NT):
    return None if (P, NT) == (4, 12) else pkg.truepeak_coef(P, NT)


class Host:
    """the host routine beside a true-peak PcmLimiter: the parameters, J, the state and the records the handle should hold"""

    def __init__(self, pkg, ns, lw, slew, coef):
        self.pkg, self.ns, self.lw, self.slew, self.coef = pkg, ns, lw, slew, coef
        self.nt = 12 if coef is None else coef.shape[1]
        self.par = np.array([ref.DEFAULT] * ns, dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
        self.J = 0
        self.reset()

    def reset(self):
        self.state, self.rec = self.pkg.limit.limit_tp_state_init(self.lw, self.nt, self.ns), self.pkg.limit.limit_identity(self.ns)

    def set_params(self, ceiling=None, release=None):
        if ceiling is not None:
            self.par["ceiling"] = ceiling
        if release is not None:
            self.par["release"] = release

    def set_gain(self, gain, jump=False):
        gain = np.broadcast_to(np.asarray(gain, np.uint32), (self.ns,))
        for s in range(self.ns):
            self.par["gain0"][s] = gain[s] if jump else ref.ramp(int(self.par["gain0"][s]), int(self.par["gain_t"][s]), self.slew, self.J)
        self.par["gain_t"] = gain
        self.J = 0

    def call(self, x):
        out, self.state, self.rec = self.pkg.pcm_limit_tp_host(x, self.lw, self.slew, self.J, self.par, self.state, self.rec, coef=self.coef)
        self.J = min(65536, self.J + x.shape[1] // 2)
        return out

    def holds(self, lim):
        par, J = lim.get_params()
        return (par.tobytes() == self.par.tobytes() and J == self.J and np.array_equal(lim.state(), self.state)
                and lim.read().tobytes() == self.rec.tobytes())


def _pair(pkg, ns, lw, slew=1, pars=True, P=4, NT=12):
    coef = _table(pkg, P, NT)
    lim, host = pkg.PcmLimiter(ns, lw, slew, detect="truepeak", coef=coef), Host(pkg, ns, lw, slew, coef)
    if pars:
        p = [PARS[s % len(PARS)] for s in range(ns)]
        for k in (lim, host):
            k.set_params([c for c, _, _ in p], [d for _, d, _ in p])
            k.set_gain([g for _, _, g in p], jump=True)
    return lim, host


@pytest.mark.parametrize("ns", [1, 3, 65])
@pytest.mark.parametrize("lw,P,NT", SHAPES)
def test_every_length_against_the_host_routine(pkg, rows, T, ns, lw, P, NT):
    """two calls of n pairs from reset, the parameters' corners mixed in the batch: PCM, state and records after either call"""
    D, H = (1 << lw) - 1, NT // 2
    lim, host = _pair(pkg, ns, lw, P=P, NT=NT)
    with lim:
        assert lim.kernel_name == "pcm-limit-tp" and lim.latency == D + H and lim.state_words == 4 * D + NT and lim.detector == (P, NT)
        for n in (1, H, D + H - 1, D + H, D + H + 1, T - 1, T, T + 1, 2 * T + 1):
            lim.reset()
            host.reset()
            for c in range(2):
                x = _input(rows, ns, c * n, (c + 1) * n)
                got, want = lim.process_batch(x), host.call(x)
                assert np.array_equal(got, want), (n, c, [s for s in range(ns) if not np.array_equal(got[s], want[s])][:5])
                assert host.holds(lim), (n, c)
                assert (np.abs(got.astype(np.int64)).max(axis=1) <= host.par["ceiling"]).all()


def test_a_peak_at_every_position(pkg, T):
    """one full-scale pair in a quiet row of T + 7 pairs, at position s in stream s, in place: every lane, window offset and tile edge sees the peak
    and the interpolator's ringing round it, and the release (9598 pairs) crosses the tile boundary"""
    import torch
    lw = 3
    L = (1 << lw) - 1 + 6
    n = T + 7
    x = np.random.default_rng(72).integers(-100, 101, size=(n, 2 * n), dtype=np.int64).astype(np.int16)
    x[np.arange(n), 2 * np.arange(n) + (np.arange(n) & 1)] = np.where(np.arange(n) & 2, 32767, -32768)
    with pkg.PcmLimiter(n, lw, detect="truepeak") as lim:
        host = Host(pkg, n, lw, 1, None)
        for k in (lim, host):
            k.set_params(8000, 874)
        d = torch.from_numpy(x).cuda()
        lim.process_batch_device(d)                                       # in place
        lim.synchronize()
        want = host.call(x)
        got = d.cpu().numpy()
        bad = [s for s in range(n) if not np.array_equal(got[s], want[s])]
        assert not bad, bad[:10]
        assert host.holds(lim)
        rec = lim.read()
        # the smallest gain is reached when the peak comes out, D + H pairs behind it; a peak in the last H pairs has not reached its detector pair
        assert (rec["at"][:n - L] == np.arange(L, n)).all() and (rec["min_gain"][:n - L] < 32768).all() and n - 8 <= int(rec["limited"][0]) <= n


def test_corners_across_three_calls_and_two_tile_borders(pkg, T):
    """delta = 1 with the release spanning three calls and more than two tiles, delta = 2^23, C = 1 and C = 32767, G in {0, 4096, 65536}, and rows on
    the rails with -32768: x' = +-2^19 on every tap"""
    lw, ns = 6, 9
    rng = np.random.default_rng(73)
    cuts = (T + 100, T, 300)
    total = sum(cuts)
    x = rng.integers(-3000, 3001, size=(ns, 2 * total), dtype=np.int64).astype(np.int16)
    x[:, 20:24] = [[32767, -32768, -32768, 32767]]                       # a full-scale burst near the start of every row
    x[6] = np.where(rng.integers(0, 2, 2 * total) > 0, 32767, -32768)    # on the rails throughout
    x[7] = -32768
    x[8] = 32767
    x[5, 1000:] = np.tile(np.array([-32768, -32768, 32767, 32767], np.int16), (2 * total - 1000) // 4)   # alternating rails, x 16: the largest |A|
    ceil = [1000, 1000, 1, 32767, 20000, 20000, 29204, 1, 32767]
    rel = [1, 1 << 23, 874, 874, 1, 1 << 23, 874, 1, 1 << 23]
    gain = [4096, 4096, 65536, 65536, 0, 65536, 4096, 65536, 4096]
    lim, host = _pair(pkg, ns, lw, pars=False)
    with lim:
        for k in (lim, host):
            k.set_params(ceil, rel)
            k.set_gain(gain, jump=True)
        at = 0
        for c in cuts:
            got, want = lim.process_batch(x[:, 2 * at:2 * (at + c)]), host.call(x[:, 2 * at:2 * (at + c)])
            assert np.array_equal(got, want) and host.holds(lim), (at, c)
            assert (np.abs(got.astype(np.int64)).max(axis=1) <= ceil).all()
            at += c
        rec = lim.read()
        assert total - 20 <= int(rec["limited"][0]) <= total and int(host.state[0, -1]) < 1 << 23   # delta = 1: still releasing at the end, two tile borders on
        assert int(rec["limited"][4]) == 0 and int(rec["min_gain"][4]) == 32768             # a gain of 0 limits nothing


def test_cuts_equal_one_call(pkg, rows, T):
    lw, ns = 6, 7
    L = (1 << lw) - 1 + 6
    cuts = (T, 1, 11, L, 7, T - 19)
    total = sum(cuts)
    whole, wh = _pair(pkg, ns, lw)
    lim, host = _pair(pkg, ns, lw)
    with whole, lim:
        x = _input(rows, ns, 0, total)
        one = whole.process_batch(x)
        assert np.array_equal(one, wh.call(x)) and wh.holds(whole)
        at, parts = 0, []
        for c in cuts:
            got = lim.process_batch(x[:, 2 * at:2 * (at + c)])
            assert np.array_equal(got, host.call(x[:, 2 * at:2 * (at + c)])) and host.holds(lim), (at, c)
            parts.append(got)
            at += c
        assert np.array_equal(np.concatenate(parts, axis=1), one)
        assert np.array_equal(lim.state(), whole.state()) and lim.read().tobytes() == whole.read().tobytes()
        assert lim.process_batch(x[:, :0]).shape == (ns, 0) and host.holds(lim)                # a call of no pairs changes nothing


def test_set_gain_and_set_params_between_calls(pkg, rows):
    lw, ns, slew = 3, 4, 2
    lim, host = _pair(pkg, ns, lw, slew, pars=False)
    with lim:
        steps = [(700, dict(gain=[4096, 9000, 0, 65536])),
                 (900, dict(gain=[4096, 1000, 65536, 0])),               # replaced while still moving
                 (1, dict(ceiling=[1, 32767, 9000, 20000])),
                 (2500, dict(release=[1 << 23, 1, 300, 5000])),
                 (3000, dict(gain=[65536, 65536, 4096, 4096], jump=True)),
                 (4000, dict(ceiling=[20000] * 4, release=[874] * 4))]
        at = 0
        for n, kw in steps:
            for k in (lim, host):
                if "gain" in kw:
                    k.set_gain(kw["gain"], jump=kw.get("jump", False))
                if "ceiling" in kw or "release" in kw:
                    k.set_params(kw.get("ceiling"), kw.get("release"))
            x = _input(rows, ns, at, at + n)
            assert np.array_equal(lim.process_batch(x), host.call(x)) and host.holds(lim), (at, n)
            at += n
        assert lim.get_params()[1] == 4000 + 3000


def test_device_rows_in_place_padding_and_host_buffers(pkg, rows, T):
    """device rows 4 bytes into their allocations with strides of 2n + 2 and 2n + 6: out of place, the padding and a canary row are neither read nor
    changed; in place, the same PCM; both on the caller's HIP stream, equal to the host-buffer call"""
    import torch
    lw, ns, n = 5, 5, T + 37
    stream = torch.cuda.Stream()
    x = _input(rows, ns, 0, 2 * n)
    a, b, ref_lim = _pair(pkg, ns, lw, P=2, NT=64)[0], _pair(pkg, ns, lw, P=2, NT=64)[0], _pair(pkg, ns, lw, P=2, NT=64)
    with a, b, ref_lim[0]:
        for k in (a, b):
            k.set_stream(stream.cuda_stream)
        for c in range(2):
            xc = x[:, 2 * c * n:2 * (c + 1) * n]
            want = ref_lim[0].process_batch(xc)                             # host buffers
            assert np.array_equal(want, ref_lim[1].call(xc))
            si, so = 2 * n + 2, 2 * n + 6
            flat_in = torch.full((2 + (ns + 1) * si,), 12345, dtype=torch.int16, device="cuda")
            flat_out = torch.full((2 + (ns + 1) * so,), -32768, dtype=torch.int16, device="cuda")
            d_in, d_out = flat_in[2:].view(ns + 1, si), flat_out[2:].view(ns + 1, so)
            d_in[:ns, :2 * n] = torch.from_numpy(np.ascontiguousarray(xc)).cuda()
            keep = flat_in.clone()
            torch.cuda.synchronize()
            a.process_batch_device(d_in[:ns], d_out[:ns], n)                # out of place
            a.synchronize()
            out = flat_out.cpu().numpy()
            assert (out[:2] == -32768).all() and torch.equal(flat_in, keep)
            out = out[2:].reshape(ns + 1, so)
            assert (out[ns] == -32768).all() and (out[:ns, 2 * n:] == -32768).all() and np.array_equal(out[:ns, :2 * n], want), c
            b.process_batch_device(d_in[:ns], None, n)                      # in place
            b.synchronize()
            inp = flat_in.cpu().numpy()
            assert (inp[:2] == 12345).all()
            inp = inp[2:].reshape(ns + 1, si)
            assert (inp[ns] == 12345).all() and (inp[:ns, 2 * n:] == 12345).all() and np.array_equal(inp[:ns, :2 * n], want), c
            assert np.array_equal(a.state(), b.state()) and ref_lim[1].holds(a) and ref_lim[1].holds(b)


def test_read_with_and_without_reset_and_reset(pkg, rows, T):
    import torch
    lw, ns, n = 6, 3, 1500
    lim, host = _pair(pkg, ns, lw)
    with lim:
        x = _input(rows, ns, 0, 3 * n)
        assert lim.read().tobytes() == pkg.limit.limit_identity(ns).tobytes()
        assert lim.state().shape == (ns, 4 * 63 + 12)
        lim.process_batch(x[:, :2 * n])
        host.call(x[:, :2 * n])
        first = lim.read()
        assert first.tobytes() == host.rec.tobytes() and lim.read().tobytes() == first.tobytes()      # a plain read changes nothing
        assert lim.read(reset=True).tobytes() == first.tobytes()
        assert lim.read().tobytes() == pkg.limit.limit_identity(ns).tobytes()                          # the records are the identity again ...
        assert np.array_equal(lim.state(), host.state)                                                 # ... and the state is kept
        got = lim.process_batch(x[:, 2 * n:4 * n])
        assert np.array_equal(got, host.call(x[:, 2 * n:4 * n]))
        d = torch.zeros(4 * ns, dtype=torch.int64, device="cuda")
        lim.read_device(d, reset=True)                                                                 # enqueued on the handle's stream
        lim.synchronize()
        second = d.cpu().numpy().view(pkg.LIMIT_DTYPE)
        assert pkg.limit_add(first.copy(), second).tobytes() == host.rec.tobytes()                     # the reads' records join to the stream's
        assert lim.read().tobytes() == pkg.limit.limit_identity(ns).tobytes()
        lim.reset()
        par, J = lim.get_params()
        assert par.tobytes() == host.par.tobytes() and J == host.J                                     # reset keeps the parameters and J
        assert np.array_equal(lim.state(), pkg.limit.limit_tp_state_init(lw, 12, ns))
        host.reset()
        assert np.array_equal(lim.process_batch(x[:, :2 * n]), host.call(x[:, :2 * n])) and host.holds(lim)


def test_every_refusal_of_create(pkg):
    """the config's refusals are the sample form's, flags != 0 included; then the table's and the window's — and a handle that was made goes on"""
    lib = pkg.load_library()
    good = dict(n_streams=1, log2_window=6, gain_slew=1, flags=0, device=0)
    tab = np.ascontiguousarray(pkg.truepeak_coef(2, 64))
    over = np.ascontiguousarray(pkg.truepeak_default_coef()).copy()
    over[0, :3] = [32767, 32767, 2]
    E = pkg.lib.EINVAL

    def create(cfg_kw, coef, P, NT, out=True):
        cfg = pkg.lib.PcmLimitConfig(**dict(good, **cfg_kw))
        h = C.c_void_p(1)
        rc = lib.sdrfm_pcm_tplimit_create(C.byref(cfg), None if coef is None else coef.ctypes.data, P, NT, C.byref(h) if out else None)
        return rc, h.value

    for kw in (dict(n_streams=0), dict(flags=1), dict(log2_window=1), dict(log2_window=9), dict(gain_slew=0), dict(gain_slew=32769)):
        assert create(kw, None, 0, 0) == (E, None), kw
    assert create({}, None, 0, 0, out=False)[0] == E
    h = C.c_void_p(1)
    assert lib.sdrfm_pcm_tplimit_create(None, None, 0, 0, C.byref(h)) == E and not h.value
    for coef, P, NT in ((tab, 3, 64), (tab, 2, 62), (tab, 2, 68), (tab, 2, 0), (over, 4, 12)):
        assert create({}, coef, P, NT) == (E, None), (P, NT)
    assert create(dict(log2_window=4), tab, 2, 64) == (E, None)                                        # 2^4 < 32
    assert create(dict(log2_window=2), None, 0, 0) == (E, None)                                        # 2^2 < 6 with the default table
    assert create(dict(device=99), None, 0, 0) == (pkg.lib.NO_DEVICE, None)
    rc, hv = create(dict(log2_window=5), tab, 2, 64)                                                   # 2^5 == 32: taken
    assert rc == 0 and hv
    P, NT, lat = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.sdrfm_pcm_tplimit_get_detector(C.c_void_p(hv), C.byref(P), C.byref(NT), C.byref(lat)) == 0 and (P.value, NT.value, lat.value) == (2, 64, 63)
    assert lib.sdrfm_pcm_tplimit_get_detector(C.c_void_p(hv), None, None, None) == 0 and lib.sdrfm_pcm_tplimit_get_detector(None, None, None, None) == E
    assert lib.sdrfm_pcm_limit_kernel_name(C.c_void_p(hv)) == b"pcm-limit-tp"
    lib.sdrfm_pcm_limit_destroy(C.c_void_p(hv))
    with pytest.raises(ValueError):
        pkg.PcmLimiter(1, 6, detect="peak")
    with pytest.raises(ValueError):
        pkg.PcmLimiter(1, 6, coef=tab)
    with pytest.raises(pkg.SdrfmError) as e:
        pkg.PcmLimiter(1, 4, detect="truepeak", coef=tab)
    assert e.value.status == E


def test_process_refusals_leave_a_true_peak_handle_as_it_was(pkg, rows):
    lib = pkg.load_library()
    lw, ns, n = 6, 2, 400
    lim, host = _pair(pkg, ns, lw)
    with lim:
        x = _input(rows, ns, 0, n)
        lim.process_batch(x)
        host.call(x)
        h = lim._h
        y = np.full((ns, 2 * n), 77, np.int16)
        E, CAP = pkg.lib.EINVAL, pkg.lib.ECAPACITY
        calls = [((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n, 2), E), ((h, x.ctypes.data, 2 * n, (1 << 20) + 1, y.ctypes.data, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n + 1, n, y.ctypes.data, 2 * n, 0), E), ((h, None, 2 * n, n, y.ctypes.data, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n - 2, n, y.ctypes.data, 2 * n, 0), CAP)]
        for args, want in calls:
            assert lib.sdrfm_pcm_limit_process_batch(*args) == want, args[1:]
        assert lib.sdrfm_pcm_limit_set_params(h, np.array([1, 32768], np.uint32).ctypes.data, None) == E
        assert lib.sdrfm_pcm_limit_set_gain(h, np.array([0, 65537], np.uint32).ctypes.data, 0) == E and lib.sdrfm_pcm_limit_get_state(h, None) == E
        assert (y == 77).all() and host.holds(lim)
        x2 = _input(rows, ns, n, 2 * n)
        assert np.array_equal(lim.process_batch(x2), host.call(x2)) and host.holds(lim)        # and the stream goes on


def test_a_sample_handle_beside_it_is_what_it_was(pkg, rows):
    """a handle made by sdrfm_pcm_limit_create in the same process, between two true-peak calls: "pcm-limit", latency D, 4 D words, the sample host
    routine's bits"""
    lw, ns, n = 6, 3, 3000
    D = (1 << lw) - 1
    tp, tph = _pair(pkg, ns, lw)
    with tp, pkg.PcmLimiter(ns, lw) as smp:
        x = _input(rows, ns, 0, 2 * n)
        assert np.array_equal(tp.process_batch(x[:, :2 * n]), tph.call(x[:, :2 * n]))
        assert smp.kernel_name == "pcm-limit" and smp.latency == D and smp.state_words == 4 * D and smp.detector == (0, 0) and smp.detect == "sample"
        par = [(PARS[s][0], PARS[s][1], PARS[s][2], PARS[s][2]) for s in range(ns)]
        smp.set_params([p[0] for p in par], [p[1] for p in par])
        smp.set_gain([p[2] for p in par], jump=True)
        got = smp.process_batch(x[:, :2 * n])
        want, st, rec = pkg.pcm_limit_host(x[:, :2 * n], lw, 1, 0, np.array(par, dtype=pkg.limit.LIMIT_PARAMS_DTYPE))
        assert np.array_equal(got, want) and np.array_equal(smp.state(), st) and smp.state().shape == (ns, 4 * D) and smp.read().tobytes() == rec.tobytes()
        assert np.array_equal(tp.process_batch(x[:, 2 * n:]), tph.call(x[:, 2 * n:])) and tph.holds(tp)
        assert not np.array_equal(got, tph.pkg.pcm_limit_tp_host(x[:, :2 * n], lw, 1, 0, np.array(par, dtype=pkg.limit.LIMIT_PARAMS_DTYPE))[0])


def test_behind_the_stereo_sink_on_its_stream_and_metered(pkg):
    """a StereoPcmSink's rows, on the sink's stream, through the true-peak limiter: the host routine on the PCM the sink returned, under +12 dB and
    a ceiling of -2 dBTP; then metered by pcm_truepeak_host — the reading is the reading of the host routine's output"""
    import torch
    ns, n, lw = 3, 4800, 6
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    rng = np.random.default_rng(74)
    t = np.arange(2 * n) / 48000.0
    left = np.stack([(0.3 + 0.2 * s) * np.sin(2 * np.pi * (400.0 + 300 * s) * t) for s in range(ns)]).astype(np.float32)
    right = (left[::-1] * 0.7 + 0.02 * rng.standard_normal(left.shape)).astype(np.float32)
    stream = torch.cuda.Stream()
    C2, boost = pkg.limit_ceiling(-2.0), int(pkg.normalise_gain_q12(-35.0)[0])
    with pkg.StereoPcmSink(ns, alpha, gain) as sink, pkg.PcmLimiter(ns, lw, 4, detect="truepeak") as lim:
        host = Host(pkg, ns, lw, 4, None)
        sink.set_stream(stream.cuda_stream)
        lim.set_stream(stream.cuda_stream)
        for k in (lim, host):
            k.set_params(C2, pkg.limit_release(0.2))
            k.set_gain(boost)
        d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        torch.cuda.synchronize()
        outs, wants = [], []
        for c in range(2):
            pcm, lim_out = (torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            sink.process_batch_device(d_l[:, c * n:(c + 1) * n], d_r[:, c * n:(c + 1) * n], pcm)
            lim.process_batch_device(pcm, lim_out)                          # no synchronisation in between: the stream orders them
            lim.synchronize()
            outs.append(lim_out.cpu().numpy())
            wants.append(host.call(pcm.cpu().numpy()))
            assert np.array_equal(outs[-1], wants[-1]) and host.holds(lim), c
        assert (lim.read()["limited"] > 0).all()
        got_rec, want_rec = pkg.pcm_truepeak_host(np.concatenate(outs, axis=1))[0], pkg.pcm_truepeak_host(np.concatenate(wants, axis=1))[0]
        assert got_rec.tobytes() == want_rec.tobytes() and int(got_rec["n"][0]) == 2 * n
