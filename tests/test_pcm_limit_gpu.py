"""The look-ahead PCM limiter on the device, against the host routine sdrfm_pcm_limit_s16 (which tests/test_limit_cpu.py holds to
the numpy restatement of the definition).  Every comparison is integer equality of PCM, all 4 D state words and all four record fields.  Nothing
here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import limit_ref as ref

pytestmark = pytest.mark.gpu

ROWS = 5
# per-stream (ceiling, release, gain): the corners of the ranges and two ordinary settings; stream s takes entry s % 7 and row s % 5
PARS = [(29204, 874, 4096), (1, 1, 65536), (32767, 1 << 23, 65536), (12000, 5000, 20000), (29204, 874, 0), (9000, 300, 4096), (32767, 1, 4096)]


@pytest.fixture(scope="module")
def T(pkg):
    return pkg.limit.TILE


@pytest.fixture(scope="module")
def rows(T):
    """five rows of full-range pairs, shared and never changed"""
    x = ref.random_full_range(np.random.default_rng(51), (ROWS, 2 * (2 * (2 * T + 1))))
    x.setflags(write=False)
    return x


def _input(rows, ns, a, b):
    return np.stack([rows[s % ROWS, 2 * a:2 * b] for s in range(ns)])


class Host:
    """the host routine beside a PcmLimiter: the parameters, J, the state and the records the handle should hold"""

    def __init__(self, pkg, ns, lw, slew):
        self.pkg, self.ns, self.lw, self.slew = pkg, ns, lw, slew
        self.par = np.array([ref.DEFAULT] * ns, dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
        self.J = 0
        self.reset()

    def reset(self):
        self.state, self.rec = self.pkg.limit.limit_state_init(self.lw, self.ns), self.pkg.limit.limit_identity(self.ns)

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
        out, self.state, self.rec = self.pkg.pcm_limit_host(x, self.lw, self.slew, self.J, self.par, self.state, self.rec)
        self.J = min(65536, self.J + x.shape[1] // 2)
        return out

    def holds(self, lim):
        par, J = lim.get_params()
        return (par.tobytes() == self.par.tobytes() and J == self.J and np.array_equal(lim.state(), self.state)
                and lim.read().tobytes() == self.rec.tobytes())


def _pair(pkg, ns, lw, slew=1, pars=True):
    lim, host = pkg.PcmLimiter(ns, lw, slew), Host(pkg, ns, lw, slew)
    if pars:
        p = [PARS[s % len(PARS)] for s in range(ns)]
        for k in (lim, host):
            k.set_params([c for c, _, _ in p], [d for _, d, _ in p])
            k.set_gain([g for _, _, g in p], jump=True)
    return lim, host


@pytest.mark.parametrize("ns", [1, 3, 65])
@pytest.mark.parametrize("lw", [2, 6, 8])
def test_every_length_against_the_host_routine(pkg, rows, T, ns, lw):
    """two calls of n pairs from reset, the parameters' corners mixed in the batch: PCM, state and records after either call"""
    D = (1 << lw) - 1
    lim, host = _pair(pkg, ns, lw)
    with lim:
        assert lim.kernel_name == "pcm-limit" and lim.latency == D and lim.state_words == 4 * D
        for n in (1, D - 1, D, D + 1, 2 * D, 2 * D + 1, T - 1, T, T + 1, 2 * T + 1):
            lim.reset()
            host.reset()
            for c in range(2):
                x = _input(rows, ns, c * n, (c + 1) * n)
                got, want = lim.process_batch(x), host.call(x)
                assert np.array_equal(got, want), (n, c, [s for s in range(ns) if not np.array_equal(got[s], want[s])][:5])
                assert host.holds(lim), (n, c)
                assert (np.abs(got.astype(np.int64)).max(axis=1) <= host.par["ceiling"]).all()


def test_a_peak_at_every_position(pkg, T):
    """one full-scale pair in a quiet row of T + 2 D + 1 pairs, at position s in stream s: every lane, chunk edge and tile edge sees the peak, and the
    release (9598 pairs) crosses the tile boundary"""
    import torch
    lw = 2
    D = (1 << lw) - 1
    n = T + 2 * D + 1
    x = np.random.default_rng(52).integers(-100, 101, size=(n, 2 * n), dtype=np.int64).astype(np.int16)
    x[np.arange(n), 2 * np.arange(n) + (np.arange(n) & 1)] = np.where(np.arange(n) & 2, 32767, -32768)
    with pkg.PcmLimiter(n, lw) as lim:
        host = Host(pkg, n, lw, 1)
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
        assert (rec["at"][:n - D] == np.arange(D, n)).all() and (rec["min_gain"] < 32768).all() and int(rec["limited"][0]) == n


def test_corners_across_three_calls_and_two_tile_borders(pkg, T):
    """delta = 1 with the release spanning three calls and more than two tiles, delta = 2^23, C = 1 and C = 32767, G in {0, 4096, 65536}, and rows on
    the rails"""
    lw, ns = 6, 9
    rng = np.random.default_rng(53)
    cuts = (T + 100, T, 300)
    total = sum(cuts)
    x = rng.integers(-3000, 3001, size=(ns, 2 * total), dtype=np.int64).astype(np.int16)
    x[:, 20:24] = [[32767, -32768, -32768, 32767]]                       # a full-scale burst near the start of every row
    x[6] = np.where(rng.integers(0, 2, 2 * total) > 0, 32767, -32768)    # on the rails throughout
    x[7] = -32768
    x[8] = 32767
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
        assert total - 10 <= int(rec["limited"][0]) <= total and int(host.state[0, -1]) < 1 << 23   # delta = 1: still releasing at the end, two tile borders on
        assert int(rec["limited"][4]) == 0 and int(rec["min_gain"][4]) == 32768             # a gain of 0 limits nothing


def test_cuts_equal_one_call(pkg, rows, T):
    lw, ns = 6, 7
    D = (1 << lw) - 1
    cuts = (T, 1, 11, D, 7, T - 19)
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
    """ramps that end inside a call, that outlast one, that are replaced half way and that J's saturation at 65536 has long ended; new ceilings and
    releases from the next call on"""
    lw, ns, slew = 3, 4, 2
    lim, host = _pair(pkg, ns, lw, slew, pars=False)
    with lim:
        steps = [(700, dict(gain=[4096, 9000, 0, 65536])),               # 4096 -> 65536 takes 30720 pairs at slew 2
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
    # J saturates: 70000 pairs of silence behind a set_gain, then a ramp's end is still where it was
    lim, host = _pair(pkg, 1, 2, 1, pars=False)
    with lim:
        for k in (lim, host):
            k.set_gain(300)
        z = np.zeros((1, 2 * 35000), np.int16)
        for _ in range(2):
            assert np.array_equal(lim.process_batch(z), host.call(z))
        assert lim.get_params()[1] == 65536 and host.holds(lim)
        x = _input(rows, 1, 0, 500)
        assert np.array_equal(lim.process_batch(x), host.call(x)) and host.holds(lim)


def test_device_rows_in_place_padding_and_the_callers_stream(pkg, rows, T):
    """device rows 4 bytes into their allocations with strides of 2n + 2 and 2n + 6: out of place, the padding and a canary row of -32768 are neither
    read nor changed; in place, the same PCM; both on the caller's HIP stream, equal to the host-buffer call"""
    import torch
    lw, ns, n = 6, 5, T + 37
    stream = torch.cuda.Stream()
    x = _input(rows, ns, 0, 2 * n)
    a, b, ref_lim = _pair(pkg, ns, lw)[0], _pair(pkg, ns, lw)[0], _pair(pkg, ns, lw)
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


def test_host_staging_grows_and_is_reused_below_capacity(pkg, rows):
    """host-buffer calls of 1000, 1025 and 3 pairs in that order on one handle of 3 streams, the stream going on from call to call: the staging is
    made, outgrown, and then used far below its capacity with the last call's pairs still behind the valid ones.  PCM, state and records after
    every call are the host routine's"""
    lim, host = _pair(pkg, 3, 6)
    with lim:
        a = 0
        for n in (1000, 1025, 3):
            x = _input(rows, 3, a, a + n)
            a += n
            got, want = lim.process_batch(x), host.call(x)
            assert got.shape == (3, 2 * n) and np.array_equal(got, want), n
            assert host.holds(lim), n


def test_read_with_and_without_reset_and_reset(pkg, rows, T):
    import torch
    lw, ns, n = 6, 3, 1500
    lim, host = _pair(pkg, ns, lw)
    with lim:
        x = _input(rows, ns, 0, 3 * n)
        assert lim.read().tobytes() == pkg.limit.limit_identity(ns).tobytes()
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
        assert np.array_equal(lim.state(), pkg.limit.limit_state_init(lw, ns))
        host.reset()
        assert np.array_equal(lim.process_batch(x[:, :2 * n]), host.call(x[:, :2 * n])) and host.holds(lim)


def test_every_refusal_leaves_the_handle_as_it_was(pkg, rows):
    import torch
    lib = pkg.load_library()
    lw, ns, n = 6, 2, 400
    lim, host = _pair(pkg, ns, lw)
    with lim:
        x = _input(rows, ns, 0, n)
        lim.process_batch(x)
        host.call(x)
        h = lim._h
        d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        o = torch.full((ns, 2 * n + 2), 77, dtype=torch.int16, device="cuda")
        y = np.full((ns, 2 * n), 77, np.int16)
        E, CAP, DEV = pkg.lib.EINVAL, pkg.lib.ECAPACITY, pkg.lib.F_DEVICE_PTRS
        calls = [((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n, 2), E), ((h, x.ctypes.data, 2 * n, (1 << 20) + 1, y.ctypes.data, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n + 1, n, y.ctypes.data, 2 * n, 0), E), ((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n + 1, 0), E),
                 ((h, None, 2 * n, n, y.ctypes.data, 2 * n, 0), E), ((h, x.ctypes.data, 2 * n, n, None, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n - 2, n, y.ctypes.data, 2 * n, 0), CAP), ((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n - 2, 0), CAP),
                 ((h, C.c_void_p(d.data_ptr() + 2), 2 * n, n - 1, C.c_void_p(o.data_ptr()), 2 * n + 2, DEV), E),
                 ((h, C.c_void_p(d.data_ptr()), 2 * n, n, C.c_void_p(o.data_ptr() + 2), 2 * n + 2, DEV), E)]
        for args, want in calls:
            assert lib.sdrfm_pcm_limit_process_batch(*args) == want, args[1:]
        bad32 = np.array([1, 1 << 24], np.uint32)
        rec = np.zeros(ns + 1, pkg.LIMIT_DTYPE)
        assert lib.sdrfm_pcm_limit_set_params(h, None, None) == E
        assert lib.sdrfm_pcm_limit_set_params(h, np.array([1, 0], np.uint32).ctypes.data, None) == E
        assert lib.sdrfm_pcm_limit_set_params(h, np.array([1, 32768], np.uint32).ctypes.data, None) == E
        assert lib.sdrfm_pcm_limit_set_params(h, None, np.array([1, 0], np.uint32).ctypes.data) == E
        assert lib.sdrfm_pcm_limit_set_params(h, np.array([5, 5], np.uint32).ctypes.data, bad32.ctypes.data) == E
        assert lib.sdrfm_pcm_limit_set_gain(h, None, 0) == E and lib.sdrfm_pcm_limit_set_gain(h, np.array([0, 65537], np.uint32).ctypes.data, 0) == E
        assert lib.sdrfm_pcm_limit_set_gain(h, np.array([0, 0], np.uint32).ctypes.data, 2) == E
        assert lib.sdrfm_pcm_limit_read(h, None, 0) == E and lib.sdrfm_pcm_limit_read(h, rec.ctypes.data, 4) == E
        assert lib.sdrfm_pcm_limit_read(h, rec.ctypes.data + 4, 0) == E and lib.sdrfm_pcm_limit_get_state(h, None) == E
        assert (y == 77).all() and bool((o == 77).all()) and not rec.tobytes().strip(b"\0")
        assert host.holds(lim)
        x2 = _input(rows, ns, n, 2 * n)
        assert np.array_equal(lim.process_batch(x2), host.call(x2)) and host.holds(lim)        # and the stream goes on


def test_behind_the_stereo_sink_on_its_stream(pkg):
    """a StereoPcmSink's rows, on the sink's stream, through the limiter in place: the host routine on the PCM the sink returned, under a boost of
    +12 dB and a ceiling of -2 dBFS; the sink's own bits are what they are without the limiter"""
    import torch
    ns, n, lw = 3, 4800, 6
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    rng = np.random.default_rng(54)
    t = np.arange(2 * n) / 48000.0
    left = np.stack([(0.3 + 0.2 * s) * np.sin(2 * np.pi * (400.0 + 300 * s) * t) for s in range(ns)]).astype(np.float32)
    right = (left[::-1] * 0.7 + 0.02 * rng.standard_normal(left.shape)).astype(np.float32)
    with pkg.StereoPcmSink(ns, alpha, gain) as plain:
        sink_pcm = [plain.process_batch(left[:, c * n:(c + 1) * n], right[:, c * n:(c + 1) * n]) for c in range(2)]
    assert max(int(np.abs(p).max()) for p in sink_pcm) > 8000
    stream = torch.cuda.Stream()
    C2, boost = pkg.limit_ceiling(-2.0), int(pkg.normalise_gain_q12(-35.0)[0])
    assert C2 == 26028 and boost == 16306
    with pkg.StereoPcmSink(ns, alpha, gain) as sink, pkg.PcmLimiter(ns, lw, 4) as lim:
        host = Host(pkg, ns, lw, 4)
        sink.set_stream(stream.cuda_stream)
        lim.set_stream(stream.cuda_stream)
        for k in (lim, host):
            k.set_params(C2, pkg.limit_release(0.2))
            k.set_gain(boost)
        d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        torch.cuda.synchronize()
        for c in range(2):
            pcm, lim_out = (torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            sink.process_batch_device(d_l[:, c * n:(c + 1) * n], d_r[:, c * n:(c + 1) * n], pcm)
            lim.process_batch_device(pcm, lim_out)                          # no synchronisation in between: the stream orders them
            lim.synchronize()
            got_sink = pcm.cpu().numpy()
            assert np.array_equal(got_sink, sink_pcm[c]), c                  # the sink's own bits are unchanged
            assert np.array_equal(lim_out.cpu().numpy(), host.call(got_sink)) and host.holds(lim), c
            assert int(np.abs(lim_out.cpu().numpy().astype(np.int64)).max()) <= C2
        assert (lim.read()["limited"] > 0).all()
