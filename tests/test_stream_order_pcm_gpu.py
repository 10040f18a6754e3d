"""The stream-ordering contract of the PCM-side handles with a call still pending (include/sdrfm.h; DESIGN.md §4.28's table): the stereo PCM sink,
the rate matcher, the limiter in both forms, the mix bus and the IQ meter.

Every test has one shape.  The handle is given a caller's stream and makes one call W that is waited for (the kernels are loaded and the carried
state is not the one after create); the stream is held back by a delay that ends by itself (tests/stream_hold.py);
device-pointer call A is enqueued and an event recorded behind it; A is asserted to be pending; the control call is made; what the header says of
its return is asserted (it waited: A's event has completed — or it only enqueued: the delay is still pending); call B is enqueued; and after a
synchronise A's and B's outputs, the handle's records and its state are compared bit for bit with the HOST MODEL RUN IN PROGRAM ORDER: A with the
settings before the control call, B with those behind it.  A and B carry different data, so a call that ran with the other's settings, a read
that copied before A had run, or a reset that overtook A cannot pass.  A stream that was not held FAILS as inconclusive; no test passes vacuously.

Sink and rate matcher reset in stream order and are not documented to wait: their results are asserted, not their return.  The IQ meter's
set_stream does not wait (a deviation kept on purpose): the test pins that A is right once the OLD stream is synchronised and that the next call
runs on the new one.

Not called with a call pending, here or anywhere: the entry points that FREE device memory (every *_disable, a second loudness_enable or
truepeak_enable, *_destroy).  A failure there would be a freed buffer under a running kernel, not a wrong number.  They are covered by reading
the code: each waits through the same call as the setters tested here (host_stream_wait / hipStreamSynchronize on the stream in use) before it
frees.  The handles whose kernels wait on the device (the FM handle, sdrfm_pcm_sink_t, the spectrum handle) stay out as well: on a held stream
such a kernel can spin on a word that only the held queue publishes."""
import time

import numpy as np
import pytest

import audio_meter_ref as am
import hicut_ref as hr
import iq_meter_cases as iqc
import limit_cases as lcases
import loudness_cases as lc
import pcm_mix_cases as mcases
import pcm_mix_ref as mref
import pcm_params as pp
import stream_hold as sh
import truepeak_ref as tp

pytestmark = pytest.mark.gpu
ONE, NONE, SPAN = mcases.ONE, mcases.NONE, mcases.SPAN


@pytest.fixture
def streams():
    """the caller's stream and a second one to switch to"""
    import torch
    return torch.cuda.Stream(), torch.cuda.Stream()


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                                      # the handles' streams do not order themselves against the one that copied
    return t


class Script:
    """the held script: hold, call A, then control calls by what the header promises of their return"""

    def __init__(self, stream, call_a, name):
        import torch
        torch.cuda.synchronize()                                  # the inputs are on the device before anything is held
        self.stream, self.name = stream, name
        self.h = sh.hold(stream)
        sh.still_held(self.h, name + ": call A (device pointers)")
        t0 = time.perf_counter()
        call_a()
        t1 = time.perf_counter()
        self.eA = sh.record(stream)
        sh.only_enqueued(self.h, name + ": call A (device pointers)", t0, t1)

    def waits(self, fn, what):
        what = self.name + ": " + what
        sh.still_held(self.h, what)
        out = fn()
        sh.waited(self.h, self.eA, what)
        return out

    def enqueues(self, fn, what):
        what = self.name + ": " + what
        sh.still_held(self.h, what)
        t0 = time.perf_counter()
        out = fn()
        sh.only_enqueued(self.h, what, t0, time.perf_counter())
        return out

    def ordered(self, fn, what):
        """a call that is stream-ordered and not documented either way: made with A pending; its results are what the test asserts"""
        sh.still_held(self.h, what)
        return fn()


def _switch(sc, dev, other, call_c):
    """set_stream to another stream with A pending (it waits), call C there, and back to the first"""
    sc.waits(lambda: dev.set_stream(other.cuda_stream), "set_stream")
    call_c()
    eC = sh.record(other)
    dev.set_stream(sc.stream.cuda_stream)                         # waits for the stream in use: C
    assert not sh.pending(eC), "set_stream back did not wait for call C on the stream it left"


# ---- the mix bus ------------------------------------------------------------------------------------------------------------------------------------------
MIX = (3, 2, 2)
MIX_N, MIX_SLEW = SPAN + 1, 7
MIX_SRC, MIX_MODE = [[0, 1], [2, 0]], [[0, 1], [4, 2]]
MIX_START, MIX_TARGET = [[ONE, 0], [0, 20000]], [[0, ONE], [ONE, 0]]          # at slew 7 a full fade takes 4682 pairs: W's and A's 4098 end in the middle


def _mix(pkg, stream, ramping=True):
    dev = pkg.PcmMixer(*MIX, MIX_SLEW, pkg.mix_curve("equal_power"))
    host = mcases.HostMixer(pkg, *MIX, MIX_SLEW, pkg.mix_curve("equal_power"))
    for k in (dev, host):
        k.set_routes(MIX_SRC, MIX_MODE)
        k.set_gains(MIX_START, jump=True)
        if ramping:
            k.set_gains(MIX_TARGET)
    dev.set_stream(stream.cuda_stream)
    xw, xa, xb = (mcases.rows(900 + k, MIX[0], MIX_N) for k in range(3))
    assert np.array_equal(dev.process_batch(xw), host.process_batch(xw))          # W, host buffers: the staging is there, the kernel loaded
    return dev, host, xa, xb


MIX_OPS = ["gains", "gains_jump", "routes", "crossfade", "read", "read_reset", "read_device_reset", "host_b", "synchronize", "set_stream", "reset"]


@pytest.mark.parametrize("op", MIX_OPS)
def test_mix_bus(pkg, streams, op):
    import torch
    stream, other = streams
    dev, host, xa, xb = _mix(pkg, stream, ramping=op != "crossfade")
    with dev:
        da, db = _cuda(xa), _cuda(xb)
        oa, ob = (torch.full((MIX[1], 2 * MIX_N), mcases.CANARY, dtype=torch.int16, device="cuda") for _ in range(2))
        d_rec = torch.full((4 * MIX[1],), -1, dtype=torch.int64, device="cuda")
        want_a = host.process_batch(xa)                           # the model runs in program order; its work is kept out of the hold
        sc = Script(stream, lambda: dev.process_batch_device(da, oa, MIX_N), "mix bus")
        b_on_host = None
        if op in ("gains", "gains_jump"):
            new = [[12345, 0], [ONE, 777]]
            if op == "gains":                                     # the set finds every ramp of the script in the middle
                mid = [mref.ramp(int(s["g0"]), int(s["gt"]), MIX_SLEW, host.J) for s in host.slots.reshape(-1)]
                assert all(0 < v < ONE for v in mid[:3]), mid
            sc.waits(lambda: dev.set_gains(new, jump=op == "gains_jump"), "set_gains")
            host.set_gains(new, jump=op == "gains_jump")
            assert host.holds(dev), "get_slots right behind set_gains: not the ramps' values at J after A"
        elif op == "routes":
            sc.waits(lambda: dev.set_routes([[2, 0], [1, NONE]], [[3, 0], [1, 4]]), "set_routes")
            host.set_routes([[2, 0], [1, NONE]], [[3, 0], [1, 4]])
            assert host.holds(dev)
        elif op == "crossfade":
            k = sc.waits(lambda: dev.crossfade(0, 2, "swap"), "crossfade")
            assert k == host.crossfade(0, 2, "swap") == 1 and host.holds(dev)
        elif op in ("read", "read_reset"):
            rec = sc.waits(lambda: dev.read(reset=op == "read_reset"), "read (host)")
            assert rec.tobytes() == host.read(reset=op == "read_reset").tobytes(), "the records read behind A do not include A"
        elif op == "read_device_reset":
            sc.enqueues(lambda: dev.read_device(d_rec, reset=True), "read (device pointers, reset)")
            want_rec = host.read(reset=True)
        elif op == "host_b":
            b_on_host = sc.waits(lambda: dev.process_batch(xb), "process_batch (host buffers)")
        elif op == "synchronize":
            sc.waits(dev.synchronize, "synchronize")
        elif op == "reset":
            sc.waits(dev.reset, "reset")
            host.read(reset=True)
        if op == "set_stream":
            _switch(sc, dev, other, lambda: dev.process_batch_device(db, ob, MIX_N))
        elif op != "host_b":
            dev.process_batch_device(db, ob, MIX_N)
        dev.synchronize()
        want_b = host.process_batch(xb)
        assert np.array_equal(oa.cpu().numpy(), want_a), "call A's output is not the model's with the settings before the control call"
        assert np.array_equal(ob.cpu().numpy() if b_on_host is None else b_on_host, want_b), "call B's output is not the model's with the settings behind it"
        if op == "read_device_reset":
            assert d_rec.cpu().numpy().tobytes() == want_rec.tobytes(), "the records copied on the device do not include A"
        assert dev.read().tobytes() == host.rec.tobytes() and host.holds(dev), "records or slots after B"


# ---- the limiter, both forms --------------------------------------------------------------------------------------------------------------------------------
LIM_NS, LIM_N = 3, lcases.TILE + 1
LIM_FORMS = {"sample": (6, 0), "truepeak": (3, 12)}                # lw, NT (the default 4 x 12 table)
LIM_GAIN0, LIM_GAIN1 = [60000, 100, 30000], [5, 65536, 4096]
LIM_OPS = ["params", "gain", "gain_jump", "get_state", "read", "read_reset", "read_device", "read_device_reset", "host_b", "synchronize", "set_stream",
           "reset"]


@pytest.mark.parametrize("op", LIM_OPS)
@pytest.mark.parametrize("form", list(LIM_FORMS))
def test_limiter(pkg, streams, form, op):
    import torch
    stream, other = streams
    lw, nt = LIM_FORMS[form]
    assert pkg.limit.TILE == lcases.TILE
    lim, host = lcases.pair(pkg, LIM_NS, lw, 1, nt)
    with lim:
        for k in (lim, host):
            k.set_gain(LIM_GAIN0)                                 # ramps that W's and A's 10242 pairs leave in the middle
        lim.set_stream(stream.cuda_stream)
        rng = np.random.default_rng([77, lw, nt])
        xw, xa, xb = (lcases.random_full_range(rng, (LIM_NS, 2 * LIM_N)) for _ in range(3))
        da, db = _cuda(xa), _cuda(xb)
        oa, ob = torch.zeros_like(da), torch.zeros_like(db)
        assert np.array_equal(lim.process_batch(xw), host.call(xw))
        d_rec = torch.full((4 * LIM_NS,), -1, dtype=torch.int64, device="cuda")
        want_a = host.call(xa)
        sc = Script(stream, lambda: lim.process_batch_device(da, oa, LIM_N), "limiter " + form)
        assert any(g != t for g, t in zip(host.now(), LIM_GAIN0)), "the script's ramps are over: nothing is set in the middle of one"
        b_on_host, want_rec = None, None
        if op == "params":
            sc.waits(lambda: lim.set_params([3000, 32767, 1], [1 << 23, 1, 5000]), "set_params")
            host.set_params([3000, 32767, 1], [1 << 23, 1, 5000])
        elif op in ("gain", "gain_jump"):
            sc.waits(lambda: lim.set_gain(LIM_GAIN1, jump=op == "gain_jump"), "set_gain")
            host.set_gain(LIM_GAIN1, jump=op == "gain_jump")
            par, J = lim.get_params()
            assert par.tobytes() == host.par.tobytes() and J == host.J == 0, "get_params right behind set_gain: not the ramps' values at J after A"
        elif op == "get_state":
            st = sc.waits(lim.state, "get_state")
            assert np.array_equal(st, host.state), "the state read behind A is not the state A leaves"
        elif op in ("read", "read_reset"):
            rec = sc.waits(lambda: lim.read(reset=op == "read_reset"), "read (host)")
            assert rec.tobytes() == host.rec.tobytes(), "the records read behind A do not include A"
        elif op in ("read_device", "read_device_reset"):
            sc.enqueues(lambda: lim.read_device(d_rec, reset=op == "read_device_reset"), "read (device pointers%s)" % (", reset" if "reset" in op else ""))
            want_rec = host.rec.copy()
        elif op == "host_b":
            b_on_host = sc.waits(lambda: lim.process_batch(xb), "process_batch (host buffers)")
        elif op == "synchronize":
            sc.waits(lim.synchronize, "synchronize")
        elif op == "reset":
            sc.waits(lim.reset, "reset")
            host.reset()
        if op.endswith("_reset"):
            host.rec = pkg.limit.limit_identity(LIM_NS)           # the reset value: the join's identity, the state stays
        if op == "set_stream":
            _switch(sc, lim, other, lambda: lim.process_batch_device(db, ob, LIM_N))
        elif op != "host_b":
            lim.process_batch_device(db, ob, LIM_N)
        lim.synchronize()
        want_b = host.call(xb)
        assert np.array_equal(oa.cpu().numpy(), want_a), "call A's output is not the model's with the settings before the control call"
        assert np.array_equal(ob.cpu().numpy() if b_on_host is None else b_on_host, want_b), "call B's output is not the model's with the settings behind it"
        if want_rec is not None:
            assert d_rec.cpu().numpy().tobytes() == want_rec.tobytes(), "the records copied on the device do not include A"
        assert host.holds(lim), "parameters, J, state or records after B"


LIM_MANY = 8192                                                    # 256 KiB of records: no longer a copy the runtime may take in one small piece


def test_limiter_device_read_with_reset_at_many_streams(pkg, streams):
    """the identity image a device read with reset puts back is 32 bytes a stream: at 8192 streams the copy that restores it is 256 KiB, and the
    call still only enqueues; the records copied include A, and B's records start from the identity"""
    import torch
    stream, _ = streams
    n = 64
    lim, host = lcases.pair(pkg, LIM_MANY, 6, 1, 0)
    with lim:
        lim.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(79)
        xw, xa, xb = (lcases.random_full_range(rng, (LIM_MANY, 2 * n)) for _ in range(3))
        da, db = _cuda(xa), _cuda(xb)
        oa, ob = torch.zeros_like(da), torch.zeros_like(db)
        d_rec = torch.full((4 * LIM_MANY,), -1, dtype=torch.int64, device="cuda")
        assert np.array_equal(lim.process_batch(xw), host.call(xw))
        want_a = host.call(xa)
        want_rec = host.rec.copy()
        sc = Script(stream, lambda: lim.process_batch_device(da, oa, n), "limiter, %d streams" % LIM_MANY)
        sc.enqueues(lambda: lim.read_device(d_rec, reset=True), "read (device pointers, reset)")
        lim.process_batch_device(db, ob, n)
        lim.synchronize()
        host.rec = pkg.limit.limit_identity(LIM_MANY)
        want_b = host.call(xb)
        assert np.array_equal(oa.cpu().numpy(), want_a) and np.array_equal(ob.cpu().numpy(), want_b)
        assert d_rec.cpu().numpy().tobytes() == want_rec.tobytes(), "the records copied on the device do not include A"
        assert host.holds(lim), "parameters, J, state or records after B"


# ---- the rate matcher ---------------------------------------------------------------------------------------------------------------------------------------
RATE_NS, RATE_N = 3, 1540                                         # 1026 outputs at the largest step, 3/2: a second span of the kernel
RATE_OPS = ["set_step", "count", "get_state", "host_b", "synchronize", "set_stream", "reset"]


class HostRate:
    """pkg.pcm_rate_host per stream, carried from call to call"""

    def __init__(self, pkg, coef, steps):
        self.pkg, self.coef, self.steps = pkg, coef, list(steps)
        self.reset()

    def reset(self):
        self.pos, self.hist = [0] * len(self.steps), [None] * len(self.steps)

    def call(self, x):
        out = []
        for s in range(len(self.steps)):
            o, self.pos[s], self.hist[s] = self.pkg.pcm_rate_host(x[s], self.coef, self.steps[s], self.pos[s], self.hist[s])
            out.append(o)
        return out


def _rate_rows(out, cnt):
    return [out[s, :2 * int(cnt[s])] for s in range(len(cnt))]


def _same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("op", RATE_OPS)
def test_rate_matcher(pkg, streams, op):
    import torch
    stream, other = streams
    coef = pkg.rate_coef()
    old = [pkg.step_for(48000, 48000, 100.0), pkg.step_for(48000, 44100), pkg.step_for(48000, 32000)]
    new = [pkg.step_for(48000, 32000, -50.0), pkg.step_for(48000, 48000, -300.0), pkg.step_for(48000, 44100, 20.0)]
    host = HostRate(pkg, coef, old)
    with pkg.PcmRateMatcher(RATE_NS, coef) as rm:
        rm.set_step(old)
        rm.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(88)
        xw, xa, xb = (lcases.random_full_range(rng, (RATE_NS, 2 * RATE_N)) for _ in range(3))
        da, db = _cuda(xa), _cuda(xb)
        width = 2 * (RATE_N * 4 + 2)                              # room for the smallest step the matcher takes
        oa, ob = (torch.full((RATE_NS, width), 0x5A5B, dtype=torch.int16, device="cuda") for _ in range(2))
        cnt = {}
        assert _same_rows(rm.process_batch(xw), host.call(xw))
        want_a = host.call(xa)
        sc = Script(stream, lambda: cnt.update(a=rm.process_batch_device(da, oa, RATE_N)), "rate matcher")
        assert min(len(w) for w in want_a) // 2 >= 1025
        b_on_host = None
        if op == "set_step":
            sc.waits(lambda: rm.set_step(new), "set_step")
            host.steps = list(new)
        elif op == "count":
            got, mx = sc.enqueues(lambda: rm.count(RATE_N), "count")
            want = [len(o) // 2 for o in HostRate.call(_copy_rate(host), xb)]
            assert list(got) == want and mx == max(want), "count behind a pending call is not the next call's counts"
        elif op == "get_state":
            step, pos = sc.waits(rm.state, "get_state")          # SDRFM_OK: the mirror is the device's pos
            assert list(pos) == host.pos and list(step) == old
        elif op == "host_b":
            b_on_host = sc.waits(lambda: rm.process_batch(xb), "process_batch (host buffers)")
        elif op == "synchronize":
            sc.waits(rm.synchronize, "synchronize")
        elif op == "reset":
            sc.ordered(rm.reset, "reset")
            host.reset()
        if op == "set_stream":
            _switch(sc, rm, other, lambda: cnt.update(b=rm.process_batch_device(db, ob, RATE_N)))
        elif op != "host_b":
            cnt["b"] = rm.process_batch_device(db, ob, RATE_N)
        rm.synchronize()
        want_b = host.call(xb)
        assert _same_rows(_rate_rows(oa.cpu().numpy(), cnt["a"]), want_a), "call A's counts or outputs are not the model's at the steps before the control call"
        got_b = _rate_rows(ob.cpu().numpy(), cnt["b"]) if b_on_host is None else b_on_host
        assert _same_rows(got_b, want_b), "call B's counts or outputs are not the model's at the steps behind it, from B's first output"
        step, pos = rm.state()
        assert list(pos) == host.pos and list(step) == host.steps


def _copy_rate(host):
    c = HostRate(host.pkg, host.coef, host.steps)
    c.pos, c.hist = list(host.pos), [None if h is None else h.copy() for h in host.hist]
    return c


# ---- the stereo PCM sink, exact form, with its three meters -------------------------------------------------------------------------------------------------
SINK_NS, SINK_N, SINK_QUIET, SINK_BL = 3, 4865, 8, 480
SINK_OPS = ["hicut_on", "hicut_retarget", "hicut_off", "meter_enable", "meter_read", "meter_read_reset", "meter_read_device", "meter_read_device_reset",
            "truepeak_read", "truepeak_read_reset", "truepeak_read_device", "truepeak_read_device_reset", "loudness_read", "loudness_get_state",
            "get_state", "host_b", "synchronize", "set_stream", "reset"]


def _join(mod, acc, rec):
    return np.array([mod.join(a, b) for a, b in zip(acc, rec)], dtype=mod.DTYPE)


class HostSink:
    """the host de-emphasis routines, plain and with high-cut, and the three meters' definitions over the PCM they give, in program order"""

    def __init__(self, pkg, alpha, gain):
        self.pkg, self.alpha, self.gain = pkg, alpha, gain
        self.hc = hr.HicutState(SINK_NS)
        self.reset()

    def reset(self):
        self.state = [(0.0, 0.0)] * SINK_NS
        self.meter, self.tprec, self.tphist = np.zeros(SINK_NS, am.DTYPE), np.zeros(SINK_NS, tp.DTYPE), None
        self.lstate, self.blocks = None, []
        self.hc.complete()

    def call(self, left, right):
        h0, ht, slew, J = self.hc.call(left.shape[1])
        pcm = np.zeros((SINK_NS, 2 * left.shape[1]), np.int16)
        for s in range(SINK_NS):
            if self.hc.on:
                pcm[s], self.state[s] = self.pkg.pcm_deemph_stereo_hicut_s16_host(left[s], right[s], self.alpha, self.gain, h0[s], ht[s], slew, J, self.state[s])
            else:
                pcm[s], self.state[s] = self.pkg.pcm_deemph_stereo_s16_host(left[s], right[s], self.alpha, self.gain, self.state[s])
        self.meter = _join(am, self.meter, am.records(pcm, SINK_QUIET))
        rec, self.tphist = tp.records(pcm, hist=self.tphist)
        self.tprec = _join(tp, self.tprec, rec)
        e, self.lstate = self.pkg.pcm_loudness_host(pcm, SINK_BL, state=self.lstate)
        self.blocks.append(e)
        return pcm

    def states(self):
        return np.array(self.state, np.float32)


def _audio(seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(-2.2, 2.2, (SINK_NS, SINK_N)).astype(np.float32) for _ in range(2))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("op", SINK_OPS)
def test_stereo_sink(pkg, streams, op):
    import torch
    stream, other = streams
    alpha = pp.alpha_of(pkg.load_library(), "75us")
    host = HostSink(pkg, alpha, pp.DEFAULT_GAIN)
    h_first, h_next = np.array([8192, 1024, 20000], np.uint16), np.array([32768, 30000, 1024], np.uint16)
    with pkg.StereoPcmSink(SINK_NS, alpha, pp.DEFAULT_GAIN, exact=True) as sink:
        sink.enable_meter(SINK_QUIET)
        sink.enable_truepeak()
        sink.enable_loudness(SINK_BL, 64)
        lib = sink._lib
        set_hicut = lambda q, slew: sink._ck(lib.sdrfm_pcm_stereo_sink_set_hicut(sink._h, None if q is None else q.ctypes.data, slew), "set_hicut")
        if op in ("hicut_retarget", "hicut_off"):
            set_hicut(h_first, 2)                                 # 2 Q15 units a sample: W's and A's 9730 samples leave the wide ramps in the middle
            host.hc.set(h_first, 2)
        sink.set_stream(stream.cuda_stream)
        (lw, rw), (la, ra), (lb, rb) = _audio(4), _audio(5), _audio(6)
        dla, dra, dlb, drb = (_cuda(x) for x in (la, ra, lb, rb))
        oa, ob = (torch.zeros((SINK_NS, 2 * SINK_N), dtype=torch.int16, device="cuda") for _ in range(2))
        d_am = torch.full((24 * SINK_NS,), -1, dtype=torch.int64, device="cuda")
        d_tp = torch.full((8 * SINK_NS,), -1, dtype=torch.int64, device="cuda")
        assert np.array_equal(sink.process_batch(lw, rw), host.call(lw, rw))
        want_a = host.call(la, ra)
        sc = Script(stream, lambda: sink.process_batch_device(dla, dra, oa, SINK_N), "stereo sink")
        b_on_host, behind = None, None
        if op in ("hicut_on", "hicut_retarget"):
            if op == "hicut_retarget":
                now = host.hc.now()
                assert (now != host.hc.ht).any(), "the script's ramps are over: nothing is re-targeted in the middle of one"
            q, slew = (h_first, 7) if op == "hicut_on" else (h_next, 40)
            sc.waits(lambda: set_hicut(q, slew), "set_hicut")
            host.hc.set(q, slew)
            host.hc.check(sink.hicut_state())
        elif op == "hicut_off":
            sc.waits(lambda: set_hicut(None, 0), "set_hicut (off)")
            host.hc.set(None, 0)
        elif op == "meter_enable":
            sc.waits(lambda: sink.enable_meter(SINK_QUIET), "meter_enable (on an enabled sink)")
            host.meter = np.zeros(SINK_NS, am.DTYPE)              # it zeroes BEHIND A
        elif op.startswith("meter_read"):
            reset = op.endswith("reset")
            if "device" in op:
                sc.enqueues(lambda: sink.read_meters_device(d_am, reset=reset), "meter_read (device pointers)")
                behind = ("audio meter", d_am, host.meter.copy())
            else:
                got = sc.waits(lambda: sink.read_meters(reset=reset), "meter_read (host)")
                assert am.same(got, host.meter), ("the audio meter's records read behind A do not include A", am.diff(got, host.meter))
            if reset:
                host.meter = np.zeros(SINK_NS, am.DTYPE)
        elif op.startswith("truepeak_read"):
            reset = op.endswith("reset")
            if "device" in op:
                sc.enqueues(lambda: sink.read_truepeak_device(d_tp, reset=reset), "truepeak_read (device pointers)")
                behind = ("true-peak meter", d_tp, host.tprec.copy())
            else:
                got = sc.waits(lambda: sink.read_truepeak(reset=reset), "truepeak_read (host)")
                assert tp.same(got, host.tprec), ("the true-peak records read behind A do not include A", tp.diff(got, host.tprec))
            if reset:
                host.tprec = np.zeros(SINK_NS, tp.DTYPE)          # the records only: the history stays
        elif op == "loudness_read":
            first, got = sc.waits(sink.read_loudness, "loudness_read")
            ok, why = lc.within(got, np.concatenate(host.blocks, axis=1), SINK_BL)
            assert first == 0 and got.shape[1] == 2 * SINK_N // SINK_BL and ok, ("the sub-blocks read behind A do not end with A's", why)
            host.blocks = []
        elif op == "loudness_get_state":
            got = sc.waits(sink.loudness_state, "loudness_get_state")
            ok, why = lc.within(got["e"], host.lstate["e"], SINK_BL)
            assert np.array_equal(got["pos"], host.lstate["pos"]) and ok, ("the loudness state read behind A is not the one A leaves", why)
        elif op == "get_state":
            got = sc.waits(sink.state, "get_state")
            assert np.array_equal(_bits(got), _bits(host.states())), "the de-emphasis states read behind A are not the ones A leaves"
        elif op == "host_b":
            b_on_host = sc.waits(lambda: sink.process_batch(lb, rb), "process_batch (host buffers)")
        elif op == "synchronize":
            sc.waits(sink.synchronize, "synchronize")
        elif op == "reset":
            sc.ordered(sink.reset, "reset")
            host.reset()
        if op == "set_stream":
            _switch(sc, sink, other, lambda: sink.process_batch_device(dlb, drb, ob, SINK_N))
        elif op != "host_b":
            sink.process_batch_device(dlb, drb, ob, SINK_N)
        sink.synchronize()
        want_b = host.call(lb, rb)
        assert np.array_equal(oa.cpu().numpy(), want_a), "call A's PCM is not the host routine's with the settings before the control call"
        assert np.array_equal(ob.cpu().numpy() if b_on_host is None else b_on_host, want_b), "call B's PCM is not the host routine's with the settings behind it"
        if behind is not None:
            what, d_out, want = behind
            assert d_out.cpu().numpy().tobytes() == want.tobytes(), "the %s's records copied on the device do not include A" % what
        assert np.array_equal(_bits(sink.state()), _bits(host.states())), "the de-emphasis states after B"
        got_am, got_tp = sink.read_meters(reset=False), sink.read_truepeak(reset=False)
        assert am.same(got_am, host.meter), ("the audio meter's records after B", am.diff(got_am, host.meter))
        assert tp.same(got_tp, host.tprec), ("the true-peak records after B", tp.diff(got_tp, host.tprec))
        first, got = sink.read_loudness()                          # the sub-blocks completed and not read yet, in order
        want_e = np.concatenate(host.blocks, axis=1)
        ok, why = lc.within(got, want_e, SINK_BL)
        assert first == int(host.lstate["pos"][0]) // SINK_BL - want_e.shape[1] and ok, ("the loudness sub-blocks after B", first, why)
        dev_l = sink.loudness_state()
        assert np.array_equal(dev_l["pos"], host.lstate["pos"]) and lc.within(dev_l["e"], host.lstate["e"], SINK_BL)[0], "the loudness state after B"
        host.hc.check(sink.hicut_state())


# ---- the IQ meter -------------------------------------------------------------------------------------------------------------------------------------------
IQ_NS, IQ_NBYTES, IQ_STRIDE = 3, iqc.CHUNK + 34, iqc.CHUNK + 34 + 7   # an odd stride: every row at another address mod 16


def _iq_rows(seed):
    import torch
    x = iqc.random_rows(seed, IQ_NS, IQ_NBYTES)
    flat = torch.zeros(IQ_NS * IQ_STRIDE, dtype=torch.uint8, device="cuda")
    flat.view(IQ_NS, IQ_STRIDE)[:, :IQ_NBYTES] = _cuda(x)
    return x, flat


def _iq_out():
    import torch
    return torch.full((8 * IQ_NS,), -1, dtype=torch.int64, device="cuda"), torch.full((512 * IQ_NS,), -1, dtype=torch.int32, device="cuda")


def _iq_is(pkg, rec, rows, x):
    want_rec, want_rows = pkg.iq_meter_host(x, with_hist=True)
    got_rows = rows.cpu().numpy().view(np.uint32).reshape(IQ_NS, 512) if hasattr(rows, "cpu") else rows
    got_rec = rec.cpu().numpy() if hasattr(rec, "cpu") else rec
    return got_rec.tobytes() == want_rec.tobytes() and np.array_equal(got_rows.astype(np.uint64), want_rows)


@pytest.mark.parametrize("op", ["host_b", "synchronize", "set_stream"])
def test_iq_meter(pkg, streams, op):
    stream, other = streams
    (xa, da), (xb, db) = _iq_rows(31), _iq_rows(32)
    (ra, ha), (rb, hb) = _iq_out(), _iq_out()
    with pkg.IqMeter(IQ_NS, IQ_NBYTES) as im:
        im.set_stream(stream.cuda_stream)
        assert _iq_is(pkg, *im.process_batch(xb[::-1], hist=True), xb[::-1])
        sc = Script(stream, lambda: im.process_batch_ptr(da.data_ptr(), IQ_STRIDE, IQ_NBYTES, ra.data_ptr(), ha.data_ptr()), "IQ meter")
        if op == "host_b":
            # the staging, d_meters and d_hist are the handle's and the device call's outputs the caller's: both calls right
            rec_b, rows_b = sc.waits(lambda: im.process_batch(xb, hist=True), "process_batch (host buffers)")
            assert _iq_is(pkg, rec_b, rows_b, xb), "the host-buffer call behind a pending device call"
        elif op == "synchronize":
            sc.waits(im.synchronize, "synchronize")
        else:
            # the deviation kept on purpose: set_stream does NOT wait for the stream in use.  Pinned: the switch returns with A
            # pending, call C runs on the NEW stream (it completes while the old one is still held), and A is right once the OLD stream is waited for
            sc.enqueues(lambda: im.set_stream(other.cuda_stream), "set_stream (the IQ meter's does not wait)")
            im.process_batch_ptr(db.data_ptr(), IQ_STRIDE, IQ_NBYTES, rb.data_ptr(), hb.data_ptr())
            eC = sh.record(other)
            im.synchronize()                                      # the stream in use now: the new one
            assert not sh.pending(eC)
            sh.still_held(sc.h, "call C completed on the new stream while the old one was held")
            assert _iq_is(pkg, rb, hb, xb), "call C on the new stream"
            stream.synchronize()
        if op != "set_stream":
            im.process_batch_ptr(db.data_ptr(), IQ_STRIDE, IQ_NBYTES, rb.data_ptr(), hb.data_ptr())
            im.synchronize()
            assert _iq_is(pkg, rb, hb, xb), "call B"
        assert _iq_is(pkg, ra, ha, xa), "call A's records and rows, in the caller's buffers"
