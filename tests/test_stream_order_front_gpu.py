"""The stream-ordering contract of the pilot-front handles with a call still pending (include/sdrfm.h; DESIGN.md §4.28's table): the broadcast
receiver in full, and reset, tune and set_stream on the stereo, RDS and scan handles where they have them.

The shape of every test is tests/test_stream_order_pcm_gpu.py's: the handle on a caller's stream, one call W that is waited for, the stream held
(tests/stream_hold.py), device-pointer call A with an event behind it, the control call with what the header says of its return asserted, call B, a
synchronise.  The expected values come from a SECOND HANDLE of the same configuration that plays the same script on a stream that is not held,
with a full synchronise after every step: its calls are the ones the rest of the suite holds to the references.  L, R, bb, PCM, the pilot counts
and the integer records are compared by equality (the kernels' split of a row over workgroups is a function of the shape, and the records are
integer sums: nothing here depends on the order in which workgroups run).  A and B carry different data.

The default shape of tests/tuned_cases.py on 3 streams, that module's NBYTES per call; the untuned stereo and RDS handles get centred stations.

The one-call PCM forms are tested in the arrangement the header allows while calls are pending: the sink was given the handle's stream.
set_stream on the four pilot-front handles waits for the stream in use, as the PCM-side handles' does.

Not called with a call pending: what frees device memory (*_destroy, the sink's *_disable and second enables); see the PCM file's docstring."""
import numpy as np
import pytest

import pcm_params as pp
import stream_hold as sh
import tuned_cases as tc
from test_stream_order_pcm_gpu import Script, _cuda, streams  # noqa: F401  (the fixture and the held script are that file's)

pytestmark = pytest.mark.gpu

CASE = ("default", 3, "signal")
NS, NBYTES = CASE[1], tc.NBYTES
SHAPE = tc.SHAPES[CASE[0]]
T, D, P, Ta, Da, Tr, Dr = SHAPE
FS = tc.fs_of(D)
SHIFT_HZ = 5e3                                                    # the second tuning: every stream 5 kHz beside the first

_made = {}


class Plain:
    """the reference's side of Script: the same steps on a stream that is not held, with a full synchronise after every one"""

    def __init__(self, handle, call_a):
        import torch
        torch.cuda.synchronize()                                  # the buffers are filled before the handle's own stream writes them
        self.sync = handle.synchronize
        call_a()
        self.sync()

    def _step(self, fn, what):
        out = fn()
        self.sync()
        return out

    waits = enqueues = ordered = _step


def _setup(pkg):
    """the case's rows and tunings, made once: iq A and B (the case's rows, and the same stations from another point of the capture), the
    first tuning and the second with its carry"""
    if "su" not in _made:
        su = tc.case_setup(pkg, CASE)
        h = su["taps"][0]
        hz = [c * FS for c in su["cycles"]]
        su["iq_b"] = np.ascontiguousarray(np.roll(su["iq"], 2 * 17001, axis=1))
        su["iq_w"] = np.ascontiguousarray(np.roll(su["iq"], 2 * 40003, axis=1))
        su["ctaps2"] = np.stack([pkg.tuned_channel_taps(h, f + SHIFT_HZ, FS) for f in hz])
        su["rot2"] = np.array([pkg.tuned_rotation(f + SHIFT_HZ, FS, D) for f in hz], np.float32)
        su["carry"] = np.stack([pkg.retune_carry(f, f + SHIFT_HZ, T, FS) for f in hz]).astype(np.float32)
        _made["su"] = su
    return _made["su"]


def _centred(pkg):
    """three centred stations for the untuned handles, rows W, A and B: made once"""
    if "centred" not in _made:
        rows = np.stack([pkg.make_iq_rds(1, 3 * NBYTES // 2, tc.GROUPS, fs=FS, rds_phase=0.4 * s, first_id=6100 + s)[0] for s in range(NS)])
        _made["centred"] = tuple(np.ascontiguousarray(rows[:, k * NBYTES:(k + 1) * NBYTES]) for k in range(3))
    return _made["centred"]


def _bcast(pkg, su):
    h, ga, gr, b, dg, rg = su["taps"]
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b, pilot_min=su["pilot_min"], diff_gain=dg,
                                                rds_gain=rg, fir_decim=D, audio_decim=Da, rds_decim=Dr, n_streams=NS, max_bytes_per_call=NBYTES))
    bc.tune(ctaps=su["ctaps"], rot=su["rot"])
    return bc


class Rows:
    """one call's device outputs of a broadcast handle, and what the test keeps of them"""

    def __init__(self, bc, pcm=False):
        import torch
        na, nr = bc.counts(NBYTES)
        self.left, self.right = (torch.full((NS, na + 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        self.bb = torch.full((NS, 2 * nr + 2), 7.0, dtype=torch.float32, device="cuda")
        self.pc = torch.full((NS,), -1, dtype=torch.int32, device="cuda")
        self.meters = torch.full((NS, 8), -1, dtype=torch.int64, device="cuda")
        self.pcm = torch.full((NS, 2 * na + 2), 0x5A5B, dtype=torch.int16, device="cuda") if pcm else None

    def host(self):
        out = dict(left=self.left, right=self.right, bb=self.bb, pc=self.pc, meters=self.meters)
        if self.pcm is not None:
            out["pcm"] = self.pcm
        return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


def _same(got, want):
    """every kept item by equality; the names of those that differ"""
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [k for k in got if got[k] != want[k]]


def _play(pkg, script, stream):
    """the script on a held stream against the same script on a handle whose stream is not held"""
    got = script(pkg, stream, True)
    want = script(pkg, None, False)
    differ = _same(got, want)
    assert not differ, "held and in program order differ in %s: a call ran with the other call's settings, or a read or reset overtook call A" % differ


# ---- the broadcast receiver -------------------------------------------------------------------------------------------------------------------------------
BCAST_OPS = ["tune", "untune", "retune_carry", "retune_restart", "set_audio", "clear_audio", "reset", "metered_b", "host_b", "synchronize", "set_stream"]


@pytest.mark.parametrize("op", BCAST_OPS)
def test_broadcast_receiver(pkg, streams, op):
    stream, other = streams
    su = _setup(pkg)
    d_a, d_b = _cuda(su["iq"]), _cuda(su["iq_b"])

    def script(pkg, stream, held):
        kept = {}
        with _bcast(pkg, su) as bc:
            if held:
                bc.set_stream(stream.cuda_stream)
            if op == "clear_audio":
                bc.set_audio(blend=[0.0, 0.5, 1.0], gain=[1.0, 0.25, 0.5], ramp_ms=100.0)  # 4800 outputs: W's and A's 2500 end in the middle
            kept["w"] = [np.ascontiguousarray(v).tobytes() for v in bc.process_batch(su["iq_w"])]
            ra, rb = Rows(bc), Rows(bc)
            call_a = lambda: bc.process_batch_device(d_a, ra.left, ra.right, ra.bb, ra.pc)
            sc = Script(stream, call_a, "broadcast receiver") if held else Plain(bc, call_a)
            if op == "tune":
                sc.waits(lambda: bc.tune(ctaps=su["ctaps2"], rot=su["rot2"]), "tune")
            elif op == "untune":
                sc.waits(bc.tune, "tune (back to the untuned kernels)")
            elif op == "retune_carry":                            # the state kept, carried over to the new offsets
                sc.waits(lambda: bc.retune(ctaps=su["ctaps2"], rot=su["rot2"], carry=su["carry"]), "retune (state kept, with carry)")
            elif op == "retune_restart":                          # two streams restarted, the third carried
                sc.waits(lambda: bc.retune(ctaps=su["ctaps2"], rot=su["rot2"], carry=su["carry"], restart=[1, 0, 1]), "retune (two streams restarted)")
            elif op == "set_audio":
                sc.waits(lambda: bc.set_audio(blend=[0.0, 0.5, 1.0], gain=[1.0, 0.25, 0.5], ramp_ms=40.0), "set_audio")
                kept["audio"] = {k: v.tobytes() for k, v in bc.audio_state().items()}
            elif op == "clear_audio":
                sc.waits(bc.clear_audio, "set_audio (off)")
            elif op == "reset":
                sc.waits(bc.reset, "reset")
            elif op == "synchronize":
                sc.waits(bc.synchronize, "synchronize")
            if op == "metered_b":                                 # a metered call behind a pending plain call: it only enqueues
                sc.enqueues(lambda: bc.process_batch_metered_device(d_b, rb.left, rb.right, rb.bb, rb.meters, rb.pc), "metered call (device pointers)")
            elif op == "host_b":
                out = sc.waits(lambda: bc.process_batch(su["iq_b"]), "process_batch (host buffers)")
                kept["b_host"] = [np.ascontiguousarray(v).tobytes() for v in out]
            elif op == "set_stream" and held:
                sc.waits(lambda: bc.set_stream(other.cuda_stream), "set_stream")
                bc.process_batch_device(d_b, rb.left, rb.right, rb.bb, rb.pc)
                eC = sh.record(other)
                bc.set_stream(stream.cuda_stream)
                assert not sh.pending(eC), "set_stream back did not wait for call C on the stream it left"
            else:
                bc.process_batch_device(d_b, rb.left, rb.right, rb.bb, rb.pc)
            bc.synchronize()
            kept["name"] = bc.kernel_name
            kept["a"], kept["b"] = ra.host(), rb.host()
        return {k: (repr(sorted(v.items())) if isinstance(v, dict) else repr(v)) for k, v in kept.items()}

    _play(pkg, script, stream)
    if op == "tune":                                              # the script is what it says: B under the second tuning is not B under the first
        assert not np.array_equal(su["ctaps"], su["ctaps2"])


# ---- the one-call PCM form with a sink that was given the handle's stream -----------------------------------------------------------------------------------
PCM_OPS = ["set_hicut", "meter_read", "meter_read_device", "truepeak_read", "get_state"]


@pytest.mark.parametrize("op", PCM_OPS)
def test_one_call_pcm_form_with_the_sink_on_the_handles_stream(pkg, streams, op):
    import torch
    stream, _ = streams
    su = _setup(pkg)
    d_a, d_b = _cuda(su["iq"]), _cuda(su["iq_b"])
    alpha = pp.alpha_of(pkg.load_library(), "75us")

    def script(pkg, stream, held):
        kept = {}
        with _bcast(pkg, su) as bc, pkg.StereoPcmSink(NS, alpha, pp.DEFAULT_GAIN) as sink:
            sink.enable_meter(8)
            sink.enable_truepeak()
            if held:                                              # both on the caller's stream: the arrangement the header allows
                bc.set_stream(stream.cuda_stream)
                sink.set_stream(stream.cuda_stream)
            kept["w"] = [np.ascontiguousarray(v).tobytes() for v in bc.process_batch_pcm(sink, su["iq_w"])]
            ra, rb = Rows(bc, pcm=True), Rows(bc, pcm=True)
            d_rec = torch.full((24 * NS,), -1, dtype=torch.int64, device="cuda")
            call_a = lambda: bc.process_batch_pcm_device(sink, d_a, ra.left, ra.right, ra.pcm, ra.bb, ra.pc)
            sc = Script(stream, call_a, "one-call PCM form") if held else Plain(bc, call_a)
            if op == "set_hicut":
                sc.waits(lambda: sink.set_hicut(np.array([8192, 1024, 20000], np.uint16), ramp_ms=50.0), "sink set_hicut")
            elif op == "meter_read":
                kept["read"] = sc.waits(lambda: sink.read_meters(reset=True), "sink meter_read (host)").tobytes()
            elif op == "meter_read_device":
                sc.enqueues(lambda: sink.read_meters_device(d_rec, reset=True), "sink meter_read (device pointers)")
            elif op == "truepeak_read":
                kept["read"] = sc.waits(lambda: sink.read_truepeak(reset=False), "sink truepeak_read (host)").tobytes()
            elif op == "get_state":
                kept["read"] = sc.waits(sink.state, "sink get_state").tobytes()
            bc.process_batch_pcm_device(sink, d_b, rb.left, rb.right, rb.pcm, rb.bb, rb.pc)
            bc.synchronize()
            kept["a"], kept["b"], kept["rec"] = ra.host(), rb.host(), d_rec.cpu().numpy().tobytes()
            kept["after"] = [sink.state().tobytes(), sink.read_meters(reset=False).tobytes(), sink.read_truepeak(reset=False).tobytes(),
                             repr(sink.hicut_state())]
        return {k: repr(sorted(v.items())) if isinstance(v, dict) else repr(v) for k, v in kept.items()}

    _play(pkg, script, stream)


# ---- reset, tune and set_stream on the stereo, RDS and scan handles ---------------------------------------------------------------------------------------
def _stereo(pkg, su):
    h, ga, gr, b, dg, rg = su["taps"]
    return pkg.StereoDemod(pkg.StereoConfig(fir_coeffs=h, audio_coeffs=ga, pilot_coeffs=b, diff_gain=dg, fir_decim=D, audio_decim=Da, n_streams=NS,
                                            max_bytes_per_call=NBYTES))


def _rds(pkg, su):
    h, ga, gr, b, dg, rg = su["taps"]
    return pkg.RdsDemod(pkg.RdsConfig(fir_coeffs=h, pilot_coeffs=b, rds_coeffs=gr, rds_gain=rg, fir_decim=D, rds_decim=Dr, n_streams=NS,
                                      max_bytes_per_call=NBYTES))


def _scan(pkg, su):
    return pkg.ScanDemod(pkg.ScanConfig(pilot_coeffs=su["taps"][3], ctaps=su["ctaps"], rot=su["rot"], fir_decim=D, max_bytes_per_call=NBYTES))


def _outputs(kind, n):
    import torch
    if kind == "stereo":
        return [torch.full((NS, n + 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)] + [torch.full((NS,), -1, dtype=torch.int32, device="cuda")]
    if kind == "rds":
        return [torch.full((NS, 2 * n + 2), 7.0, dtype=torch.float32, device="cuda"), torch.full((NS,), -1, dtype=torch.int32, device="cuda")]
    return [torch.full((NS, 8), -1, dtype=torch.int64, device="cuda")]


FRONT_OPS = [("stereo", "reset"), ("stereo", "set_stream"), ("rds", "reset"), ("rds", "set_stream"), ("scan", "reset"), ("scan", "tune"),
             ("scan", "set_stream")]


@pytest.mark.parametrize("kind,op", FRONT_OPS, ids=["%s-%s" % k for k in FRONT_OPS])
def test_stereo_rds_and_scan_handles(pkg, streams, kind, op):
    stream, other = streams
    su = _setup(pkg)
    x_w, x_a, x_b = (su["iq_w"], su["iq"], su["iq_b"]) if kind == "scan" else _centred(pkg)
    d_a, d_b = _cuda(x_a), _cuda(x_b)
    make = dict(stereo=_stereo, rds=_rds, scan=_scan)[kind]

    def script(pkg, stream, held):
        kept = {}
        with make(pkg, su) as dm:
            if held:
                dm.set_stream(stream.cuda_stream)
            w = dm.process_batch(x_w)
            kept["w"] = [np.ascontiguousarray(v).tobytes() for v in (w if isinstance(w, tuple) else (w,))]
            n = dm.audio_count(NBYTES) if kind == "stereo" else dm.count(NBYTES) if kind == "rds" else 0
            oa, ob = _outputs(kind, n), _outputs(kind, n)
            call_a = lambda: dm.process_batch_device(d_a, *oa)
            sc = Script(stream, call_a, kind + " handle") if held else Plain(dm, call_a)
            if op == "reset":
                sc.waits(dm.reset, "reset")
            elif op == "tune":
                sc.waits(lambda: dm.tune(ctaps=su["ctaps2"], rot=su["rot2"]), "tune")
            if op == "set_stream" and held:
                sc.waits(lambda: dm.set_stream(other.cuda_stream), "set_stream")
                dm.process_batch_device(d_b, *ob)
                eC = sh.record(other)
                dm.set_stream(stream.cuda_stream)
                assert not sh.pending(eC), "set_stream back did not wait for call C on the stream it left"
            else:
                dm.process_batch_device(d_b, *ob)
            dm.synchronize()
            kept["a"], kept["b"] = [t.cpu().numpy().tobytes() for t in oa], [t.cpu().numpy().tobytes() for t in ob]
            if kind != "scan":                                    # the centred stations are received: a pilot on every stream
                assert (oa[-1].cpu().numpy() > 0).all() and (ob[-1].cpu().numpy() > 0).all(), "no pilot: the rows say nothing"
        return {k: repr(v) for k, v in kept.items()}

    _play(pkg, script, stream)
