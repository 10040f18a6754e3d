"""GPU test of the status of every refusal of the six PCM-side handles' call entries (the PCM sink, the stereo PCM sink, the rate matcher, the
limiter, the mix bus and the IQ meter), on host buffers and with SDRFM_F_DEVICE_PTRS: every single defect of an entry's DEFECTS and every pair
of them, against tests/golden/pcm_call_status.json — the statuses recorded from the library as it was before the handles' host plumbing
moved into csrc/sdrfm_host.h and csrc/sdrfm_pcm_rows.h.  The pairs pin the order of the checks: "stride one short" is both short and odd, so
the sinks answer ECAPACITY where the three newer handles answer EINVAL.

Every handle has 2 streams (the mix bus 2 rows in, 2 buses out) and a call has 8 pairs (the IQ meter: 8 byte-pairs of at most 64 bytes a
call).  In a row every pointer that is not the row's defect is real memory of the row's kind with a row of slack behind it, so a row the
library accepts is a legal call of a few pairs: no defect; n = 0 beside anything the empty call does not look at; an address at 2 mod 4 in
host memory, which only device rows must avoid; an odd audio stride of a sink, whose audio rows are floats; the IQ meter's rows at an odd
address and its call with the histogram, which are no defects at all and stand in the table for their pairs.  Nothing else is accepted: a
count over the handle's maximum, null rows, short strides and overlapping mix rows are refused before any device work, and the sinks, which
have no maximum, get no such row.  The handle is reset after an accepted row.  Beside the tables: the read-outs of the limiter, the mix
bus and the stereo sink's audio meter, every entry on a null handle, and kernel_name(NULL)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS, N, ROW = 2, 8, 32                                           # streams, pairs per call, int16 / float elements per buffer row
IQ_MAX, IQ_BYTES = 64, 16
N_MAX = 1 << 20                                                 # SDRFM_LIMIT_N_MAX = SDRFM_RATE_N_MAX = PMIX_N_MAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcm_call_status.json")
HANDLES = ("pcm_sink", "pcm_stereo_sink", "pcm_rate", "pcm_limit", "pcm_mix", "iq_meter")
FORMS = ("host", "device")
F_DEVICE_PTRS, F_UNKNOWN, F_RESET = 1, 0x80, 8


def _set(**kw):
    return lambda a: a.update(kw)


def _stride(which, by):
    """the stride the row needs (the default of arguments), moved by `by` elements"""
    return lambda a: a.update({which: a[which] + by})


# (name, what it does to a call's arguments); a pair is both, in this order.  A pointer argument holds the name of its buffer, None, or
# (name, byte offset)
_LR = [
    ("unknown flag", lambda a: a.update(flags=a["flags"] | F_UNKNOWN)),
    ("n = N_MAX + 1", _set(n=N_MAX + 1)),
    ("odd in_stride", _stride("in_stride", +1)),
    ("odd out_stride", _stride("out_stride", +1)),
    ("n = 0", _set(n=0)),
    ("null rows", _set(inp=None, out=None)),
    ("null in only", _set(inp=None)),
    ("null out only", _set(out=None)),
    ("in at 2 mod 4", _set(inp=("inp", 2))),
    ("out at 2 mod 4", _set(out=("out", 2))),
    ("in_stride one short", _stride("in_stride", -1)),
    ("out_stride one short", _stride("out_stride", -1)),
    ("in_stride one pair short", _stride("in_stride", -2)),
    ("out_stride one pair short", _stride("out_stride", -2)),
]
_SINK = [
    ("unknown flag", lambda a: a.update(flags=a["flags"] | F_UNKNOWN)),
    ("n = 0", _set(n=0)),
    ("null rows", _set(inp=None, inp2=None, out=None)),
    ("null audio only", _set(inp=None, inp2=None)),
    ("null pcm only", _set(out=None)),
    ("odd audio_stride", _stride("in_stride", +1)),
    ("odd pcm_stride", _stride("out_stride", +1)),
    ("pcm at 2 mod 4", _set(out=("out", 2))),
    ("audio_stride one short", _stride("in_stride", -1)),
    ("pcm_stride one short", _stride("out_stride", -1)),
    ("pcm_stride one pair short", _stride("out_stride", -2)),
]
DEFECTS = {
    "pcm_sink": _SINK,
    "pcm_stereo_sink": _SINK + [("null left only", _set(inp=None)), ("null right only", _set(inp2=None))],
    "pcm_rate": _LR,
    "pcm_limit": _LR,
    "pcm_mix": _LR + [("out = in", _set(out="inp")), ("out one pair into in", _set(out=("inp", 4)))],
    "iq_meter": [
        ("unknown flag", lambda a: a.update(flags=a["flags"] | F_UNKNOWN)),
        ("null meters", _set(meters=None)),
        ("meters at 4 mod 8", _set(meters=("meters", 4))),
        ("hist at 2 mod 4", _set(hist=("hist", 2))),
        ("with hist", _set(hist="hist")),
        ("odd nbytes", _set(n=IQ_BYTES + 1)),
        ("nbytes over the maximum", _set(n=IQ_MAX + 2)),
        ("nbytes = 0", _set(n=0)),
        ("null iq", _set(inp=None)),
        ("iq at an odd address", _set(inp=("iq", 1))),
        ("iq_stride one short", _stride("in_stride", -1)),
    ],
}
# two defects of one argument that cannot both hold
EXCLUSIVE = [{"n = N_MAX + 1", "n = 0"}, {"odd in_stride", "in_stride one short"}, {"odd in_stride", "in_stride one pair short"},
             {"odd out_stride", "out_stride one short"}, {"odd out_stride", "out_stride one pair short"},
             {"in_stride one short", "in_stride one pair short"}, {"out_stride one short", "out_stride one pair short"},
             {"null rows", "null in only"}, {"null rows", "null out only"}, {"null in only", "in at 2 mod 4"}, {"null out only", "out at 2 mod 4"},
             {"null rows", "in at 2 mod 4"}, {"null rows", "out at 2 mod 4"}, {"null in only", "null out only"},
             {"null rows", "null audio only"}, {"null rows", "null pcm only"}, {"null audio only", "null pcm only"}, {"null rows", "pcm at 2 mod 4"},
             {"null pcm only", "pcm at 2 mod 4"}, {"odd audio_stride", "audio_stride one short"}, {"odd pcm_stride", "pcm_stride one short"},
             {"odd pcm_stride", "pcm_stride one pair short"}, {"pcm_stride one short", "pcm_stride one pair short"},
             {"null rows", "null left only"}, {"null rows", "null right only"}, {"null audio only", "null left only"},
             {"null audio only", "null right only"}, {"null left only", "null right only"},
             {"out = in", "out one pair into in"}, {"out = in", "null rows"}, {"out = in", "null out only"}, {"out = in", "out at 2 mod 4"},
             {"out one pair into in", "null rows"}, {"out one pair into in", "null out only"}, {"out one pair into in", "out at 2 mod 4"},
             {"null meters", "meters at 4 mod 8"}, {"hist at 2 mod 4", "with hist"}, {"odd nbytes", "nbytes over the maximum"},
             {"odd nbytes", "nbytes = 0"}, {"nbytes over the maximum", "nbytes = 0"}, {"null iq", "iq at an odd address"}]


def rows(handle):
    """[(name, (defect, ...))] of a handle's call entry: no defect, every single one, every pair"""
    mine = DEFECTS[handle]
    pairs = [p for p in itertools.combinations(mine, 2) if {p[0][0], p[1][0]} not in EXCLUSIVE]
    return [("no defect", ())] + [(d[0], (d,)) for d in mine] + [("%s + %s" % (p[0][0], p[1][0]), p) for p in pairs]


def arguments(handle, form, defects, out_stride):
    """the arguments of a row, pointers by name"""
    flags = F_DEVICE_PTRS if form == "device" else 0
    if handle == "iq_meter":
        a = dict(inp="iq", in_stride=IQ_BYTES, n=IQ_BYTES, meters="meters", hist=None, flags=flags)
    elif handle in ("pcm_sink", "pcm_stereo_sink"):
        a = dict(inp="left", inp2="right", in_stride=N, n=N, out="out", out_stride=2 * N, flags=flags)
    else:
        a = dict(inp="inp", in_stride=2 * N, n=N, out="out", out_stride=out_stride, flags=flags)
    for d in defects:
        d[1](a)
    return a


class _Buffers:
    """a call's buffers of one form, each with a row of slack, and the addresses of their names"""

    def __init__(self, form):
        rng = np.random.default_rng(20251)
        shapes = dict(inp=rng.integers(-20000, 20000, (NS + 1, ROW)).astype(np.int16), out=np.zeros((NS + 1, ROW), np.int16),
                      left=rng.standard_normal((NS + 1, ROW)).astype(np.float32), right=rng.standard_normal((NS + 1, ROW)).astype(np.float32),
                      iq=rng.integers(0, 256, (NS + 1, IQ_MAX + 8), dtype=np.uint8), meters=np.zeros((NS + 1, 8), np.int64),
                      hist=np.zeros((NS + 1, 512), np.int32), rec=np.zeros((NS + 1, 24), np.int64))
        if form == "device":
            import torch
            self.keep = {k: torch.from_numpy(v).cuda() for k, v in shapes.items()}
            torch.cuda.synchronize()
            self.adr = {k: v.data_ptr() for k, v in self.keep.items()}
        else:
            self.keep = {k: v.copy() for k, v in shapes.items()}
            self.adr = {k: v.ctypes.data for k, v in self.keep.items()}
        self.cnt = np.zeros(NS, np.uint32)
        assert all(self.adr[k] % 8 == 0 for k in self.adr)

    def of(self, v):
        if v is None or isinstance(v, int):
            return v
        return self.adr[v] if isinstance(v, str) else self.adr[v[0]] + v[1]


def make_handle(pkg, handle):
    if handle == "pcm_sink":
        return pkg.PcmSink(NS, 0.25, 1000.0)
    if handle == "pcm_stereo_sink":
        return pkg.StereoPcmSink(NS, 0.25, 1000.0)
    if handle == "pcm_rate":
        return pkg.PcmRateMatcher(NS, pkg.rate_coef())
    if handle == "pcm_limit":
        return pkg.PcmLimiter(NS, 6, 8)
    if handle == "pcm_mix":
        return pkg.PcmMixer(NS, NS, 2, slew=32)
    return pkg.IqMeter(NS, IQ_MAX)


def call(lib, handle, h, a, buf):
    """the C call of a row: its status"""
    v = {k: buf.of(x) for k, x in a.items()}
    if handle == "pcm_sink":
        return lib.sdrfm_pcm_sink_process_batch(h, v["inp"], v["in_stride"], v["n"], v["out"], v["out_stride"], v["flags"])
    if handle == "pcm_stereo_sink":
        return lib.sdrfm_pcm_stereo_sink_process_batch(h, v["inp"], v["inp2"], v["in_stride"], v["n"], v["out"], v["out_stride"], v["flags"])
    if handle == "pcm_rate":
        return lib.sdrfm_pcm_rate_process_batch(h, v["inp"], v["in_stride"], v["n"], v["out"], v["out_stride"], buf.cnt.ctypes.data, v["flags"])
    if handle == "pcm_limit":
        return lib.sdrfm_pcm_limit_process_batch(h, v["inp"], v["in_stride"], v["n"], v["out"], v["out_stride"], v["flags"])
    if handle == "pcm_mix":
        return lib.sdrfm_pcm_mix_process_batch(h, v["inp"], v["in_stride"], v["n"], v["out"], v["out_stride"], v["flags"])
    return lib.sdrfm_iq_meter_process_batch(h, v["inp"], v["in_stride"], v["n"], v["meters"], v["hist"], v["flags"])


def run_table(pkg, handle, form):
    """[status of every row of rows(handle)] on one handle; the handle is reset after an accepted row"""
    lib, buf, out = pkg.load_library(), _Buffers(form), []
    with make_handle(pkg, handle) as k:
        out_stride = 2 * N
        if handle == "pcm_rate":                                # the rate matcher's need is its largest count's
            out_stride = 2 * k.count(N)[1]
            assert 2 <= out_stride <= 2 * N + 2, out_stride
        for name, defects in rows(handle):
            a = arguments(handle, form, defects, out_stride)
            st = int(call(lib, handle, k._h, a, buf))
            out.append(st)
            if st == pkg.lib.OK:
                k.synchronize()
                if hasattr(k, "reset"):
                    k.reset()
    return out


READS = ("no defect", "reset", "null out", "unknown flag", "out at 4 mod 8", "unknown flag + null out", "null out + reset")


def run_reads(pkg, form):
    """{entry: [status of every row of READS]}: the read-outs that share their flag logic"""
    lib, buf = pkg.load_library(), _Buffers(form)
    f0 = F_DEVICE_PTRS if form == "device" else 0
    rec = buf.adr["rec"]
    args = [(rec, f0), (rec, f0 | F_RESET), (None, f0), (rec, f0 | F_UNKNOWN), (rec + 4, f0), (None, f0 | F_UNKNOWN), (None, f0 | F_RESET)]
    out = {}
    with pkg.PcmLimiter(NS, 6, 8) as lm, pkg.PcmMixer(NS, NS, 2) as mx, pkg.StereoPcmSink(NS, 0.25, 1000.0) as sk:
        out["pcm_limit_read"] = [int(lib.sdrfm_pcm_limit_read(lm._h, p, f)) for p, f in args]
        lm.synchronize()
        out["pcm_mix_read"] = [int(lib.sdrfm_pcm_mix_read(mx._h, p, f)) for p, f in args]
        mx.synchronize()
        out["pcm_stereo_sink_meter_read, meter off"] = [int(lib.sdrfm_pcm_stereo_sink_meter_read(sk._h, p, f)) for p, f in args]
        sk.enable_meter(0)
        out["pcm_stereo_sink_meter_read"] = [int(lib.sdrfm_pcm_stereo_sink_meter_read(sk._h, p, f)) for p, f in args]
        sk.synchronize()
    return out


# every entry of the six handles that takes the handle first, called on a null handle with its other arguments zero
NULL_HANDLE = [(h + e) for h, es in (
    ("sdrfm_pcm_sink", ("_reset", "_set_stream", "_synchronize", "_process_batch", "_get_state")),
    ("sdrfm_pcm_stereo_sink", ("_reset", "_set_stream", "_synchronize", "_process_batch", "_get_state", "_meter_read")),
    ("sdrfm_pcm_rate", ("_reset", "_set_stream", "_synchronize", "_process_batch", "_get_state", "_set_step")),
    ("sdrfm_pcm_limit", ("_reset", "_set_stream", "_synchronize", "_process_batch", "_get_state", "_read")),
    ("sdrfm_pcm_mix", ("_reset", "_set_stream", "_synchronize", "_process_batch", "_read")),
    ("sdrfm_iq_meter", ("_set_stream", "_synchronize", "_process_batch"))) for e in es]
KERNEL_NAMES = ("sdrfm_pcm_rate_kernel_name", "sdrfm_pcm_limit_kernel_name", "sdrfm_pcm_mix_kernel_name", "sdrfm_iq_meter_kernel_name")


def run_null(pkg):
    """({entry: status on a null handle}, {kernel_name entry: what it answers for NULL, None for a null pointer})"""
    lib = pkg.load_library()
    st = {}
    for name in NULL_HANDLE:
        f = getattr(lib, name)
        st[name] = int(f(None, *([None if t is C.c_void_p or hasattr(t, "contents") else 0 for t in f.argtypes[1:]])))
    names = {}
    for name in KERNEL_NAMES:
        s = getattr(lib, name)(None)
        names[name] = None if s is None else s.decode()
    return st, names


def record(pkg):
    """the whole table as the fixture holds it"""
    st, names = run_null(pkg)
    return {"n_streams": NS, "n": N, "iq_max_bytes": IQ_MAX,
            "status_names": {"0": "SDRFM_OK", "16": "SDRFM_EINVAL", "17": "SDRFM_EODD", "18": "SDRFM_ECAPACITY"},
            "rows": {h: [n for n, _ in rows(h)] for h in HANDLES},
            "status": {form: {h: run_table(pkg, h, form) for h in HANDLES} for form in FORMS},
            "read_rows": list(READS), "reads": {form: run_reads(pkg, form) for form in FORMS},
            "null_handle": st, "kernel_name_null": names}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("handle", HANDLES)
def test_every_call_has_the_recorded_status(pkg, golden, handle, form):
    assert (golden["n_streams"], golden["n"], golden["iq_max_bytes"]) == (NS, N, IQ_MAX)
    names = [n for n, _ in rows(handle)]
    assert golden["rows"][handle] == names
    want = golden["status"][form][handle]
    got = run_table(pkg, handle, form)
    assert len(got) == len(want) == len(names) and want[0] == pkg.lib.OK
    wrong = [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    print("%s, %s buffers: %d rows, %d accepted, %d differ" % (handle, form, len(got), got.count(0), len(wrong)))
    assert not wrong, wrong[:20]


def test_the_sinks_answer_capacity_before_the_odd_stride_and_the_newer_handles_after(golden):
    """the two-faults-at-once row, a stride that is both short and odd, as the fixture holds it: the order of the checks is each handle's"""
    for form in FORMS:
        for h in ("pcm_sink", "pcm_stereo_sink"):
            assert golden["status"][form][h][golden["rows"][h].index("pcm_stride one short")] == 18, (form, h)
        for h in ("pcm_rate", "pcm_limit", "pcm_mix"):
            assert golden["status"][form][h][golden["rows"][h].index("out_stride one short")] == 16, (form, h)
            assert golden["status"][form][h][golden["rows"][h].index("out_stride one pair short")] == 18, (form, h)


@pytest.mark.parametrize("form", FORMS)
def test_every_read_out_has_the_recorded_status(pkg, golden, form):
    assert golden["read_rows"] == list(READS)
    got = run_reads(pkg, form)
    assert got == golden["reads"][form], (got, golden["reads"][form])


def test_a_null_handle_and_kernel_name_of_null_answer_as_recorded(pkg, golden):
    st, names = run_null(pkg)
    assert sorted(st) == sorted(NULL_HANDLE) and st == golden["null_handle"], (st, golden["null_handle"])
    assert names == golden["kernel_name_null"], (names, golden["kernel_name_null"])
    assert names["sdrfm_iq_meter_kernel_name"] == "" and names["sdrfm_pcm_mix_kernel_name"] is None    # unlike the other handles: the IQ meter answers ""
