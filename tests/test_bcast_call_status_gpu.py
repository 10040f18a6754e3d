"""GPU test of the status of every refusal of the broadcast receiver's three call entries (sdrfm_bcast_process_batch, _pcm and _metered,
the last without and with a sink), on host buffers and with SDRFM_F_DEVICE_PTRS, on an untuned handle and on one tuned with
SDRFM_TUNE_SHARED_INPUT: every single defect of DEFECTS and every pair of them, against tests/golden/bcast_call_status.json — the statuses
recorded from the library as it was before the entries were given one call path.  The pairs pin the order of the checks.

The handle is the smallest with every count non-zero: 2 streams, T 8, D 2, P 3, Ta 4, Da 2, Tr 4, Dr 3, 256 bytes a call at the most; a call
of 96 bytes gives 24 d's, 12 audio outputs and 8 RDS outputs.  In a row every pointer that is not the row's defect is real memory of the
row's kind, sized for the call, so the rows the library accepts are calls the header allows and nothing is launched on a pointer the
library neither owns nor checked.  The accepted rows, from reading the checks: no defect; nbytes = 0 beside anything the empty call does not
look at (iq, rows, bb, strides; pcm of a sink form, whose checks are skipped for no outputs); a short iq_stride on the shared-input handle,
which ignores it; both rows NULL in a sink form (the sink reads the handle's own rows), beside a short audio_stride, which nothing then
reads; NULL sink and NULL pcm together in the metered entry, which is its plain form.  The handle and the sink are reset after an accepted
row; after the whole table one valid call gives bit for bit what it gives on a fresh handle and sink: the refusals changed nothing."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import tuned_cases as tc

pytestmark = pytest.mark.gpu

SHAPE = (8, 2, 3, 4, 2, 4, 3)                                   # (T, D, P, Ta, Da, Tr, Dr)
NS, CAPACITY, NBYTES, AA, AR = 2, 256, 96, 12, 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bcast_call_status.json")
ENTRIES = ("process_batch", "process_batch_pcm", "process_batch_metered", "process_batch_metered+sink")
SINK = ENTRIES[1::2]                                            # the entries that want a sink
METERED = ENTRIES[2:]
FORMS = ("host", "device")
HANDLES = ("untuned", "shared")
F_DEVICE_PTRS, F_OVERLAP, F_UNKNOWN = 1, 2, 0x80


def _set(**kw):
    return lambda a: a.update(kw)


def _flag(bit):
    return lambda a: a.update(flags=a["flags"] | bit)


# (name, the entries it applies to, what it does to a call's arguments); a pair is both, in this order.  An argument that is a pointer
# holds the name of its buffer, None, or (name, byte offset)
DEFECTS = [
    ("null n_audio", ENTRIES, _set(n_audio=None)),
    ("null n_rds", ENTRIES, _set(n_rds=None)),
    ("unknown flag", ENTRIES, _flag(F_UNKNOWN)),
    ("SDRFM_F_OVERLAP", ENTRIES, _flag(F_OVERLAP)),
    ("odd nbytes", ENTRIES, lambda a: a.update(nbytes=a["nbytes"] | 1)),
    ("nbytes over capacity", ENTRIES, lambda a: a.update(nbytes=CAPACITY + 2 + (a["nbytes"] & 1))),
    ("nbytes = 0", ENTRIES, _set(nbytes=0)),
    ("null iq", ENTRIES, _set(iq=None)),
    ("short iq_stride", ENTRIES, _set(iq_stride=NBYTES - 1)),
    ("null left only", ENTRIES, _set(left=None)),
    ("null right only", ENTRIES, _set(right=None)),
    ("both rows null", ENTRIES, _set(left=None, right=None)),
    ("null bb", ENTRIES, _set(bb=None)),
    ("short audio_stride", ENTRIES, _set(audio_stride=AA - 1)),
    ("short bb_stride", ENTRIES, _set(bb_stride=2 * AR - 1)),
    ("null sink", SINK, _set(sink=None)),
    ("null pcm", SINK, _set(pcm=None)),
    ("short pcm_stride", SINK, _set(pcm_stride=2 * AA - 1)),
    ("pcm without sink", METERED[:1], _set(pcm="pcm")),
    ("null meters", METERED, _set(meters=None)),
    ("meters at 4 mod 8", METERED, _set(meters=("meters", 4))),
]
# two defects of one argument that cannot both hold
EXCLUSIVE = [{"nbytes = 0", "odd nbytes"}, {"nbytes = 0", "nbytes over capacity"}, {"null left only", "null right only"},
             {"null left only", "both rows null"}, {"null right only", "both rows null"}, {"null meters", "meters at 4 mod 8"}]


def rows(entry):
    """[(name, (defect, ...))] of an entry: no defect, every single one, every pair"""
    mine = [d for d in DEFECTS if entry in d[1]]
    pairs = [p for p in itertools.combinations(mine, 2) if {p[0][0], p[1][0]} not in EXCLUSIVE]
    return [("no defect", ())] + [(d[0], (d,)) for d in mine] + [("%s + %s" % (p[0][0], p[1][0]), p) for p in pairs]


def arguments(entry, form, defects):
    """the arguments of a row, pointers by name"""
    a = dict(sink="sink" if entry in SINK else None, iq="iq", iq_stride=NBYTES, nbytes=NBYTES, left="left", right="right", audio_stride=AA,
             pcm="pcm" if entry in SINK else None, pcm_stride=2 * AA if entry in SINK else 0, bb="bb", bb_stride=2 * AR, pilot_count="pilot_count",
             meters="meters" if entry in METERED else None, n_audio="n_audio", n_rds="n_rds", flags=F_DEVICE_PTRS if form == "device" else 0)
    for d in defects:
        d[2](a)
    return a


class _Buffers:
    """a call's buffers of one form, and the addresses of their names"""

    def __init__(self, pkg, form, sink):
        import torch
        rng = np.random.default_rng(20250)
        self.iq = rng.integers(0, 256, (NS, NBYTES), dtype=np.uint8)
        shapes = dict(iq=self.iq, left=np.zeros((NS, AA), np.float32), right=np.zeros((NS, AA), np.float32), pcm=np.zeros((NS, 2 * AA), np.int16),
                      bb=np.zeros((NS, 2 * AR), np.float32), pilot_count=np.zeros(NS, np.int32), meters=np.zeros((NS, 8), np.int64))
        self.keep = {k: (torch.from_numpy(v).cuda() if form == "device" else v.copy()) for k, v in shapes.items()}
        self.adr = {k: (v.data_ptr() if form == "device" else v.ctypes.data) for k, v in self.keep.items()}
        self.na, self.nr = C.c_uint32(), C.c_uint32()
        self.adr.update(sink=sink._h.value if hasattr(sink._h, "value") else sink._h, n_audio=C.addressof(self.na), n_rds=C.addressof(self.nr))
        assert self.adr["meters"] % 8 == 0 and self.adr["pcm"] % 4 == 0

    def of(self, v):
        if v is None or isinstance(v, int):
            return v
        return self.adr[v] if isinstance(v, str) else self.adr[v[0]] + v[1]


def call(lib, h, entry, a, buf):
    """the C call of a row: its status"""
    v = {k: buf.of(x) for k, x in a.items()}
    na, nr = C.cast(v["n_audio"], C.POINTER(C.c_uint32)), C.cast(v["n_rds"], C.POINTER(C.c_uint32))
    front = (v["iq"], v["iq_stride"], v["nbytes"], v["left"], v["right"], v["audio_stride"])
    if entry == "process_batch":
        return lib.sdrfm_bcast_process_batch(h, *front, v["bb"], v["bb_stride"], v["pilot_count"], na, nr, v["flags"])
    back = (v["pcm"], v["pcm_stride"], v["bb"], v["bb_stride"], v["pilot_count"])
    if entry == "process_batch_pcm":
        return lib.sdrfm_bcast_process_batch_pcm(h, v["sink"], *front, *back, na, nr, v["flags"])
    return lib.sdrfm_bcast_process_batch_metered(h, v["sink"], *front, *back, v["meters"], na, nr, v["flags"])


def make_handles(pkg, kind):
    """(BroadcastDemod of SHAPE, untuned or tuned with SDRFM_TUNE_SHARED_INPUT; a StereoPcmSink of its streams)"""
    T, D, P, Ta, Da, Tr, Dr = SHAPE
    h, ga, gr, b, dg, rg = tc.shape_taps(pkg, SHAPE)
    bc = pkg.BroadcastDemod(pkg.BroadcastConfig(fir_coeffs=h, audio_coeffs=ga, rds_coeffs=gr, pilot_coeffs=b, diff_gain=dg, rds_gain=rg, fir_decim=D,
                                                audio_decim=Da, rds_decim=Dr, n_streams=NS, max_bytes_per_call=CAPACITY))
    if kind == "shared":
        bc.tune(offsets_hz=[0.0, 100e3], shared_input=True)
    assert bc.counts(NBYTES) == (AA, AR)
    return bc, pkg.StereoPcmSink(NS, 0.25, 1000.0)


def run_table(pkg, bc, sink, form):
    """{entry: [status of every row of rows(entry)]} on one handle; the handle and the sink are reset after an accepted row"""
    lib, buf, out = pkg.load_library(), _Buffers(pkg, form, sink), {}
    for entry in ENTRIES:
        out[entry] = []
        for name, defects in rows(entry):
            st = call(lib, bc._h, entry, arguments(entry, form, defects), buf)
            out[entry].append(int(st))
            if st == pkg.lib.OK:
                bc.synchronize()
                bc.reset()
                sink.reset()
    return out


def _valid_call(pkg, bc, sink, buf, shared):
    out = bc.process_batch_pcm(sink, buf.iq[:1] if shared else buf.iq)
    return [np.ascontiguousarray(x).view(np.uint8) for x in out]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", HANDLES)
def test_every_refusal_has_the_recorded_status_and_changes_nothing(pkg, kind, form):
    golden = json.load(open(GOLDEN))
    for entry in ENTRIES:
        assert golden["rows"][entry] == [n for n, _ in rows(entry)], entry
    bc, sink = make_handles(pkg, kind)
    fresh, fresh_sink = make_handles(pkg, kind)
    with bc, sink, fresh, fresh_sink:
        got = run_table(pkg, bc, sink, form)
        wrong = []
        for entry in ENTRIES:
            want = golden["status"][kind][form][entry]
            names = golden["rows"][entry]
            assert len(got[entry]) == len(want) == len(names)
            assert want[0] == pkg.lib.OK, (entry, want[0])
            wrong += [(entry, n, g, w) for n, g, w in zip(names, got[entry], want) if g != w]
        print("%s handle, %s buffers: %d rows, %d accepted, %d differ" % (kind, form, sum(len(v) for v in got.values()),
                                                                         sum(v.count(0) for v in got.values()), len(wrong)))
        assert not wrong, wrong[:20]
        buf = _Buffers(pkg, "host", sink)
        a, b = _valid_call(pkg, bc, sink, buf, kind == "shared"), _valid_call(pkg, fresh, fresh_sink, buf, kind == "shared")
        assert len(a) == len(b) == 5 and all(np.array_equal(x, y) for x, y in zip(a, b))
        assert a[0].size == NS * AA * 4 and a[3].size == NS * AR * 8 and np.any(a[0])
