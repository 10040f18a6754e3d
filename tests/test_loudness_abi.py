"""The loudness meter's ABI (include/sdrfm.h): the symbols, the struct layouts in the header, in ctypes and in numpy, and the
refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sdrfm_loudness_default_coef", "sdrfm_loudness_check_coef", "sdrfm_loudness_check_domain", "sdrfm_pcm_loudness_s16", "sdrfm_loudness_gate_create", "sdrfm_loudness_gate_push",
           "sdrfm_loudness_gate_report", "sdrfm_loudness_gate_reset", "sdrfm_loudness_gate_free", "sdrfm_pcm_stereo_sink_loudness_enable",
           "sdrfm_pcm_stereo_sink_loudness_disable", "sdrfm_pcm_stereo_sink_loudness_read", "sdrfm_pcm_stereo_sink_loudness_get_state"]


def test_symbols_and_exports(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    for sym in SYMBOLS:
        assert sym in pkg.ABI_SYMBOLS and getattr(lib, sym) is not None and re.search(r"\b%s\(" % sym, header), sym
    for name in ("LOUDNESS_STATE_DTYPE", "loudness_default_coef", "pcm_loudness_host", "LoudnessGate", "LoudnessMonitor", "loudness_alarms"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    for m in ("enable_loudness", "disable_loudness", "read_loudness"):
        assert hasattr(pkg.StereoPcmSink, m), m


def test_struct_layouts_in_header_ctypes_and_numpy(pkg):
    l = pkg.lib
    header = open(os.path.join(ROOT, "include", "sdrfm.h")).read()
    assert "typedef struct sdrfm_loudness_coef { double c[10]; } sdrfm_loudness_coef;" in header
    assert "typedef struct sdrfm_loudness_state { uint64_t pos; double z[2][4]; double e[2]; } sdrfm_loudness_state;" in header
    assert "typedef struct sdrfm_loudness_block { double e_l, e_r; } sdrfm_loudness_block;" in header
    assert C.sizeof(l.LoudnessCoef) == 80 and C.sizeof(l.LoudnessState) == 88 and C.sizeof(l.LoudnessBlock) == 16 and C.sizeof(l.LoudnessReport) == 104
    assert (l.LoudnessState.pos.offset, l.LoudnessState.z.offset, l.LoudnessState.e.offset) == (0, 8, 72)
    d = pkg.LOUDNESS_STATE_DTYPE
    assert d.itemsize == 88 and [d.fields[n][1] for n in ("pos", "z", "e")] == [0, 8, 72] and d["z"].shape == (2, 4)
    assert l.LOUDNESS_BLOCK_DTYPE.itemsize == 16
    rep = re.search(r"typedef struct sdrfm_loudness_report_t \{(.*?)\}", header, re.S).group(1)
    names = [n.strip() for part in re.findall(r"(?:double|uint64_t)\s+([^;]+);", rep) for n in part.split(",")]
    assert names == [n for n, _ in l.LoudnessReport._fields_]


def test_coefficients_and_their_check(pkg):
    lib = pkg.load_library()
    c = pkg.loudness_default_coef()
    assert c.tolist() == [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                          1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert lib.sdrfm_loudness_check_coef(c.ctypes.data) == 0 and lib.sdrfm_loudness_check_coef(None) == pkg.lib.EINVAL
    assert lib.sdrfm_loudness_default_coef(None) == pkg.lib.EINVAL
    for k, v in [(0, np.nan), (7, np.inf), (4, 1.0), (4, -1.0), (9, 1.5), (3, 1.0 + c[4]), (3, -(1.0 + c[4])), (8, -2.0)]:
        bad = c.copy()
        bad[k] = v
        assert lib.sdrfm_loudness_check_coef(bad.ctypes.data) == pkg.lib.EINVAL, (k, v)
    edge = c.copy()
    edge[3] = np.nextafter(1.0 + c[4], 0.0)
    assert lib.sdrfm_loudness_check_coef(edge.ctypes.data) == 0


def test_the_device_domain_is_refused_without_a_device(pkg):
    """sdrfm_loudness_check_domain is what _loudness_enable asks before any device work: a stable set outside the domain answers SDRFM_EINVAL,
    with the two figures that say why; sdrfm_loudness_check_coef and the host routine go on accepting it"""
    import loudness_cases as lc
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    sets = lc.coef_sets()
    rel, ab = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.sdrfm_loudness_check_domain(None, C.byref(rel), C.byref(ab)) == E and (rel.value, ab.value) == (-1.0, -1.0)
    unstable = pkg.loudness_default_coef()
    unstable[9] = 1.0
    assert lib.sdrfm_loudness_check_domain(unstable.ctypes.data, C.byref(rel), C.byref(ab)) == E and (rel.value, ab.value) == (-1.0, -1.0)
    c = pkg.loudness_default_coef()
    assert lib.sdrfm_loudness_check_domain(c.ctypes.data, None, None) == 0
    assert lib.sdrfm_loudness_check_domain(c.ctypes.data, C.byref(rel), C.byref(ab)) == 0
    assert 0.0 < rel.value <= lc.MEASURED_REL and 0.0 < ab.value <= lc.MEASURED_ABS          # the default's figures peak on the probe's own DC rows
    pcm = lc.interleave(*lc.random_rows(300, 1))
    for name in ("k192000", "hp r=0.99 th=pi-1e-3", "hp r=0.999 th=1e-3", "shelf r=0.999 th=0.01"):
        bad = sets[name]
        assert lib.sdrfm_loudness_check_coef(bad.ctypes.data) == 0, name
        assert lib.sdrfm_loudness_check_domain(bad.ctypes.data, C.byref(rel), C.byref(ab)) == E, name
        assert rel.value > 1e-9 / 16 or ab.value > 1e-3 / 16, (name, rel.value, ab.value)
        assert lib.sdrfm_pcm_stereo_sink_loudness_enable(None, bad.ctypes.data, 4800, 64) == E
        assert pkg.pcm_loudness_host(pcm, 64, bad)[0].shape == (1, 4, 2), name               # exact by definition: the host routine serves it


def test_host_routine_refusals_change_nothing(pkg):
    lib, E, CAP = pkg.load_library(), pkg.lib.EINVAL, pkg.lib.ECAPACITY
    c = pkg.loudness_default_coef()
    pcm = np.arange(-300, 300, dtype=np.int16)                                               # 300 pairs
    st = np.zeros(1, pkg.LOUDNESS_STATE_DTYPE)
    out = np.full((8, 2), -1.0)
    nb = C.c_uint32(77)
    call = lambda p, n, co, bl, s, o, cap, q: lib.sdrfm_pcm_loudness_s16(p, n, co, bl, s, o, cap, q)
    args = (pcm.ctypes.data, 300, c.ctypes.data, 64, st.ctypes.data, out.ctypes.data, 8, C.byref(nb))
    for k, v in [(0, None), (2, None), (4, None), (7, None), (3, 63), (3, (1 << 20) + 1), (3, 0)]:
        bad = list(args)
        bad[k] = v
        assert call(*bad) == E, k
    nan = c.copy()
    nan[2] = np.nan
    assert call(*(args[:2] + (nan.ctypes.data,) + args[3:])) == E
    assert call(*(args[:6] + (3,) + args[7:])) == CAP                                        # 300 pairs complete 4 sub-blocks of 64
    assert call(*(args[:5] + (None,) + args[6:])) == E
    assert st.tobytes() == bytes(88) and (out == -1.0).all() and nb.value == 77              # nothing changed
    assert call(*args) == 0 and nb.value == 4 and int(st["pos"][0]) == 300 and (out[:4] > 0).all() and (out[4:] == -1.0).all()
    assert call(None, 0, c.ctypes.data, 64, st.ctypes.data, None, 0, C.byref(nb)) == 0 and nb.value == 0   # no pairs, no sub-block: no buffers
    assert call(pcm.ctypes.data, 19, c.ctypes.data, 64, st.ctypes.data, None, 0, C.byref(nb)) == 0 and nb.value == 0 and int(st["pos"][0]) == 319
    assert call(pcm.ctypes.data, 1, c.ctypes.data, 64, st.ctypes.data, None, 0, C.byref(nb)) == CAP and int(st["pos"][0]) == 319


def test_gate_refusals(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    h = C.c_void_p()
    assert lib.sdrfm_loudness_gate_create(4800, None) == E
    for bl in (0, 63, (1 << 20) + 1):
        assert lib.sdrfm_loudness_gate_create(bl, C.byref(h)) == E and not h.value
    assert lib.sdrfm_loudness_gate_create(64, C.byref(h)) == 0 and h.value
    rep = pkg.lib.LoudnessReport()
    good = np.ones((5, 2))
    assert lib.sdrfm_loudness_gate_push(None, good.ctypes.data, 5) == E and lib.sdrfm_loudness_gate_push(h, None, 5) == E
    assert lib.sdrfm_loudness_gate_report(None, C.byref(rep)) == E and lib.sdrfm_loudness_gate_report(h, None) == E
    assert lib.sdrfm_loudness_gate_reset(None) == E
    for v in (-1.0, np.nan, np.inf):
        bad = good.copy()
        bad[4, 1] = v
        assert lib.sdrfm_loudness_gate_push(h, bad.ctypes.data, 5) == E
    assert lib.sdrfm_loudness_gate_report(h, C.byref(rep)) == 0 and rep.n_blocks == 0       # a refused push takes nothing
    assert lib.sdrfm_loudness_gate_push(h, None, 0) == 0 and lib.sdrfm_loudness_gate_push(h, good.ctypes.data, 5) == 0
    assert lib.sdrfm_loudness_gate_report(h, C.byref(rep)) == 0 and rep.n_blocks == 5 and rep.n_gating == 2
    assert lib.sdrfm_loudness_gate_reset(h) == 0 and lib.sdrfm_loudness_gate_report(h, C.byref(rep)) == 0 and rep.n_blocks == 0
    lib.sdrfm_loudness_gate_free(h)
    lib.sdrfm_loudness_gate_free(None)


def test_sink_entry_points_refuse_a_null_sink(pkg):
    lib, E = pkg.load_library(), pkg.lib.EINVAL
    first, nb = C.c_uint64(), C.c_uint32()
    out = np.zeros(4)
    assert lib.sdrfm_pcm_stereo_sink_loudness_enable(None, None, 4800, 64) == E
    assert lib.sdrfm_pcm_stereo_sink_loudness_disable(None) == E
    assert lib.sdrfm_pcm_stereo_sink_loudness_read(None, out.ctypes.data, 2, C.byref(first), C.byref(nb), 0) == E
    assert lib.sdrfm_pcm_stereo_sink_loudness_get_state(None, out.ctypes.data) == E
