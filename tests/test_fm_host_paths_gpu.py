"""The FM handle's host-buffer paths and its ring against each other and against the oracle: every ladder of tests/fm_host_cases.py (one stream, call sizes
built from the rules of csrc/sdrfm_fm_call.h; pre-checked on the CPU by tests/test_fm_host_cases_cpu.py) fed, cut the same way, through a default handle
(mapped rows up to 65 536 bytes), a SDRFM_CFG_NO_ZEROCOPY handle (staged rows) and a ring of 3 slots.  All three end in the same enqueue() with rows whose
pointer and stride are multiples of 16 bytes, and every kernel but design Q is bit-identical to the definition — design Q's calls are whole multiples of
16 bytes on every path —, so the audio of every call is the same bits on the three paths, served by the same kernel, and the concatenation is the oracle's
at the project's tolerance.  Behind the sweep: refused calls that must change nothing, and host batches with padded rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import fm_host_cases as hc
import fm_ring_util as ru
from conftest import scaled_err, TOL

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _taps(pkg, g):
    if hc.names_words(g):
        return pkg.default_config(g.T, fir_decim=g.D, audio_taps=g.Ta, audio_decim=g.Da)
    rng = np.random.default_rng(g.T + g.D)                        # (audio taps of unit absolute sum: the plain tolerance applies)
    h = (rng.standard_normal(g.T) / np.sqrt(g.T)).astype(np.float32)
    a = rng.standard_normal(g.Ta)
    return h, (a / np.abs(a).sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _iq(pkg, mode, nsamp):
    iq = pkg.make_iq(1, nsamp, mode=mode, first_id=4100 + nsamp % 97)[0]
    iq.setflags(write=False)
    return iq


def _handle(pkg, g, flags, max_bytes, **kw):
    h, a = _taps(pkg, g)
    return pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=a, fir_decim=g.D, audio_decim=g.Da, max_bytes_per_call=max_bytes,
                                    bit_exact=flags == "bit_exact", force_generic=flags == "force_generic", **kw))


def _chunks(iq, sizes):
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [iq[cuts[i]:cuts[i + 1]] for i in range(len(sizes))]


def _direct(dm, chunks):
    """sdrfm_process call by call: (audio per call, kernel_name after each call, sdrfm_audio_count's answer right before it)"""
    outs, names, counts = [], [], []
    for chunk in chunks:
        counts.append(dm.audio_count(len(chunk)))
        outs.append(dm.process(chunk).copy())
        names.append(dm.kernel_name)
    return outs, names, counts


@pytest.mark.parametrize("case", hc.all_cases(), ids=lambda c: c.name)
def test_three_paths_give_the_same_bits_from_the_same_kernel(pkg, oracle_mod, case):
    g, lib = case.geom, pkg.load_library()
    sizes = [k.nbytes for k in case.calls]
    iq = _iq(pkg, case.mode, sum(sizes) // 2)
    chunks = _chunks(iq, sizes)
    slot = hc.slot_bytes(case)
    runs = {}
    for path in ("mapped", "staged", "ring"):
        dm = _handle(pkg, g, case.flags, slot, no_zerocopy=path == "staged")
        first_name = dm.kernel_name
        if path == "ring":
            ring = ru.Ring(lib, dm, hc.n_slots(case), slot)
            outs, busy, names, counts = ru.feed(ring, chunks)
            if case.ladder == "q":                                # (two calls in two slots: a submit to the full ring is made on purpose, and consumes nothing)
                assert busy == 0
                assert ring.submit(chunks[0]) == ru.OK and ring.submit(chunks[1]) == ru.OK and ring.submit(chunks[1]) == ru.BUSY
                again = ring.drain()
                assert len(again) == 2
            else:
                assert busy > 0, "no submit met a full ring"
            ring.destroy()
        else:
            outs, names, counts = _direct(dm, chunks)
        dm.close()
        runs[path] = (outs, [first_name] + names, counts)

    # ---- count: every call gives what sdrfm_audio_count answered just before it, which is the oracle's count for that chunk
    h, a = _taps(pkg, g)
    orc = oracle_mod.Oracle(h, a, g.D, g.Da)
    want = [orc.process(chunk) if len(chunk) else np.zeros(0, np.float32) for chunk in chunks]
    for path, (outs, names, counts) in runs.items():
        assert [o.size for o in outs] == counts == [k.A for k in case.calls] == [w.size for w in want], (case.name, path)
    # ---- three-path bit equality, call by call
    for path in ("staged", "ring"):
        for i, (x, y) in enumerate(zip(runs["mapped"][0], runs[path][0])):
            assert np.array_equal(_bits(x), _bits(y)), (case.name, path, i, sizes[i], runs["mapped"][1][i + 1], runs[path][1][i + 1])
    # ---- kernel word: the same on the three paths, the table's where it names one; a 0-byte call leaves the name as it was
    words = []
    for i, k in enumerate(case.calls):
        per_path = [runs[p][1][i + 1] for p in ("mapped", "staged", "ring")]
        if k.N == 0:
            assert per_path == [runs[p][1][i] for p in ("mapped", "staged", "ring")], (case.name, i)
            words.append("-")
            continue
        first = [n.split()[0] for n in per_path]
        assert first[0] == first[1] == first[2], (case.name, i, sizes[i], first)
        if k.word is not None:
            assert first[0] == k.word, (case.name, i, sizes[i], first[0], k.word)
        if "design-q" in k.tags:
            assert all(n.startswith("fast-q") for n in per_path), per_path
        words.append(first[0])
    # ---- one-shot equality: bit for bit one sdrfm_process call of the whole input on a fresh staged handle
    got = np.concatenate(runs["mapped"][0])
    if case.flags in ("bit_exact", "force_generic"):
        with _handle(pkg, g, case.flags, iq.size, no_zerocopy=True) as one:
            whole = one.process(iq)
        assert np.array_equal(_bits(whole), _bits(got)), case.name
    # ---- oracle
    err = scaled_err(got, np.concatenate(want))
    tally = " ".join("%s x%d" % (w, words.count(w)) for w in ("fast-q", "fast-b", "generic") if w in words)
    print("\n[fm-host-paths] %-44s calls %2d  audio %6d  worst scaled err %.3g  (%s)" % (case.name, len(sizes), got.size, err, tally))
    assert err <= TOL, (case.name, err)


# ---- refusals change nothing --------------------------------------------------------------------------------------------------------------------
REFUSAL_SIZES = (4000, 2002, 8000, 1998, 4096)


@pytest.mark.parametrize("flags", ("default", "bit_exact"))
@pytest.mark.parametrize("staged", (False, True), ids=("mapped", "staged"))
def test_refused_calls_change_nothing(pkg, staged, flags):
    g, lib = hc.GEOMS[0], pkg.load_library()
    iq = _iq(pkg, "fm", sum(REFUSAL_SIZES) // 2)
    chunks = _chunks(iq, REFUSAL_SIZES)
    max_bytes = 8000
    with _handle(pkg, g, flags, max_bytes, no_zerocopy=staged) as clean:
        want, want_names, _ = _direct(clean, chunks)
    big = np.ascontiguousarray(np.tile(iq, 2)[:max_bytes + 2])
    buf = np.full(1024, ru.CANARY, np.float32)
    n = C.c_uint32()
    with _handle(pkg, g, flags, max_bytes, no_zerocopy=staged) as dm:
        for i, chunk in enumerate(chunks):
            name, count = dm.kernel_name, dm.audio_count(len(chunk))
            assert count > 0
            refusals = ((big.ctypes.data, 4001, buf.size, ru.EODD),                       # an odd nbytes
                        (big.ctypes.data, max_bytes + 2, buf.size, ru.ECAPACITY),          # two bytes above max_bytes_per_call
                        (chunk.ctypes.data, len(chunk), count - 1, ru.ECAPACITY))          # an audio_cap one short
            for ptr, nbytes, cap, status in refusals:
                n.value = 0xFFFF
                assert lib.sdrfm_process(dm._h, ptr, nbytes, buf.ctypes.data, cap, C.byref(n)) == status, (i, nbytes, cap)
                assert (buf == ru.CANARY).all() and dm.kernel_name == name and dm.audio_count(len(chunk)) == count
            got = dm.process(chunk)
            assert np.array_equal(_bits(got), _bits(want[i])) and dm.kernel_name == want_names[i], (i, dm.kernel_name, want_names[i])


# ---- host batches ---------------------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (2, 3998, 20002, 0, 8000, 70002)                    # (one sample; an odd count and the call behind it; nothing; a call above the mapped path's limit)


@pytest.mark.parametrize("ns", (3, 5))
@pytest.mark.parametrize("g", (hc.GEOMS[0], hc.GEOMS[3]), ids=lambda g: "T%d-D%d" % (g.T, g.D))
def test_host_batches_with_padded_rows(pkg, oracle_mod, g, ns):
    """sdrfm_process_batch on host buffers with iq_stride > nbytes and audio_stride > A: the staged path whatever the size; every stream against its own
    oracle, canaries in both paddings intact (the input's too: the call only reads)."""
    lib = pkg.load_library()
    h, a = _taps(pkg, g)
    total = sum(BATCH_SIZES)
    rows = pkg.make_iq(ns, total // 2, mode="fm", first_id=4300)
    orcs = [oracle_mod.Oracle(h, a, g.D, g.Da) for _ in range(ns)]
    n = C.c_uint32()
    worst, pos = 0.0, 0
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=a, fir_decim=g.D, audio_decim=g.Da, n_streams=ns, max_bytes_per_call=max(BATCH_SIZES))) as dm:
        for nbytes in BATCH_SIZES:
            A = dm.audio_count(nbytes)
            iq = np.full((ns, nbytes + 6), 0xA5, np.uint8)
            iq[:, :nbytes] = rows[:, pos:pos + nbytes]
            audio = np.full((ns, A + 3), ru.CANARY, np.float32)
            assert lib.sdrfm_process_batch(dm._h, iq.ctypes.data, nbytes + 6, nbytes, audio.ctypes.data, A + 3, C.byref(n), 0) == ru.OK
            assert n.value == A and (audio[:, A:] == ru.CANARY).all() and (iq[:, nbytes:] == 0xA5).all()
            assert np.array_equal(iq[:, :nbytes], rows[:, pos:pos + nbytes])
            for s in range(ns):
                want = orcs[s].process(rows[s, pos:pos + nbytes])
                assert want.size == A
                worst = max(worst, scaled_err(audio[s, :A], want))
            pos += nbytes
    print("\n[fm-host-paths] host batch T%d D%d Ta%d Da%d x %d streams, padded rows: worst scaled err %.3g" % (g.T, g.D, g.Ta, g.Da, ns, worst))
    assert worst <= TOL


@pytest.mark.parametrize("staged", (False, True), ids=("mapped", "staged"))
def test_one_stream_host_batch_ignores_both_strides(pkg, staged):
    """sdrfm_process_batch with one stream, iq_stride = 0 and audio_stride = 0: the bits of sdrfm_process (stage_iq / fetch_audio take the call's own sizes)"""
    g, lib = hc.GEOMS[0], pkg.load_library()
    sizes = [s for s in BATCH_SIZES if s]
    iq = _iq(pkg, "fm", sum(sizes) // 2)
    chunks = _chunks(iq, sizes)
    with _handle(pkg, g, "default", max(sizes), no_zerocopy=staged) as ref:
        want, want_names, _ = _direct(ref, chunks)
    n = C.c_uint32()
    with _handle(pkg, g, "default", max(sizes), no_zerocopy=staged) as dm:
        for i, chunk in enumerate(chunks):
            A = dm.audio_count(len(chunk))
            audio = np.full(A + 4, ru.CANARY, np.float32)
            assert lib.sdrfm_process_batch(dm._h, chunk.ctypes.data, 0, len(chunk), audio.ctypes.data, 0, C.byref(n), 0) == ru.OK
            assert n.value == A and (audio[A:] == ru.CANARY).all()
            assert np.array_equal(_bits(audio[:A]), _bits(want[i])) and dm.kernel_name == want_names[i], (i, dm.kernel_name)
