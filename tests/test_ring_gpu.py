"""Pinned-ring streaming front end (sdrfm_ring_*): the reference's declared-but-unused 15 x 262144-byte buffer scheme
(usbh_rtlsdr.h:277-278) driven without blocking, audio in order and identical to the synchronous path."""
import ctypes as C

import numpy as np
import pytest

import fm_host_cases as hc
import fm_ring_util as ru
from conftest import scaled_err, TOL

pytestmark = pytest.mark.gpu
BUSY = 1


def test_ring_feeds_in_order_and_matches_oracle(pkg, oracle_mod):
    lib = pkg.load_library()
    h, g = pkg.default_config(64)
    dm = pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, max_bytes_per_call=262144))
    ring = C.c_void_p()
    assert lib.sdrfm_ring_create(dm._h, 15, 16 * 32 * 512, C.byref(ring)) == 0     # DEFAULT_BUF_NUMBER x DEFAULT_BUF_LENGTH
    iq = pkg.make_iq(1, 131072 * 40 + 12345 * 1, mode="fm", first_id=61)[0]
    iq = iq[: iq.size & ~1]
    out, pos, busy_submit = [], 0, 0
    buf = np.empty(262144 // 2 // 10 // 5 + 8, np.float32)
    n = C.c_uint32()
    reuse = np.empty(262144, np.uint8)                                             # ONE caller buffer, reused like CommItf.buff
    while pos < iq.size or True:
        if pos < iq.size:
            m = min(262144, iq.size - pos)
            reuse[:m] = iq[pos:pos + m]
            st = lib.sdrfm_ring_submit(ring, reuse.ctypes.data, m)
            if st == 0:
                pos += m
                reuse[:] = 0xEE                                                     # slot owns a copy: clobbering is harmless
            else:
                assert st == BUSY
                busy_submit += 1
                assert lib.sdrfm_ring_collect(ring, buf.ctypes.data, buf.size, C.byref(n), 1) == 0
                out.append(buf[: n.value].copy())
            continue
        st = lib.sdrfm_ring_collect(ring, buf.ctypes.data, buf.size, C.byref(n), 1)
        if st == BUSY:
            break                                                                  # ring drained
        assert st == 0
        out.append(buf[: n.value].copy())
    got = np.concatenate(out)
    want = oracle_mod.Oracle(h, g).process(iq)
    assert busy_submit > 0                                                         # 41 buffers through 15 slots
    assert got.size == want.size
    assert scaled_err(got, want) <= TOL
    # non-blocking collect on an empty ring and argument checks
    assert lib.sdrfm_ring_collect(ring, buf.ctypes.data, buf.size, C.byref(n), 0) == BUSY
    assert lib.sdrfm_ring_submit(ring, reuse.ctypes.data, 7) == 17
    assert lib.sdrfm_ring_submit(ring, reuse.ctypes.data, 262146) == 18
    lib.sdrfm_ring_destroy(ring)
    dm.close()


# ---- the ring's lifecycle at small shapes (the cases tools/fuzz_parity.py `ring` used to be alone with) ---------------------------------------------
RING_GEOMS = (hc.GEOMS[0], hc.GEOMS[3])                            # (64, 10, 32, 5) and (7, 3, 5, 4)
geoms = pytest.mark.parametrize("g", RING_GEOMS, ids=lambda g: "T%d-D%d" % (g.T, g.D))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _taps(pkg, g):
    if g.Ta == 32:
        return pkg.default_config(g.T, fir_decim=g.D, audio_taps=g.Ta, audio_decim=g.Da)
    rng = np.random.default_rng(g.T + g.D)                        # (audio taps of unit absolute sum: the plain tolerance applies)
    h = (rng.standard_normal(g.T) / np.sqrt(g.T)).astype(np.float32)
    a = rng.standard_normal(g.Ta)
    return h, (a / np.abs(a).sum()).astype(np.float32)


def _dm(pkg, g, max_bytes=4096, **kw):
    h, a = _taps(pkg, g)
    return pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=a, fir_decim=g.D, audio_decim=g.Da, max_bytes_per_call=max_bytes, **kw))


def _cut(iq, sizes):
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    assert cuts[-1] <= iq.size
    return [iq[cuts[i]:cuts[i + 1]] for i in range(len(sizes))]


def _ragged(total_bytes, slot):
    """chunk sizes up to one slot: full slots, one sample short, one sample, half a slot, nothing"""
    out, pattern, k = [], (slot, slot - 2 if slot > 2 else slot, 2, slot, max(2, slot // 2 & ~1), 0, slot), 0
    while sum(out) + slot <= total_bytes:
        out.append(pattern[k % len(pattern)])
        k += 1
    return out


@geoms
@pytest.mark.parametrize("n_buffers,buffer_bytes", ((2, 512), (64, 512), (2, 2), (64, 2)))
def test_ring_at_its_limits_matches_the_oracle(pkg, oracle_mod, g, n_buffers, buffer_bytes):
    lib = pkg.load_library()
    sizes = _ragged(80 * 512 if buffer_bytes == 512 else 2 * 400, buffer_bytes)
    assert sum(1 for s in sizes if s) > n_buffers
    iq = pkg.make_iq(1, sum(sizes) // 2, mode="fm", first_id=62)[0]
    chunks = _cut(iq, sizes)
    h, a = _taps(pkg, g)
    with _dm(pkg, g) as dm:
        ring = ru.Ring(lib, dm, n_buffers, buffer_bytes)
        outs, busy, _, counts = ru.feed(ring, chunks)
        ring.destroy()
    assert busy > 0 and [o.size for o in outs] == counts
    got, want = np.concatenate(outs), oracle_mod.Oracle(h, a, g.D, g.Da).process(iq)
    assert want.size > 0 and scaled_err(got, want) <= TOL


def test_ring_create_refusals(pkg):
    lib, g = pkg.load_library(), RING_GEOMS[0]
    with _dm(pkg, g) as dm:
        for n_buffers, buffer_bytes in ((1, 512), (65, 512), (3, 0), (3, 511), (0, 512)):
            st, out = ru.ring_create(lib, dm, n_buffers, buffer_bytes)
            assert st == ru.EINVAL and not out.value, (n_buffers, buffer_bytes, st)
    h, a = _taps(pkg, g)
    with pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=a, n_streams=2, max_bytes_per_call=4096)) as dm2:
        st, out = ru.ring_create(lib, dm2, 3, 512)
        assert st == ru.EINVAL and not out.value                    # single-stream handles only


@geoms
def test_ring_slot_accounting_and_refused_submits(pkg, g):
    """Exactly n_buffers submits go in without a collect; SDRFM_BUSY, SDRFM_ECAPACITY and SDRFM_EODD consume nothing and a 0-byte submit takes no slot even
    on a full ring: the audio is bit for bit a ring's that never saw those calls."""
    lib = pkg.load_library()
    iq = pkg.make_iq(1, 5 * 256, mode="fm", first_id=63)[0]
    chunks = _cut(iq, [512] * 5)
    with _dm(pkg, g) as clean:
        ring = ru.Ring(lib, clean, 3, 512)
        want, _, _, _ = ru.feed(ring, chunks)
        ring.destroy()
    with _dm(pkg, g) as dm:
        ring = ru.Ring(lib, dm, 3, 512)
        assert [ring.submit(c) for c in chunks[:3]] == [ru.OK] * 3
        count = dm.audio_count(512)
        over = np.zeros(514, np.uint8)
        for _ in range(2):
            assert ring.submit(chunks[3]) == ru.BUSY
            assert ring.submit(np.zeros(0, np.uint8)) == ru.OK
            assert ring.submit(over) == ru.ECAPACITY and ring.submit(over[:511]) == ru.EODD
            assert dm.audio_count(512) == count
        got = [ring.collect(1) for _ in range(3)]
        assert ring.collect(1)[0] == ru.BUSY and ring.collect(0)[0] == ru.BUSY          # the 0-byte submits and the refused ones left nothing behind
        assert [ring.submit(c) for c in chunks[3:]] == [ru.OK] * 2
        got += [ring.collect(1) for _ in range(2)]
        assert ring.submit(over) == ru.ECAPACITY and ring.submit(over[:511]) == ru.EODD   # (on an empty ring too)
        ring.destroy()
    assert [st for st, _ in got] == [ru.OK] * 5
    for i, (_, out) in enumerate(got):
        assert out.size > 0 and np.array_equal(_bits(out), _bits(want[i])), i


@geoms
def test_ring_collect_into_too_small_a_buffer_keeps_the_slot(pkg, g):
    lib = pkg.load_library()
    iq = pkg.make_iq(1, 3 * 256, mode="fm", first_id=64)[0]
    chunks = _cut(iq, [512] * 3)
    with _dm(pkg, g) as clean:
        ring = ru.Ring(lib, clean, 3, 512)
        want, _, _, _ = ru.feed(ring, chunks)
        ring.destroy()
    with _dm(pkg, g) as dm:
        ring = ru.Ring(lib, dm, 3, 512)
        assert [ring.submit(c) for c in chunks] == [ru.OK] * 3
        for i in range(3):
            assert want[i].size > 1
            for wait in (1, 0, 1):                                # (the slot is finished after the first blocking attempt: wait = 0 finds it ready)
                st, out = ring.collect(wait, cap=want[i].size - 1)   # n_audio = 0 and the canaries are checked in there
                assert st == ru.ECAPACITY and out is None
            st, out = ring.collect(0, cap=want[i].size)            # exactly enough room: the same slot, intact
            assert st == ru.OK and np.array_equal(_bits(out), _bits(want[i])), i
        assert ring.collect(1)[0] == ru.BUSY
        ring.destroy()


@geoms
def test_ring_keeps_order_with_polled_and_blocking_collects_mixed(pkg, oracle_mod, g):
    lib = pkg.load_library()
    sizes = [512, 2, 300, 512, 2, 2, 512, 130, 512, 512, 4, 512]  # (the chunks of one or two samples mostly produce no audio: their slots still come back)
    iq = pkg.make_iq(1, sum(sizes) // 2, mode="fm", first_id=65)[0]
    chunks = _cut(iq, sizes)
    h, a = _taps(pkg, g)
    orc = oracle_mod.Oracle(h, a, g.D, g.Da)
    want = [orc.process(c) for c in chunks]
    assert any(w.size == 0 for w in want) and sum(w.size for w in want) > 20
    outs, pending = [], 0
    with _dm(pkg, g) as dm:
        ring = ru.Ring(lib, dm, 4, 512)
        for i, chunk in enumerate(chunks):
            if pending == 4:                                        # full: take the oldest one, polled and blocking in turn
                outs.append(ring.collect_polled()[0] if i % 2 else ring.collect(1)[1])
                pending -= 1
            assert ring.submit(chunk) == ru.OK
            pending += 1
            if i % 3 == 0:                                          # ... and one in between, whatever is in flight
                outs.append(ring.collect_polled(8)[0] if i % 2 == 0 else ring.collect(1)[1])
                pending -= 1
        while pending:
            outs.append(ring.collect_polled()[0] if pending % 2 else ring.collect(1)[1])
            pending -= 1
        assert ring.collect(0)[0] == ru.BUSY
        ring.destroy()
    assert [o.size for o in outs] == [w.size for w in want]
    assert scaled_err(np.concatenate(outs), np.concatenate(want)) <= TOL


@geoms
def test_ring_and_process_calls_continue_one_stream(pkg, g):
    """sdrfm_process calls, a drained ring, sdrfm_process, the ring again on one bit-exact handle: bit for bit an all-sdrfm_process run of the same cuts;
    after sdrfm_reset the next submits are a fresh stream's, first-call fix-up included."""
    lib = pkg.load_library()
    sizes = [2 * g.D * (hc.y_aff(g) + g.Ta + g.Da), 1002, 4096, 2, 3000, 998, 4096, 514]   # (the first call: long enough for the fast kernel and its fix-up)
    assert max(sizes) <= 4096
    iq = pkg.make_iq(1, sum(sizes) // 2, mode="fm", first_id=66)[0]
    chunks = _cut(iq, sizes)
    with _dm(pkg, g, bit_exact=True) as ref:
        want = [ref.process(c).copy() for c in chunks]
    with _dm(pkg, g, bit_exact=True) as dm:
        ring = ru.Ring(lib, dm, 2, 4096)
        got = [dm.process(c).copy() for c in chunks[:2]]
        got += ru.feed(ring, chunks[2:5])[0]
        got += [dm.process(chunks[5]).copy()]
        got += ru.feed(ring, chunks[6:])[0]
        for i in range(len(sizes)):
            assert np.array_equal(_bits(got[i]), _bits(want[i])), (i, sizes[i])
        dm.reset()
        again, _, names, _ = ru.feed(ring, chunks[:3])
        for i in range(3):
            assert np.array_equal(_bits(again[i]), _bits(want[i])), (i, sizes[i])
        if g.Ta == 32:
            assert names[0].startswith("fast-b"), names                # (the fast kernel and the generic fix-up of the first tiles, on the ring)
        ring.destroy()


@geoms
def test_ring_destroyed_with_slots_in_flight_leaves_the_handle_usable(pkg, oracle_mod, g):
    lib = pkg.load_library()
    iq = pkg.make_iq(1, 3 * 2048, mode="fm", first_id=67)[0]
    h, a = _taps(pkg, g)
    with _dm(pkg, g, max_bytes=iq.size) as dm:
        ring = ru.Ring(lib, dm, 4, 4096)
        assert [ring.submit(c) for c in _cut(iq, [4096] * 3)] == [ru.OK] * 3
        ring.destroy()                                              # no collect: ring_free synchronises its three streams
        dm.reset()
        got = dm.process(iq)
    assert scaled_err(got, oracle_mod.Oracle(h, a, g.D, g.Da).process(iq)) <= TOL


@geoms
def test_ring_on_a_caller_stream_gives_the_same_bits(pkg, g):
    import torch
    lib = pkg.load_library()
    sizes = _ragged(12 * 512, 512)
    iq = pkg.make_iq(1, sum(sizes) // 2, mode="fm", first_id=68)[0]
    chunks = _cut(iq, sizes)
    with _dm(pkg, g) as own:
        ring = ru.Ring(lib, own, 3, 512)
        want = ru.feed(ring, chunks)[0]
        ring.destroy()
    stream = torch.cuda.Stream()
    with _dm(pkg, g) as dm:
        dm.set_stream(stream.cuda_stream)                           # before the ring is created
        ring = ru.Ring(lib, dm, 3, 512)
        got = ru.feed(ring, chunks)[0]
        ring.destroy()
        dm.set_stream(None)
    stream.synchronize()
    assert len(got) == len(want) and sum(o.size for o in got) > 0
    for i in range(len(got)):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), i


def test_two_handles_each_with_a_ring_interleaved(pkg, oracle_mod):
    lib = pkg.load_library()
    sizes = [[512, 300, 512, 2, 512, 512, 130, 512], [256, 512, 512, 512, 4, 512, 510, 512]]
    iqs = [pkg.make_iq(1, sum(s) // 2, mode=m, first_id=69 + k)[0] for k, (s, m) in enumerate(zip(sizes, ("fm", "random")))]
    chunks = [_cut(iq, s) for iq, s in zip(iqs, sizes)]
    dms = [_dm(pkg, g) for g in RING_GEOMS]
    rings = [ru.Ring(lib, dm, 2, 512) for dm in dms]
    outs, pending = [[], []], [0, 0]
    for i in range(8):
        for k in (0, 1):
            if pending[k] == 2:
                outs[k].append(rings[k].collect_polled(4)[0])
                pending[k] -= 1
            assert rings[k].submit(chunks[k][i]) == ru.OK
            pending[k] += 1
    for k in (1, 0):
        outs[k] += rings[k].drain()
    for k in (0, 1):
        rings[k].destroy()
        dms[k].close()
        g = RING_GEOMS[k]
        h, a = _taps(pkg, g)
        want = oracle_mod.Oracle(h, a, g.D, g.Da).process(iqs[k])
        got = np.concatenate(outs[k])
        assert got.size == want.size > 0 and scaled_err(got, want) <= TOL, k
