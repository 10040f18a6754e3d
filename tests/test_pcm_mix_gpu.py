"""The PCM mix bus on the device: k_pcm_mix against the host routine sdrfm_pcm_mix_s16 bit for bit, records included, over the
shapes of tests/pcm_mix_cases.py — every n around a workgroup's span, every slot count's ends, every mode, dead slots beside live ones, rows at
every address a 4-byte aligned row can have mod 16 between canaries — then ramps across calls and sets, cut invariance, the three identities,
the call forms, every refusal, and the chain sink -> limiter -> mixer on one stream."""
import ctypes as C

import numpy as np
import pytest

import pcm_mix_cases as cases

pytestmark = pytest.mark.gpu
ONE, NONE, SPAN = cases.ONE, cases.NONE, cases.SPAN


def _pair(pkg, n_in, n_bus, n_slots, slew, curve=None):
    t = None if curve is None else pkg.mix_curve(curve)
    return pkg.PcmMixer(n_in, n_bus, n_slots, slew, t), cases.HostMixer(pkg, n_in, n_bus, n_slots, slew, t)


def _device_call(mixer, x, n_bus, in_off=0, out_off=0, pad_in=2, pad_out=6):
    """one device call on rows in_off and out_off bytes into 16-byte aligned allocations, strides 2n + pad: the PCM [n_bus, 2n]; the input, the
    padding between the rows and behind the last, and a canary row are neither changed nor written"""
    import torch
    n_in, n = x.shape[0], x.shape[1] // 2
    si, so = 2 * n + pad_in, 2 * n + pad_out
    flat_in = torch.full((in_off // 2 + (n_in + 1) * si,), 12345, dtype=torch.int16, device="cuda")
    flat_out = torch.full((out_off // 2 + (n_bus + 1) * so,), cases.CANARY, dtype=torch.int16, device="cuda")
    assert flat_in.data_ptr() % 16 == 0 and flat_out.data_ptr() % 16 == 0
    d_in = flat_in[in_off // 2:].view(n_in + 1, si)
    if n:
        d_in[:n_in, :2 * n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    keep = flat_in.clone()
    torch.cuda.synchronize()
    mixer.process_batch_ptr(flat_in.data_ptr() + in_off, si, n, flat_out.data_ptr() + out_off, so)
    mixer.synchronize()
    assert torch.equal(flat_in, keep)
    out = flat_out.cpu().numpy()
    assert (out[:out_off // 2] == cases.CANARY).all()
    out = out[out_off // 2:].reshape(n_bus + 1, so)
    assert (out[n_bus] == cases.CANARY).all() and (out[:n_bus, 2 * n:] == cases.CANARY).all()
    return out[:n_bus, :2 * n]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("n", cases.N_VALUES)
def test_device_is_the_host_routine(pkg, n, shape):
    n_in, n_bus, n_slots = shape
    idx = cases.N_VALUES.index(n) * len(cases.SHAPES) + cases.SHAPES.index(shape)
    in_off, out_off = cases.OFFSETS[idx % 4], cases.OFFSETS[(idx // 4 + idx) % 4]
    for curve in (None, "equal_power"):
        for first_mode in (range(5) if n_bus * n_slots < 5 else (idx % 5,)):      # every mode, also where the table has a single slot
            dev, host = _pair(pkg, n_in, n_bus, n_slots, cases.SLEWS[idx % 3], curve)
            with dev:
                table = cases.slot_table(idx, n_in, n_bus, n_slots, first_mode)
                cases.load(dev, table)
                host.load(table)
                assert host.holds(dev) and dev.kernel_name() == "pcm-mix"
                for call in range(2):                                              # the second call goes on from the first's J
                    x = cases.rows(100 * idx + call, n_in, n)
                    got = _device_call(dev, x, n_bus, in_off, out_off)
                    assert np.array_equal(got, host.process_batch(x)), (curve, first_mode, call)
                    assert host.holds(dev) and dev.read().tobytes() == host.rec.tobytes(), (curve, first_mode, call)


def test_rows_at_every_address(pkg):
    """input and output rows independently at 0, 4, 8 and 12 bytes mod 16, and with strides that move every further row by 4 and by 12 bytes"""
    n_in, n_bus, n_slots, n = 3, 2, 2, SPAN + 1
    dev, host = _pair(pkg, n_in, n_bus, n_slots, 7, "equal_power")
    with dev:
        table = cases.slot_table(5, n_in, n_bus, n_slots)
        cases.load(dev, table)
        host.load(table)
        for k, (in_off, out_off) in enumerate((a, b) for a in cases.OFFSETS for b in cases.OFFSETS):
            x = cases.rows(300 + k, n_in, n)
            assert np.array_equal(_device_call(dev, x, n_bus, in_off, out_off), host.process_batch(x)), (in_off, out_off)
        assert dev.read().tobytes() == host.rec.tobytes() and host.holds(dev)


@pytest.mark.parametrize("kind", ["rail_lo", "rail_hi"])
def test_the_two_rails(pkg, kind):
    """eight STEREO slots at unity on a constant rail: the sum at its bound, every output clipped, peak 2^18 on the negative rail; and the case
    table's mixture of slots on the same rows"""
    n = SPAN + 1
    x = cases.rows(0, 2, n, kind)
    dev, host = _pair(pkg, 2, 5, 8, 1)
    with dev:
        for k in (dev, host):
            k.set_routes(np.arange(40).reshape(5, 8) % 2, 0)
            k.set_gains(ONE, jump=True)
        got = _device_call(dev, x, 5, 4, 8)
        assert np.array_equal(got, host.process_batch(x)) and (got == (-32768 if kind == "rail_lo" else 32767)).all()
        rec = dev.read(reset=True)
        assert rec.tobytes() == host.read(reset=True).tobytes()
        assert [tuple(int(v) for v in r) for r in rec] == [(n, n, n, 262144 if kind == "rail_lo" else 8 * 32767)] * 5
    table = cases.slot_table(9, 2, 5, 8)
    dev, host = _pair(pkg, 2, 5, 8, 7, "equal_power")
    with dev:
        cases.load(dev, table)
        host.load(table)
        assert np.array_equal(_device_call(dev, x, 5, 12, 0), host.process_batch(x)) and dev.read().tobytes() == host.rec.tobytes()


@pytest.mark.parametrize("slew", cases.SLEWS)
def test_ramps_across_calls_and_sets(pkg, slew):
    """a crossfade, and ramps that end inside a span, at a span's last pair and inside a later call; then set_gains without and with a jump and
    set_routes between calls"""
    n1 = 2 * SPAN + 3
    cap = lambda pairs: min(ONE, slew * pairs)
    src = [[0, 1], [2, 0], [1, NONE]]
    mode = [[0, 0], [1, 4], [2, 0]]
    start = [[ONE, 0], [0, 0], [0, 0]]
    target = [[0, ONE], [cap(1000), cap(SPAN)], [cap(n1 + 500), 0]]
    for curve in (None, "equal_power"):
        dev, host = _pair(pkg, 3, 3, 2, slew, curve)
        with dev:
            for k in (dev, host):
                k.set_routes(src, mode)
                k.set_gains(start, jump=True)
                k.set_gains(target)
            script = [("call", n1), ("call", 700),
                      ("gains", [[ONE, 0], [0, 5], [123, 0]], False), ("call", 700),          # from wherever the ramps have got to
                      ("routes", [[2, 1], [0, NONE], [1, 2]], [[4, 3], [1, 4], [2, 0]]), ("call", SPAN + 1),
                      ("gains", [[77, 30000], [ONE, ONE], [0, 1]], True), ("call", 5),
                      ("gains", 0, False), ("call", SPAN)]
            for step, op in enumerate(script):
                if op[0] == "call":
                    x = cases.rows(500 + step, 3, op[1])
                    got = _device_call(dev, x, 3, cases.OFFSETS[step % 4], cases.OFFSETS[(step + 1) % 4])
                    assert np.array_equal(got, host.process_batch(x)), (curve, step)
                elif op[0] == "gains":
                    dev.set_gains(op[1], jump=op[2])
                    host.set_gains(op[1], jump=op[2])
                else:
                    dev.set_routes(op[1], op[2])
                    host.set_routes(op[1], op[2])
                assert host.holds(dev), (curve, step)
            assert dev.read().tobytes() == host.rec.tobytes()
            if slew == 7 and curve is None:                                     # the script is what its docstring says
                assert target[1] == [7000, 14336] and target[2][0] == 7 * (n1 + 500) < ONE


def test_j_past_its_ceiling_and_the_longest_call(pkg):
    """one call of 70 000 pairs on one bus carries J past 65536, then one more call; and one call of 2^20 pairs.  The crossfade is on one source:
    the bus is the row itself throughout"""
    dev, host = _pair(pkg, 1, 1, 2, 1)
    with dev:
        for k in (dev, host):
            k.set_routes(0, [[0, 0]])
            k.set_gains([[ONE, 0]], jump=True)
            k.set_gains([[0, ONE]])
        for n, J in ((70000, 65536), (100, 65536)):
            x = cases.rows(n, 1, n)
            got = _device_call(dev, x, 1, 8, 4)
            assert np.array_equal(got, host.process_batch(x)) and np.array_equal(got, x) and host.holds(dev) and dev.slots()[1] == J
        assert dev.read().tobytes() == host.rec.tobytes()
    dev, host = _pair(pkg, 1, 1, 1, 1, "equal_power")
    with dev:
        for k in (dev, host):
            k.set_routes(0, 1)
            k.set_gains(ONE, jump=True)
            k.set_gains(0)
        x = cases.rows(77, 1, 1 << 20)
        got = _device_call(dev, x, 1, 12, 12)
        assert np.array_equal(got, host.process_batch(x)) and host.holds(dev) and dev.read().tobytes() == host.rec.tobytes()
        assert got[:, :2000].any() and not got[:, 2 * 32768:].any()             # faded out after 32768 pairs


def test_cuts_equal_one_call(pkg):
    """a run in one call against the cuts (0, 1, SPAN - 1, SPAN + 2, rest), twice, with the same sets at the same pair positions — before the
    run and between the two runs: equal PCM, and equal records after mix_add"""
    n_in, n_bus, n_slots, n = 3, 2, 2, SPAN + SPAN + 2 + 700
    table = cases.slot_table(21, n_in, n_bus, n_slots)
    for curve in (None, "equal_power"):
        one, host = _pair(pkg, n_in, n_bus, n_slots, 7, curve)
        cut = _pair(pkg, n_in, n_bus, n_slots, 7, curve)[0]
        with one, cut:
            cases.load(one, table)
            cases.load(cut, table)
            host.load(table)
            acc = np.zeros(n_bus, pkg.MIX_DTYPE)
            for run in range(2):
                x = cases.rows(600 + run, n_in, n)
                whole = _device_call(one, x, n_bus, 4, 0)
                parts, at = [], 0
                for c in cases.cuts(n):
                    parts.append(_device_call(cut, x[:, 2 * at:2 * (at + c)], n_bus, cases.OFFSETS[len(parts) % 4], 8))
                    pkg.mix_add(acc, cut.read(reset=True))
                    at += c
                assert at == n and np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(whole, host.process_batch(x)), (curve, run)
                assert acc.tobytes() == one.read().tobytes() == host.rec.tobytes(), (curve, run)
                assert host.holds(one) and host.holds(cut)
                for k in (one, cut, host):
                    k.set_gains([[ONE, 100], [0, 20000]])


def test_the_three_identities(pkg):
    n = SPAN + 1
    x = cases.rows(31, 2, n)
    # unity: one STEREO slot at 32768 beside a slot at 0 and one without a source
    with pkg.PcmMixer(2, 2, 3, 5) as dev:
        dev.set_routes([[0, 1, NONE], [NONE, 0, 1]], [[0, 1, 2], [3, 4, 0]])
        dev.set_gains([[ONE, 0, ONE], [ONE, 0, ONE]], jump=True)
        got = _device_call(dev, x, 2, 4, 12)
        assert np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[1])
        assert [tuple(int(v) for v in r)[:3] for r in dev.read()] == [(n, 0, 0)] * 2
    # the self-crossfade at every slew: y = x at every pair, from the set's first pair to far behind the ramp's end
    for slew in cases.IDENTITY_SLEWS:
        for curve in (None, "linear"):
            with pkg.PcmMixer(2, 1, 2, slew, None if curve is None else pkg.mix_curve(curve)) as dev:
                dev.set_routes(1, 0)
                dev.set_gains([[ONE, 0]], jump=True)
                dev.set_gains([[0, ONE]])
                for call in range(2):
                    assert np.array_equal(_device_call(dev, x, 1, 0, 4)[0], x[1]), (slew, curve, call)
    # MONO at 32768 is (L + R + 1) >> 1 and never clips: full-range pairs and the four corners
    corners = np.array([[-32768, -32768, 32767, 32767, -32768, 32767, 32767, -32768]], np.int16)
    y = np.concatenate([corners, x[:1, :2 * n - 8]], axis=1)
    with pkg.PcmMixer(1, 1, 1, 1) as dev:
        dev.set_routes(0, "mono")
        dev.set_gains(ONE, jump=True)
        got = _device_call(dev, y, 1, 8, 8)[0]
        L, R = y[0, 0::2].astype(np.int64), y[0, 1::2].astype(np.int64)
        assert np.array_equal(got[0::2], (L + R + 1) >> 1) and np.array_equal(got[0::2], got[1::2])
        rec = dev.read()[0]
        assert (int(rec["n"]), int(rec["clipped_l"]), int(rec["clipped_r"])) == (n, 0, 0) and int(rec["peak"]) == 32768


def test_call_forms(pkg):
    """host rows against device rows; the caller's stream; read with and without reset, to host and to device memory; reset"""
    import torch
    n_in, n_bus, n_slots, n = 3, 2, 2, SPAN + 5
    table = cases.slot_table(41, n_in, n_bus, n_slots)
    stream = torch.cuda.Stream()
    a, host = _pair(pkg, n_in, n_bus, n_slots, 7, "equal_power")
    b = _pair(pkg, n_in, n_bus, n_slots, 7, "equal_power")[0]
    with a, b:
        b.set_stream(stream.cuda_stream)
        cases.load(a, table)
        cases.load(b, table)
        host.load(table)
        zero = np.zeros(n_bus, pkg.MIX_DTYPE)
        assert a.read().tobytes() == zero.tobytes()
        x = cases.rows(700, n_in, 2 * n)
        d_x = torch.from_numpy(x).cuda()
        d_rec = torch.zeros(4 * n_bus, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        first = None
        for c in range(2):
            xc = np.ascontiguousarray(x[:, 2 * c * n:2 * (c + 1) * n])
            want = host.process_batch(xc)
            assert np.array_equal(a.process_batch(xc), want), c                  # host rows: staged and synchronous
            d_out = torch.full((n_bus, 2 * n + 4), 99, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            got = b.process_batch(d_x[:, 2 * c * n:2 * (c + 1) * n], d_out, n)  # device rows on the caller's stream: enqueued only
            assert got is d_out
            b.read_device(d_rec, reset=(c == 0))                                 # behind the call, on the same stream
            stream.synchronize()
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:, :2 * n], want) and (out[:, 2 * n:] == 99).all(), c
            rec_b = d_rec.cpu().numpy().view(pkg.MIX_DTYPE)
            if c == 0:
                first = rec_b.copy()
                assert first.tobytes() == a.read().tobytes() == a.read().tobytes()   # a plain read changes nothing
            else:
                assert pkg.mix_add(first.copy(), rec_b).tobytes() == host.rec.tobytes() == a.read().tobytes()
                assert b.read().tobytes() == rec_b.tobytes()                     # the second device read did not reset
            assert host.holds(a) and host.holds(b)
        assert a.read(reset=True).tobytes() == host.rec.tobytes() and a.read().tobytes() == zero.tobytes()
        b.reset()
        assert b.read().tobytes() == zero.tobytes() and host.holds(b)            # reset keeps the slots, the ramps and J
        host.read(reset=True)
        x3 = cases.rows(701, n_in, 300)
        want = host.process_batch(x3)
        assert np.array_equal(a.process_batch(x3), want) and np.array_equal(_device_call(b, x3, n_bus), want)
        assert a.read().tobytes() == b.read().tobytes() == host.rec.tobytes()
        b.set_stream(None)                                                       # back on its own stream
        assert np.array_equal(_device_call(b, x3, n_bus), a.process_batch(x3))


def test_host_staging_grows_and_is_reused_below_capacity(pkg):
    """host-buffer calls of 1000, 1025 and 3 pairs in that order on one handle of 3 rows in and 3 buses: the staging is made, outgrown, and
    then used far below its capacity with the last call's pairs still behind the valid ones.  Every call's PCM and the records are the host
    routine's, J going on from call to call"""
    dev, host = _pair(pkg, 3, 3, 2, cases.SLEWS[1], "equal_power")
    with dev:
        table = cases.slot_table(77, 3, 3, 2)
        cases.load(dev, table)
        host.load(table)
        for call, n in enumerate((1000, 1025, 3)):
            x = cases.rows(7700 + call, 3, n)
            got = dev.process_batch(x)
            assert got.shape == (3, 2 * n) and np.array_equal(got, host.process_batch(x)), n
            assert host.holds(dev) and dev.read().tobytes() == host.rec.tobytes(), n


def test_every_refusal_leaves_the_handle_as_it_was(pkg):
    import torch
    lib = pkg.load_library()
    n_in, n_bus, n_slots, n = 2, 2, 2, 400
    table = cases.slot_table(51, n_in, n_bus, n_slots)
    dev, host = _pair(pkg, n_in, n_bus, n_slots, 7)
    with dev:
        cases.load(dev, table)
        host.load(table)
        x = cases.rows(800, n_in, n)
        assert np.array_equal(dev.process_batch(x), host.process_batch(x))
        h = dev._h
        d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        o = torch.full((n_bus, 2 * n + 2), 77, dtype=torch.int16, device="cuda")
        both = torch.full((4 * n_in, 2 * n), 77, dtype=torch.int16, device="cuda")
        y = np.full((n_bus, 2 * n), 77, np.int16)
        xy = np.full((3, 2 * n), 77, np.int16)
        torch.cuda.synchronize()
        E, CAP, DEV = pkg.lib.EINVAL, pkg.lib.ECAPACITY, pkg.lib.F_DEVICE_PTRS
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        calls = [((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n, 2), E), ((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n, 8), E),
                 ((h, x.ctypes.data, 2 * n, (1 << 20) + 1, y.ctypes.data, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n + 1, n, y.ctypes.data, 2 * n, 0), E), ((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n + 1, 0), E),
                 ((h, None, 2 * n, n, y.ctypes.data, 2 * n, 0), E), ((h, x.ctypes.data, 2 * n, n, None, 2 * n, 0), E),
                 ((h, x.ctypes.data, 2 * n - 2, n, y.ctypes.data, 2 * n, 0), CAP), ((h, x.ctypes.data, 2 * n, n, y.ctypes.data, 2 * n - 2, 0), CAP),
                 ((h, P(d, 2), 2 * n, n - 1, P(o), 2 * n + 2, DEV), E), ((h, P(d), 2 * n, n, P(o, 2), 2 * n + 2, DEV), E),
                 # no in-place form: the output rows on the input rows, one row into them from either side, and host rows likewise
                 ((h, P(both), 2 * n, n, P(both), 2 * n, DEV), E), ((h, P(both), 2 * n, n, P(both, 4 * n), 2 * n, DEV), E),
                 ((h, P(both, 4 * n), 2 * n, n, P(both), 2 * n, DEV), E), ((h, P(both, 4 * n), 2 * n, n - 1, P(both, 12 * n - 8), 2 * n, DEV), E),
                 ((h, xy.ctypes.data, 2 * n, n, xy.ctypes.data + 4 * n, 2 * n, 0), E)]
        for args, want in calls:
            assert lib.sdrfm_pcm_mix_process_batch(*args) == want, args[1:]
        # ... while rows that only touch are taken: the output rows begin where the input rows end
        assert lib.sdrfm_pcm_mix_process_batch(h, P(both), 2 * n, 0, P(both), 2 * n, DEV) == pkg.lib.OK      # (n == 0 comes first: a no-op)
        held = []

        def u(*v):
            held.append(np.array(v, np.uint32))                                  # (kept alive until the test ends)
            return held[-1].ctypes.data
        rec = np.zeros(n_bus + 1, pkg.MIX_DTYPE)
        assert lib.sdrfm_pcm_mix_set_routes(h, None, None) == E
        assert lib.sdrfm_pcm_mix_set_routes(h, u(0, 1, 2, 0), None) == E and lib.sdrfm_pcm_mix_set_routes(h, u(0, 1, NONE - 1, 0), None) == E
        assert lib.sdrfm_pcm_mix_set_routes(h, None, u(0, 1, 5, 0)) == E and lib.sdrfm_pcm_mix_set_routes(h, u(1, 1, 1, 1), u(0, 0, 0, 5)) == E
        assert lib.sdrfm_pcm_mix_set_gains(h, None, 0) == E and lib.sdrfm_pcm_mix_set_gains(h, u(0, 0, 0, ONE + 1), 0) == E
        assert lib.sdrfm_pcm_mix_set_gains(h, u(0, 0, 0, 0), 2) == E and lib.sdrfm_pcm_mix_set_gains(h, u(1, 1, 1, 1), 0xFFFFFFFF) == E
        assert lib.sdrfm_pcm_mix_read(h, None, 0) == E and lib.sdrfm_pcm_mix_read(h, rec.ctypes.data, 4) == E
        assert lib.sdrfm_pcm_mix_read(h, rec.ctypes.data + 4, 0) == E and lib.sdrfm_pcm_mix_read(h, rec.ctypes.data, 2) == E
        dev.synchronize()
        assert (y == 77).all() and (xy == 77).all() and bool((o == 77).all()) and bool((both == 77).all()) and not rec.tobytes().strip(b"\0")
        assert host.holds(dev) and dev.read().tobytes() == host.rec.tobytes()
        x2 = cases.rows(801, n_in, n)
        assert np.array_equal(dev.process_batch(x2), host.process_batch(x2)) and host.holds(dev)     # and the next call's bits
        assert dev.read().tobytes() == host.rec.tobytes()
        # rows that touch without overlapping are taken
        both[:n_in] = d
        torch.cuda.synchronize()
        dev.process_batch_ptr(both.data_ptr(), 2 * n, n, both.data_ptr() + 2 * n_in * 2 * n, 2 * n)
        dev.synchronize()
        assert np.array_equal(both[n_in:2 * n_in].cpu().numpy(), host.process_batch(x)) and bool((both[2 * n_in:] == 77).all())
    # a crossfade on a bus without a free slot raises and changes nothing
    with pkg.PcmMixer(1, 1, 1, 7) as busy:
        busy.set_routes(0, "swap")
        busy.set_gains(ONE, jump=True)
        before = busy.slots()
        with pytest.raises(ValueError):
            busy.crossfade(0, 0)
        after = busy.slots()
        assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1] == 0


def test_behind_the_sink_and_the_limiter_on_one_stream(pkg):
    """sink -> limiter -> mixer on one stream, no synchronisation between them: one bus that plays station 0, then crossfades to station 1.  The bus
    equals the host routine fed the limiter's output; before the fade it is station 0's PCM and behind it station 1's, bit for bit"""
    import torch
    ns, n, lw, slew = 2, 4800, 6, 32
    alpha, gain = pkg.load_library().sdrfm_pcm_alpha(48000.0, 75e-6), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))
    t = np.arange(3 * n) / 48000.0
    left = np.stack([(0.3 + 0.2 * s) * np.sin(2 * np.pi * (400.0 + 300 * s) * t) for s in range(ns)]).astype(np.float32)
    right = (left[::-1] * 0.7 + 0.02 * np.random.default_rng(54).standard_normal(left.shape)).astype(np.float32)
    stream = torch.cuda.Stream()
    with pkg.StereoPcmSink(ns, alpha, gain) as sink, pkg.PcmLimiter(ns, lw, 4) as lim, pkg.PcmMixer(ns, 1, 2, slew) as mixer:
        host = cases.HostMixer(pkg, ns, 1, 2, slew)
        for k in (sink, lim, mixer):
            k.set_stream(stream.cuda_stream)
        for k in (mixer, host):
            k.set_routes([[0, NONE]], 0)
            k.set_gains([[ONE, 0]], jump=True)
        d_l, d_r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        torch.cuda.synchronize()
        for c in range(3):
            if c == 1:
                assert mixer.crossfade(0, 1) == host.crossfade(0, 1) == 1
            pcm, limited = (torch.zeros((ns, 2 * n), dtype=torch.int16, device="cuda") for _ in range(2))
            bus = torch.zeros((1, 2 * n), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            sink.process_batch_device(d_l[:, c * n:(c + 1) * n], d_r[:, c * n:(c + 1) * n], pcm)
            lim.process_batch_device(pcm, limited)
            mixer.process_batch(limited, bus)
            mixer.synchronize()
            fed, got = limited.cpu().numpy(), bus.cpu().numpy()
            assert np.abs(fed).max() > 4000 and np.array_equal(got, host.process_batch(fed)) and host.holds(mixer), c
            if c == 0:
                assert np.array_equal(got[0], fed[0])
            elif c == 1:
                fade = pkg.fade_pairs(slew)
                assert fade == 1024 and np.array_equal(got[0, 2 * fade:], fed[1, 2 * fade:]) and not np.array_equal(got[0, :2 * fade], fed[1, :2 * fade])
            else:
                assert np.array_equal(got[0], fed[1])
        assert mixer.read().tobytes() == host.rec.tobytes()
