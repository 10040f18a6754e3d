"""The FM handle (sdrfm_create, sdrfm_process_batch) across row layouts and call forms.  Which kernel serves a device-pointer call depends on where the
caller's rows lie (csrc/sdrfm.hip: enqueue, csrc/sdrfm_fm_call.h): iq and iq_stride multiples of 16 -> design Q or S, of 4 only -> design B, anything
else -> the generic kernel; an overlapped call warms up from the previous call's buffer, whatever its stride, length and kernel were; design Q stores
8-byte pairs aligned in memory whatever the parity of the audio row.  Here: unaligned rows cut from a larger allocation with random bytes between them,
layouts that change under a running stream, overlapped calls behind a different previous call, canaries around odd-word audio rows for every design,
refused calls between valid ones, one stream with a short stride, and the PCM call on unaligned rows.

References: oracle.Oracle at TOL for every distinct row; the bit-exact kernels (generic, B, S) bit for bit across every layout and against the host-buffer
call; design Q bit for bit among its own calls and within 2e-6 of a bit_exact=True twin (the bound tests/test_route_gpu.py holds a take-over call to).
Every call asserts the first word of kernel_name against tests/fm_shape_cases.py, which tests/test_fm_shapes_cpu.py holds to the host arithmetic."""
import ctypes as C

import numpy as np
import pytest

import fm_shape_cases as fc
from conftest import scaled_err, TOL

pytestmark = pytest.mark.gpu

Q_TWIN = 2e-6                                                   # design Q against the bit-exact kernels (tests/test_route_gpu.py)
SETTLED = 8                                                     # audio outputs of a take-over call that still meet the other design's 31 discriminator outputs
SENT = -12345.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def _taps(pkg, T, D, Da):
    return pkg.default_config(T, fir_decim=D, audio_taps=32, audio_decim=Da)


def _rows12(pkg, nsamp, first_id):
    """12 distinct rows: 6 carriers, 4 of noise, one constant, one counter"""
    return np.concatenate([pkg.make_iq(6, nsamp, mode="fm", first_id=first_id), pkg.make_iq(4, nsamp, mode="random", first_id=first_id + 50),
                           pkg.make_iq(1, nsamp, mode="const", first_id=first_id + 90), pkg.make_iq(1, nsamp, mode="counter", first_id=first_id + 95)])


def _tiled(torch, rows12, ns):
    """(device, host) [ns, nbytes]: stream s holds row s % 12"""
    idx = np.arange(ns) % 12
    return torch.from_numpy(rows12).cuda()[torch.from_numpy(idx).cuda()].contiguous(), rows12[idx]


def _oracle(oracle_mod, h, g, D, Da, rows12):
    return [oracle_mod.Oracle(h, g, D=D, Da=Da).process(r) for r in rows12]


def _embed(torch, piece, cls, variant, seed):
    """`piece` [ns, nb] in rows cut from a larger uint8 allocation of random bytes at layout LAYOUTS[cls][variant]; the stride is topped up to the
    layout's residue mod 16 where nb is no whole number of 16-byte pieces.  Returns (the allocation, the rows)."""
    off, pad = fc.LAYOUTS[cls][variant % len(fc.LAYOUTS[cls])]
    ns, nb = piece.shape
    stride = nb + pad + (-nb) % 16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    buf = torch.randint(0, 256, (off + ns * stride + 256,), dtype=torch.uint8, device="cuda", generator=gen)
    rows = buf[off:off + ns * stride].view(ns, stride)
    rows[:, :nb] = piece
    assert buf.data_ptr() % 256 == 0 and fc.align_class(rows.data_ptr(), rows.stride(0)) == cls, (off, pad, stride)
    return buf, rows


def _demod(pkg, case, h, g, max_bytes, bit_exact=None, ns=None):
    return pkg.FmDemod(pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, fir_decim=case.D, audio_decim=case.Da, n_streams=ns or case.ns,
                                    bit_exact=case.bit_exact if bit_exact is None else bit_exact, max_bytes_per_call=max_bytes))


def _word(name):
    return name.split(" ")[0]


def _check_name(case, k, name):
    call = case.calls[k]
    assert _word(name) == call.expect, (case.name, k, name)
    assert ("overlapped" in name) == call.overlapped, (case.name, k, name)
    if call.mixed is None:
        assert "+" not in name, (case.name, k, name)
    else:
        assert "+" in name and "(%d streams)" % case.n_routed in name and ("in one launch" in name) == (call.mixed == "one"), (case.name, k, name)


def _run(torch, dm, case, feeds, host_np, flags=True, audio=None, route=None):
    """The case's calls on dm.  feeds[k]: device rows holding call k's bytes from column 0 (None for a host-buffer call, which takes host_np[k]); audio[k]:
    where call k's audio goes (default: a fresh contiguous tensor).  Returns ([audio of call k as numpy], [kernel names])."""
    DDa = case.D * case.Da
    if audio is None:
        audio = [torch.zeros((case.ns, max(c.nsamp // DDa, 1)), dtype=torch.float32, device="cuda") for c in case.calls]
    torch.cuda.synchronize()                                     # (the fills ran on torch's stream, the calls run on the handle's)
    outs, names = [], []
    for k, c in enumerate(case.calls):
        if k == case.route_at and route is not None:
            assert np.array_equal(dm.route(route), route)
        if c.device:
            n = dm.process_batch_device(feeds[k], audio[k], nbytes=2 * c.nsamp, overlap=bool(c.overlap and flags))
            outs.append(n)
        else:
            outs.append(dm.process_batch(host_np[k]))
        names.append(dm.kernel_name)
    dm.synchronize()
    torch.cuda.synchronize()
    outs = [audio[k][:, :o].cpu().numpy() if isinstance(o, int) else o for k, o in enumerate(outs)]
    return outs, names


def _hold_to_oracle(got, want12, where):
    """got [ns, A]: every distinct row within TOL of the oracle, every copy of a row the same bits.  Returns the worst scaled error."""
    worst = 0.0
    for r in range(min(12, got.shape[0])):
        e = scaled_err(got[r], want12[r][:got.shape[1]])
        assert e <= TOL, (where, r, e)
        worst = max(worst, e)
    idx = np.arange(got.shape[0]) % 12
    assert np.array_equal(_bits(got), _bits(got[idx])), (where, "copies of a row differ")
    return worst


# ---- 1. row alignment selects the kernel and never changes the audio ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", fc.GEOMS, ids=["T%d-D%d-Da%d" % g for g in fc.GEOMS])
def test_row_alignment_selects_the_kernel_and_never_changes_the_audio(pkg, oracle_mod, geom):
    import torch
    T, D, Da = geom
    ns, sizes = fc.align_shape(T, D, Da)
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    h, g = _taps(pkg, T, D, Da)
    rows12 = _rows12(pkg, total, 11000 + 100 * T + D)
    dev, host = _tiled(torch, rows12, ns)
    want = _oracle(oracle_mod, h, g, D, Da, rows12)
    tag = "T%d-D%d-Da%d" % geom
    got, reached = {}, set()
    any_case = fc.by_name("align-%s-q-al16" % tag)
    with _demod(pkg, any_case, h, g, 2 * max(sizes), bit_exact=False) as dq, _demod(pkg, any_case, h, g, 2 * max(sizes), bit_exact=True) as dx:
        x_host = np.concatenate([dx.process_batch(host[:, 2 * cuts[k]:2 * cuts[k + 1]]) for k in range(3)], axis=1)
        for cls, layouts in fc.LAYOUTS.items():
            for v, (off, pad) in enumerate(layouts):
                buf, rows = _embed(torch, dev, cls, v, 7 * off + pad)
                assert (rows.data_ptr() - buf.data_ptr(), rows.stride(0) - dev.shape[1]) == (off, pad)
                feeds = [rows[:, 2 * cuts[k]:] for k in range(3)]
                for dm, kind in ((dq, "q"), (dx, "x")):
                    case = fc.by_name("align-%s-%s-al%d" % (tag, kind, cls))
                    dm.reset()
                    outs, names = _run(torch, dm, case, feeds, None)
                    for k, name in enumerate(names):
                        _check_name(case, k, name)
                        reached.add(_word(name))
                    got[kind, off, pad] = np.concatenate(outs, axis=1)
                del buf, rows, feeds
    worst = 0.0
    q16 = [got["q", o, p] for o, p in fc.LAYOUTS[16]]
    for (kind, off, pad), a in got.items():
        cls = next(c for c, ls in fc.LAYOUTS.items() if (off, pad) in ls)
        assert a.shape == x_host.shape
        if kind == "x" or cls != 16:                              # the bit-exact kernels: one answer, the host-buffer call's
            assert np.array_equal(_bits(a), _bits(x_host)), (kind, off, pad, int(np.argmax((_bits(a) != _bits(x_host)).any(axis=0))))
        else:                                                     # design Q: bit for bit among its aligned layouts, within 2e-6 of the twin
            assert np.array_equal(_bits(a), _bits(q16[0])), (off, pad)
            assert _rel(a, x_host) <= Q_TWIN, (off, pad, _rel(a, x_host))
        worst = max(worst, _hold_to_oracle(a, want, (kind, off, pad)))
    print("fm shapes 1 (%s, %d streams x %s samples, 11 layouts): %s; design Q within %.3g of its twin; worst scaled error %.3g" % (
        tag, ns, "/".join(str(s) for s in sizes), " ".join(sorted(reached)), _rel(q16[0], x_host), worst))


# ---- 2. layout changes under a running stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in fc.switch_cases()])
def test_layout_changes_under_a_running_stream(pkg, oracle_mod, name):
    import torch
    case = fc.by_name(name)
    sizes = [c.nsamp for c in case.calls]
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum([c.nsamp for c in case.calls])])
    h, g = _taps(pkg, case.T, case.D, case.Da)
    rows12 = _rows12(pkg, total, 12000 + case.ns)
    dev, host = _tiled(torch, rows12, case.ns)
    want = _oracle(oracle_mod, h, g, case.D, case.Da, rows12)
    copies = {cls: _embed(torch, dev, cls, len(fc.LAYOUTS[cls]) - 1, 31 + cls) for cls in (16, 4, 1)}
    feeds = [copies[c.cls][1][:, 2 * cuts[k]:] if c.device else None for k, c in enumerate(case.calls)]
    host_np = [host[:, 2 * cuts[k]:2 * cuts[k + 1]] for k in range(len(sizes))]
    plain = case._replace(calls=tuple(fc.Call(c.nsamp, 16, expect=fc.expect_word(16, case.bit_exact)) for c in case.calls))
    plain_feeds = [dev[:, 2 * cuts[k]:] for k in range(len(sizes))]
    with _demod(pkg, case, h, g, 2 * max(sizes)) as dm:
        outs, names = _run(torch, dm, case, feeds, host_np)
    for k, nm in enumerate(names):
        _check_name(case, k, nm)
    with _demod(pkg, case, h, g, 2 * max(sizes)) as same:          # the same handle kind on contiguous aligned rows throughout
        own, own_names = _run(torch, same, plain, plain_feeds, None)
    assert all(_word(n) == plain.calls[0].expect for n in own_names), own_names
    with _demod(pkg, case, h, g, 2 * max(sizes), bit_exact=True) as tw:
        twin, _ = _run(torch, tw, plain, plain_feeds, None)
    got, twin_all = np.concatenate(outs, axis=1), np.concatenate(twin, axis=1)
    worst = _hold_to_oracle(got, want, name)
    assert _rel(got, twin_all) <= Q_TWIN, _rel(got, twin_all)
    if case.bit_exact:
        assert np.array_equal(_bits(got), _bits(np.concatenate(own, axis=1))) and np.array_equal(_bits(got), _bits(twin_all))
    else:
        for k, c in enumerate(case.calls):
            ref = own[k] if c.expect == "fast-q" else twin[k]      # design Q's calls against design Q alone, the others against the bit-exact twin
            took_over = k > 0 and (c.expect == "fast-q") != (case.calls[k - 1].expect == "fast-q")
            lo = SETTLED if took_over else 0                       # (a take-over call meets the other design's last 31 discriminator outputs)
            assert outs[k].shape[1] > SETTLED
            assert np.array_equal(_bits(outs[k][:, lo:]), _bits(ref[:, lo:])), (name, k, c.expect, lo)
    print("fm shapes 2 (%s, %d streams x %d samples): %s; within %.3g of the bit-exact twin; worst scaled error %.3g" % (
        name, case.ns, sizes[0], " ".join(_word(n) for n in names), _rel(got, twin_all), worst))


# ---- 3. overlapped calls behind a different previous call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in fc.overlap_cases()])
def test_overlapped_calls_behind_a_different_previous_call(pkg, oracle_mod, name):
    import torch
    case = fc.by_name(name)
    sizes = [c.nsamp for c in case.calls]
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    h, g = _taps(pkg, case.T, case.D, case.Da)
    rows12 = _rows12(pkg, total, 13000 + len(name))
    dev, host = _tiled(torch, rows12, case.ns)
    want = _oracle(oracle_mod, h, g, case.D, case.Da, rows12)
    # every call's bytes in an allocation of its own (the previous call's rows stay intact), consecutive calls at different layouts of their class:
    # another offset, another stride
    held = [_embed(torch, dev[:, 2 * cuts[k]:2 * cuts[k + 1]], c.cls, k, 50 + k) if c.device else None for k, c in enumerate(case.calls)]
    feeds = [b[1] if b else None for b in held]
    host_np = [host[:, 2 * cuts[k]:2 * cuts[k + 1]] for k in range(len(sizes))]
    route = np.array([1 if s % 4 == 2 else 0 for s in range(case.ns)], dtype=np.uint8) if case.n_routed else None
    assert route is None or int(route.sum()) == case.n_routed
    with _demod(pkg, case, h, g, 2 * max(sizes)) as dm, _demod(pkg, case, h, g, 2 * max(sizes)) as ref:
        outs, names = _run(torch, dm, case, feeds, host_np, route=route)
        serial, serial_names = _run(torch, ref, case, feeds, host_np, flags=False, route=route)
    for k, nm in enumerate(names):
        _check_name(case, k, nm)
        assert _word(serial_names[k]) == case.calls[k].expect and "overlapped" not in serial_names[k], (k, serial_names[k])
        assert np.array_equal(_bits(outs[k]), _bits(serial[k])), (name, k, nm)
    worst = _hold_to_oracle(np.concatenate(outs, axis=1), want, name)
    print("fm shapes 3 (%s, %d streams): %s; bitwise the serial calls; worst scaled error %.3g" % (
        name, case.ns, ", ".join(_word(n) + ("*" if "overlapped" in n else "") for n in names), worst))


# ---- 4. canaries and odd-word audio rows for every design --------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["even-rows", "odd-rows"])
@pytest.mark.parametrize("name", [c.name for c in fc.canary_cases()])
def test_every_design_writes_only_its_audio_on_even_and_odd_word_rows(pkg, oracle_mod, name, odd):
    import torch
    case = fc.by_name(name)
    sizes = [c.nsamp for c in case.calls]
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    DDa = case.D * case.Da
    h, g = pkg.default_config(case.T) if case.T == 48 else _taps(pkg, case.T, case.D, case.Da)
    rows12 = _rows12(pkg, total, 14000 + case.ns + case.T)
    dev, host = _tiled(torch, rows12, case.ns)
    want = _oracle(oracle_mod, h, g, case.D, case.Da, rows12)
    cls = case.calls[0].cls
    held = _embed(torch, dev, cls, len(fc.LAYOUTS[cls]) - 1, 77) if cls != 16 else (None, dev)
    feeds = [held[1][:, 2 * cuts[k]:] for k in range(len(sizes))]   # views of one capture, as tests/test_route_gpu.py feeds its overlapped calls
    route = np.array([1 if s % 4 == 2 else 0 for s in range(case.ns)], dtype=np.uint8) if case.n_routed else None
    assert route is None or int(route.sum()) == case.n_routed
    pad = 63 if odd else 64
    bigs, views, geo = [], [], []
    for n in sizes:
        A = n // DDa
        stride = A + 37
        stride += (stride % 2) != int(odd)                        # both even, or both odd: rows start on odd floats and every second row flips parity
        big = torch.full((pad + case.ns * stride + 64,), SENT, dtype=torch.float32, device="cuda")
        assert big.data_ptr() % 8 == 0
        bigs.append(big), views.append(big[pad:pad + case.ns * stride].view(case.ns, stride)), geo.append((A, stride))
    with _demod(pkg, case, h, g, 2 * max(sizes)) as dm:
        outs, names = _run(torch, dm, case, feeds, None, audio=views, route=route)
        dm.reset()
        plain, plain_names = _run(torch, dm, case, feeds, None, route=route)
    assert names == plain_names
    for k, nm in enumerate(names):
        _check_name(case, k, nm)
        A, stride = geo[k]
        hostbuf = bigs[k].cpu().numpy()
        assert np.all(hostbuf[:pad] == SENT) and np.all(hostbuf[pad + case.ns * stride:] == SENT), (name, k, "wrote outside the rows")
        rows = hostbuf[pad:pad + case.ns * stride].reshape(case.ns, stride)
        assert outs[k].shape[1] == A
        assert np.all(rows[:, A:] == SENT), (name, k, "wrote past the audio of a stream", np.argwhere(rows[:, A:] != SENT)[:4])
        assert not np.any(rows[:, :A] == SENT), (name, k, "left audio unwritten", np.argwhere(rows[:, :A] == SENT)[:4])
        assert np.array_equal(_bits(rows[:, :A]), _bits(plain[k])), (name, k)
    got = np.concatenate(outs, axis=1)
    worst = _hold_to_oracle(got, want, name)                      # (copies of a row share their side of the assignment: s % 4 == s % 12 % 4)
    print("fm shapes 4 (%s, %s, %d streams): %s; nothing outside [0, A) of a row, bitwise the contiguous buffer; worst scaled error %.3g" % (
        name, "odd-word rows" if odd else "even-word rows", case.ns, " | ".join(names), worst))


# ---- 5. refused calls leave the stream untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in fc.refusal_cases()])
def test_refused_calls_leave_the_stream_untouched(pkg, oracle_mod, name):
    import torch
    case = fc.by_name(name)
    sizes = [c.nsamp for c in case.calls]
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    DDa = case.D * case.Da
    h, g = _taps(pkg, case.T, case.D, case.Da)
    rows12 = _rows12(pkg, total, 15000 + case.ns)
    dev, host = _tiled(torch, rows12, case.ns)
    want = _oracle(oracle_mod, h, g, case.D, case.Da, rows12)
    feeds = [dev[:, 2 * cuts[k]:] for k in range(len(sizes))]
    cap = 2 * max(sizes)
    lib, L = pkg.load_library(), pkg.lib
    big_host = np.zeros((case.ns, cap + 2), np.uint8)
    host_audio = np.zeros((case.ns, cap // (2 * DDa) + 2), np.float32)
    scratch = torch.full((case.ns, max(sizes) // DDa + 2), SENT, dtype=torch.float32, device="cuda")
    refused = []

    def refuse_all(dm, k):
        nb = 2 * sizes[k]
        A = dm.audio_count(nb)
        n = C.c_uint32()
        d_iq, d_au = C.c_void_p(feeds[k].data_ptr()), C.c_void_p(scratch.data_ptr())
        h_iq, h_au = big_host.ctypes.data_as(C.c_void_p), host_audio.ctypes.data_as(C.c_void_p)
        for what, want_rc, args in (
                ("audio_stride < A", L.ECAPACITY, (d_iq, dev.stride(0), nb, d_au, A - 1, C.byref(n), L.F_DEVICE_PTRS)),
                ("iq_stride < nbytes", L.ECAPACITY, (d_iq, nb - 2, nb, d_au, scratch.stride(0), C.byref(n), L.F_DEVICE_PTRS)),
                ("nbytes over the capacity", L.ECAPACITY, (h_iq, big_host.strides[0], cap + 2, h_au, host_audio.shape[1], C.byref(n), 0)),
                ("odd byte count", L.EODD, (d_iq, dev.stride(0), nb + 1, d_au, scratch.stride(0), C.byref(n), L.F_DEVICE_PTRS)),
                ("SDRFM_F_OVERLAP without SDRFM_F_DEVICE_PTRS", L.EINVAL, (h_iq, big_host.strides[0], nb, h_au, host_audio.shape[1], C.byref(n), L.F_OVERLAP))):
            rc = lib.sdrfm_process_batch(dm._h, *args)
            assert rc == want_rc, (name, k, what, rc)
            refused.append(what)
        assert dm.audio_count(nb) == A

    with _demod(pkg, case, h, g, cap) as dm, _demod(pkg, case, h, g, cap) as ref:
        want_runs, want_names = _run(torch, ref, case, feeds, None)
        audio = [torch.zeros((case.ns, n // DDa), dtype=torch.float32, device="cuda") for n in sizes]
        torch.cuda.synchronize()
        outs, names = [], []
        for k, c in enumerate(case.calls):
            refuse_all(dm, k)
            n = dm.process_batch_device(feeds[k], audio[k], nbytes=2 * c.nsamp)
            names.append(dm.kernel_name)
            outs.append((k, n))
        refuse_all(dm, len(sizes) - 1)
        dm.synchronize()
        torch.cuda.synchronize()
    assert names == want_names
    for k, n in outs:
        _check_name(case, k, names[k])
        assert np.array_equal(_bits(audio[k][:, :n].cpu().numpy()), _bits(want_runs[k])), (name, k)
    assert bool((scratch == SENT).all())                          # no refused call wrote audio
    worst = _hold_to_oracle(np.concatenate(want_runs, axis=1), want, name)
    print("fm shapes 5 (%s, %d streams): %d refused calls (%s) between %s; bitwise the uninterrupted run; worst scaled error %.3g" % (
        name, case.ns, len(refused), "; ".join(sorted(set(refused))), " ".join(_word(n) for n in names), worst))


# ---- 6. one stream ----------------------------------------------------------------------------------------------------------------------------------
def test_one_stream_with_a_short_stride_at_three_offsets(pkg, oracle_mod):
    import torch
    nsamp, nb = fc.ONE_NSAMP, 2 * fc.ONE_NSAMP
    h, g = _taps(pkg, 64, 10, 5)
    row = pkg.make_iq(1, nsamp, mode="fm", first_id=16000)
    want = oracle_mod.Oracle(h, g, D=10, Da=5).process(row[0])
    A = nsamp // 50
    drow = torch.from_numpy(row[0]).cuda()
    lib = pkg.load_library()
    one = fc.by_name("one-off0-stride0-q")
    reached, worst, q_twin = [], 0.0, 0.0
    with _demod(pkg, one, h, g, nb, bit_exact=False) as dq, _demod(pkg, one, h, g, nb, bit_exact=True) as dx:
        x_host, q_host = dx.process_batch(row), dq.process_batch(row)
        assert _word(dq.kernel_name) == "fast-q" and _word(dx.kernel_name) == "fast-b", (dq.kernel_name, dx.kernel_name)
        assert x_host.shape == (1, A) and _rel(q_host, x_host) <= Q_TWIN
        for off in fc.ONE_OFFSETS:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(off)
            buf = torch.randint(0, 256, (nb + 256,), dtype=torch.uint8, device="cuda", generator=gen)
            buf[off:off + nb] = drow
            for stride in (0, 2):
                for dm, kind in ((dq, "q"), (dx, "x")):
                    case = fc.by_name("one-off%d-stride%d-%s" % (off, stride, kind))
                    audio = torch.full((1, A + 3), SENT, dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    dm.reset()
                    n = C.c_uint32()
                    rc = lib.sdrfm_process_batch(dm._h, C.c_void_p(buf.data_ptr() + off), stride, nb, C.c_void_p(audio.data_ptr()), 0, C.byref(n),
                                                 pkg.lib.F_DEVICE_PTRS)
                    assert rc == pkg.lib.OK and n.value == A, (rc, n.value)
                    dm.synchronize()
                    _check_name(case, 0, dm.kernel_name)
                    reached.append(_word(dm.kernel_name))
                    a = audio.cpu().numpy()
                    assert np.all(a[:, A:] == SENT)
                    a = a[:, :A]
                    if _word(dm.kernel_name) == "fast-q":
                        assert np.array_equal(_bits(a), _bits(q_host)), (off, stride)
                        q_twin = max(q_twin, _rel(a, x_host))
                        assert q_twin <= Q_TWIN
                    else:
                        assert np.array_equal(_bits(a), _bits(x_host)), (off, stride, kind, dm.kernel_name)
                    e = scaled_err(a[0], want)
                    assert e <= TOL, (off, stride, kind, e)
                    worst = max(worst, e)
    print("fm shapes 6 (one stream x %d samples, offsets 0 / 4 / 6, iq_stride 0 and 2): %s; design Q within %.3g of its twin; worst scaled error %.3g" % (
        nsamp, " ".join(reached), q_twin, worst))


# ---- 7. the PCM call on unaligned input rows ---------------------------------------------------------------------------------------------------------
def test_the_pcm_call_on_unaligned_input_rows(pkg, oracle_mod):
    """The sink's EXACT form (bit for bit the host routine) is NOT held here and cannot be: sdrfm_process_batch_pcm takes no SDRFM_PCM_F_EXACT, it serves its
    PCM by the sink's default form only (the chain inside design Q's launch, or the sink's own blocked scan behind any other kernel).  That form is held to 1 LSB of the host routine over the bit-exact twin's audio, the state carried by the host routine across all calls — a sink state
    lost at a switch between the two paths would be whole LSBs off at the next call's first samples (the carriers' audio has a DC offset)."""
    import torch
    case = fc.by_name("pcm-switch")
    sizes = [c.nsamp for c in case.calls]
    total, cuts = sum(sizes), np.concatenate([[0], np.cumsum(sizes)])
    na = fc.PCM_NSAMP // 50
    h, g = _taps(pkg, case.T, case.D, case.Da)
    lib = pkg.load_library()
    alpha, gain = lib.sdrfm_pcm_alpha(48000.0, 75e-6), np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3))
    rows12 = _rows12(pkg, total, 17000)
    dev, host = _tiled(torch, rows12, case.ns)
    want = _oracle(oracle_mod, h, g, case.D, case.Da, rows12)
    copies = {cls: _embed(torch, dev, cls, len(fc.LAYOUTS[cls]) - 1, 91 + cls) for cls in (16, 4, 1)}
    audio = [torch.zeros((case.ns, na), dtype=torch.float32, device="cuda") for _ in sizes]
    pcm = [torch.full((case.ns, 2 * na + 6), 12345, dtype=torch.int16, device="cuda") for _ in sizes]
    torch.cuda.synchronize()
    names = []
    with _demod(pkg, case, h, g, 2 * max(sizes)) as dm, pkg.PcmSink(case.ns, alpha, gain) as sink:
        for k, c in enumerate(case.calls):
            assert dm.process_batch_pcm_device(sink, copies[c.cls][1][:, 2 * cuts[k]:], audio[k], pcm[k], nbytes=2 * c.nsamp) == na
            names.append(dm.kernel_name)
        dm.synchronize()
        torch.cuda.synchronize()
    for k, (c, nm) in enumerate(zip(case.calls, names)):
        assert _word(nm) == c.expect, (k, nm)
        assert nm.endswith("+ pcm") == (c.cls == 16 and k > 0), (k, nm)   # aligned rows: the chain in design Q's launch (never at a stream's first call); else the sink's own kernel follows
    plain = case._replace(bit_exact=True, calls=tuple(fc.Call(c.nsamp, 16, expect="fast-b") for c in case.calls))
    with _demod(pkg, plain, h, g, 2 * max(sizes)) as tw:
        twin, _ = _run(torch, tw, plain, [dev[:, 2 * cuts[k]:] for k in range(len(sizes))], None)
    got_audio = [a.cpu().numpy() for a in audio]
    got_pcm = [p.cpu().numpy() for p in pcm]
    worst = _hold_to_oracle(np.concatenate(got_audio, axis=1), want, "pcm-switch")
    assert _rel(np.concatenate(got_audio, axis=1), np.concatenate(twin, axis=1)) <= Q_TWIN
    worst_lsb = 0
    for s in range(12):
        st = 0.0
        for k in range(len(sizes)):
            ref, st = pkg.pcm_deemph_s16_host(twin[k][s], alpha, gain, st)
            d = np.abs(got_pcm[k][s, :2 * na].astype(np.int32) - ref.astype(np.int32))
            assert d.max() <= 1, (s, k, names[k], int(d.max()), int(np.argmax(d)))
            worst_lsb = max(worst_lsb, int(d.max()))
            assert (got_pcm[k][s, 2 * na:] == 12345).all(), (s, k)
    print("fm shapes 7 (pcm call, %d streams x %d samples): %s; PCM within %d LSB of the host routine over the bit-exact twin's audio; worst scaled error %.3g" % (
        case.ns, fc.PCM_NSAMP, " | ".join(_word(n) + (" + pcm" if n.endswith("+ pcm") else "") for n in names), worst_lsb, worst))
