"""GPU sweep of the spectrum view (sdrfm_spectrum_*) over the sizes, frame counts, windows and call forms that select and steer its two
kernels: k_spectrum<log2 N> at all seven sizes over its own round geometry, the bytes behind the last whole frame, six windows (two of
them asymmetric), long averages and more streams than the machine holds at a time on k_spectrum_chain, 2048 / 4096 points through every
call form, one handle alternating between the kernels, and the refusals.  Every comparison is bit for bit against
oracle_mod.SpectrumOracle: there is no tolerance in this file.

The helpers that build a case (`case_counts`, `case_rows`, `make_window`, `tail_case`, `tiled_rows`) take no device, so the oracle side of
the sweep runs on a CPU-only machine (tests/test_spectrum_oracle.py does that)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
# Round geometry of k_spectrum<log2 N>, from spec_logb / spec_nwf in csrc/sdrfm_spectrum.hip: a wave's block is max(N, 1024) points =
# FPW frames (spec_logb), a workgroup has NWF waves (spec_nwf), a round is FPR = FPW NWF frames.   nfft: (FPW, NWF, FPR)
GEOMETRY = {64: (16, 16, 256), 128: (8, 16, 128), 256: (4, 16, 64), 512: (2, 8, 16), 1024: (1, 8, 8), 2048: (1, 8, 8), 4096: (1, 4, 4)}
CHAIN_SIZES = tuple(n for n in SIZES if n <= 1024)               # k_spectrum_chain serves these when iq and iq_stride are even
CLASSES = ("fm", "random", "counter")
WINDOWS = ("rect", "noise", "hann_holes", "hann_tiny", "hann_huge", "ramp")


def fpw(nfft):
    return GEOMETRY[nfft][0]


def fpr(nfft):
    return GEOMETRY[nfft][2]


def hann(nfft):
    """the periodic Hann window as the library computes it: in double, rounded to fp32"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)


def make_window(name, nfft):
    """the six windows of the sweep.  `noise` and `ramp` are not symmetric about N/2 (periodic Hann and the rectangle are), and every value
    of `ramp` is distinct: a kernel that reads win[n] at another n cannot pass on them."""
    rng = np.random.default_rng(4000 + nfft)
    if name == "rect":
        return np.ones(nfft, np.float32)
    if name == "noise":
        return rng.standard_normal(nfft).astype(np.float32)      # signed
    if name == "hann_holes":
        w = hann(nfft)
        w[rng.permutation(nfft)[:nfft // 2]] = 0.0
        return w
    if name == "hann_tiny":
        return (hann(nfft).astype(np.float64) * 1e-20).astype(np.float32)
    if name == "hann_huge":
        return (hann(nfft).astype(np.float64) * 1e6).astype(np.float32)
    if name == "ramp":
        w = ((np.arange(nfft) + 1.0) / nfft).astype(np.float32)
        assert np.unique(w).size == nfft
        return w
    raise ValueError(name)


def case_counts(nfft):
    """frame counts around the blocks and rounds of k_spectrum<log2 N> and around the eight-at-a-time leg of its frame sum"""
    w, r = fpw(nfft), fpr(nfft)
    return sorted(set(c for c in (1, 2, 7, 8, 9, w - 1, w, w + 1, r - 1, r, r + 1, r + 8, r + 9, 2 * r - 1, 2 * r, 2 * r + 1, 3 * r + 5) if c > 0))


def case_rows(pkg, nfft, F, ns, first_id, extra=7, classes=CLASSES):
    """ns streams of F frames and `extra` samples behind them, the input classes in turn -> uint8 [ns, 2 (F nfft + extra)]"""
    return np.stack([pkg.make_iq(1, F * nfft + extra, mode=classes[s % len(classes)], first_id=first_id + s)[0] for s in range(ns)])


def oracle_rows(oracle_mod, nfft, iq, window=None, frames=None):
    """the oracle's power of every row of iq (its frame count checked against `frames`) -> float32 [ns, nfft]"""
    o = oracle_mod.SpectrumOracle(nfft, window)
    out = []
    for row in iq:
        p, f = o.process(row)
        assert frames is None or f == frames, (nfft, f, frames)
        out.append(p)
    o.close()
    return np.stack(out)


TAIL_FILLS = ("zeros", "ones", "random")


def tail_frames(nfft):
    """F = 4 FPW + 1: the last block of a wave holds one frame of the call and FPW - 1 behind it (N >= 1024: an odd count, no multiple of
    the chained kernel's run of two blocks nor of a round)"""
    return 4 * fpw(nfft) + 1


def tail_case(pkg, nfft, offset, stride_extra, fill, ns=3):
    """Rows of tail_frames(nfft) frames at byte `offset` of a buffer, row stride 2 F N + pad; the pad of every row (more than a block of
    1024 points, so whatever a wave computes past F comes from there) and 64 bytes before and behind the batch hold `fill`.
    -> (buffer bytes, offset of row 0 in it, stride, nbytes, the rows)"""
    F = tail_frames(nfft)
    nbytes = 2 * F * nfft
    stride = nbytes + 2048 + 38 + stride_extra
    rows = case_rows(pkg, nfft, F, ns, 5000 + nfft, extra=0)
    total = 64 + offset + ns * stride + 64
    if fill == "zeros":
        buf = np.zeros(total, np.uint8)
    elif fill == "ones":
        buf = np.full(total, 255, np.uint8)
    else:
        buf = np.random.default_rng(77 + nfft + offset).integers(0, 256, total, dtype=np.uint8)
    for s in range(ns):
        buf[64 + offset + s * stride:64 + offset + s * stride + nbytes] = rows[s]
    return buf, 64 + offset, stride, nbytes, rows


def tiled_rows(pkg, nfft, F, ns, first_id, distinct=12):
    """`distinct` different rows tiled to ns streams (the oracle leg stays short) -> (uint8 [ns, 2 F nfft], the distinct rows)"""
    rows = case_rows(pkg, nfft, F, distinct, first_id, extra=0, classes=("fm", "random") * 5 + ("counter", "const"))   # (a counter or const row is the same whatever its id)
    assert len({r.tobytes() for r in rows}) == distinct
    return np.tile(rows, ((ns + distinct - 1) // distinct, 1))[:ns], rows


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _aligned(torch, nbytes_total):
    """a device byte buffer whose address is a multiple of 4 (the allocator's blocks are 512-byte aligned; asserted, since the address
    parity selects the kernel)"""
    buf = torch.zeros(nbytes_total, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf


def _place(torch, iq, offset, stride):
    """iq [ns, nbytes] as device rows at byte `offset` of a zeroed buffer, `stride` bytes apart -> the [ns, nbytes] view"""
    ns, nbytes = iq.shape
    assert stride >= nbytes
    buf = _aligned(torch, offset + ns * stride + 8)
    view = buf[offset:offset + ns * stride].view(ns, stride)[:, :nbytes]
    view.copy_(torch.from_numpy(iq))
    assert view.data_ptr() % 4 == offset % 4 and view.stride(0) == stride
    return view


def _power(torch, ns, nfft, pad=5):
    """padded power rows holding -1: what a call leaves of them behind column nfft must stay -1"""
    return torch.full((ns, nfft + pad), -1.0, dtype=torch.float32, device="cuda")


def _check_power(power, nfft, want, where):
    got = power.cpu().numpy()
    assert np.array_equal(_bits(got[:, :nfft]), _bits(want)), where
    assert np.all(got[:, nfft:] == -1.0), where


def _chain_name(nfft):
    return "k_spectrum_chain<%d, 12, 2>" % int(np.log2(nfft))


def _typed_name(nfft):
    return "k_spectrum<%d>" % int(np.log2(nfft))


def _call(pkg, sv, iq_ptr, iq_stride, nbytes, power_ptr, power_stride, flags):
    """sdrfm_spectrum_process_batch on raw addresses (strides and flags the wrapper cannot express) -> (status, frames)"""
    n = C.c_uint32()
    rc = pkg.load_library().sdrfm_spectrum_process_batch(sv._h, C.c_void_p(iq_ptr), int(iq_stride), int(nbytes), C.c_void_p(power_ptr),
                                                         int(power_stride), C.byref(n), int(flags))
    return rc, n.value


# ---- a. k_spectrum<log2 N> at all seven sizes, over its own frame counts ------------------------------------------------------------------
@pytest.mark.parametrize("nfft", SIZES)
def test_typed_load_kernel_over_its_rounds(pkg, oracle_mod, nfft):
    """Frame counts below, at and above a wave's block, a round, two rounds and the eight-at-a-time leg of the frame sum; 3 streams of
    different classes, 7 samples behind the last frame; an odd iq with an even stride and an even iq with an odd stride (up to 1024 points
    that is what selects k_spectrum; 2048 / 4096 points run it anyway)."""
    import torch
    counts, ns = case_counts(nfft), 3
    assert counts[-1] == 3 * fpr(nfft) + 5
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=2 * (counts[-1] * nfft + 7)))
    for F in counts:
        iq = case_rows(pkg, nfft, F, ns, 2000 + 7 * F)
        want = oracle_rows(oracle_mod, nfft, iq, frames=F)
        for offset, stride_extra in ((1, 4), (0, 5)):
            view = _place(torch, iq, offset, iq.shape[1] + stride_extra)
            assert (view.data_ptr() | view.stride(0)) & 1
            power = _power(torch, ns, nfft)
            torch.cuda.synchronize()
            assert sv.process_batch_device(view, power) == F
            assert sv.kernel_name == _typed_name(nfft)
            sv.synchronize()
            _check_power(power, nfft, want, (nfft, F, offset, stride_extra))
    sv.close()


# ---- b. what lies behind the last whole frame has no effect -----------------------------------------------------------------------------
def _tail_forms(nfft):
    """(kernel, byte offset of row 0 mod 4, extra stride): both kernels; iq = 2 mod 4 for the chained one (its descriptor is rounded out
    over two bytes before and two behind the batch)"""
    if nfft <= 1024:
        return (("chain", 0, 0), ("chain", 2, 0), ("typed", 1, 0), ("typed", 0, 1))
    return (("typed", 0, 0), ("typed", 1, 0), ("typed", 2, 1))


@pytest.mark.parametrize("nfft", SIZES)
def test_bytes_behind_the_last_frame_have_no_effect(pkg, oracle_mod, nfft):
    """Both kernels transform the frames past F that a wave's last block holds and must not sum them.  The same call with the pad of every
    row and 64 bytes around the batch filled with 0, with 255 and with random bytes: three times the same bits, and the oracle's."""
    import torch
    ns, F = 3, tail_frames(nfft)
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=2 * F * nfft))
    for kernel, offset, stride_extra in _tail_forms(nfft):
        want, first = None, None
        for fill in TAIL_FILLS:
            host, at, stride, nbytes, rows = tail_case(pkg, nfft, offset, stride_extra, fill, ns)
            if want is None:
                want = oracle_rows(oracle_mod, nfft, rows, frames=F)
            buf = _aligned(torch, host.size)
            buf.copy_(torch.from_numpy(host))
            view = buf[at:at + ns * stride].view(ns, stride)[:, :nbytes]
            assert view.stride(0) == stride > nbytes and view.data_ptr() % 4 == at % 4 == offset % 4
            power = _power(torch, ns, nfft)
            torch.cuda.synchronize()
            assert sv.process_batch_device(view, power) == F
            assert sv.kernel_name == (_chain_name(nfft) if kernel == "chain" else _typed_name(nfft))
            sv.synchronize()
            _check_power(power, nfft, want, (nfft, kernel, offset, stride_extra, fill))
            got = power.cpu().numpy()
            first = got if first is None else first
            assert np.array_equal(_bits(got), _bits(first)), (nfft, kernel, offset, fill)
    sv.close()


# ---- c. windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", SIZES)
def test_windows_on_both_kernels(pkg, oracle_mod, nfft):
    import torch
    ns, F = 2, 3 * fpw(nfft) + 1
    iq = case_rows(pkg, nfft, F, ns, 6000 + nfft)
    forms = ((0, 0), (1, 0)) if nfft <= 1024 else ((0, 0),)     # (offset, extra stride): the chained kernel, the typed-load kernel
    views = [_place(torch, iq, off, iq.shape[1] + ex) for off, ex in forms]
    default = oracle_rows(oracle_mod, nfft, iq, frames=F)
    for name in WINDOWS + ("hann", None):
        win = hann(nfft) if name == "hann" else (None if name is None else make_window(name, nfft))
        want = oracle_rows(oracle_mod, nfft, iq, win, frames=F)
        assert np.all(np.isfinite(want)) and want.max() > 0
        if name in ("hann", None):                               # the explicit Hann == window=None
            assert np.array_equal(_bits(want), _bits(default))
        sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, window=win, n_streams=ns, max_bytes_per_call=iq.shape[1]))
        for (off, ex), view in zip(forms, views):
            power = _power(torch, ns, nfft)
            torch.cuda.synchronize()
            assert sv.process_batch_device(view, power) == F
            assert sv.kernel_name == (_chain_name(nfft) if nfft <= 1024 and not off else _typed_name(nfft))
            sv.synchronize()
            _check_power(power, nfft, want, (nfft, name, off))
        sv.close()


# ---- d. long averages and many streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,F", [(64, 8191), (1024, 2048)])
def test_long_averages_on_the_chained_kernel(pkg, oracle_mod, nfft, F):
    """thousands of hand-overs of the running sum (64 points: one call of 1 MiB per stream), four streams, each against the oracle"""
    ns = 4
    iq = case_rows(pkg, nfft, F, ns, 7000 + nfft, extra=0, classes=("fm", "random", "counter", "const"))
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=iq.shape[1]))
    got, frames = sv.process_batch(iq)
    assert frames == F and sv.kernel_name == _chain_name(nfft)
    assert np.array_equal(_bits(got), _bits(oracle_rows(oracle_mod, nfft, iq, frames=F)))
    sv.close()


@pytest.mark.parametrize("nfft,odd_stride", [(256, False), (1024, False), (1024, True)], ids=["chain-256", "chain-1024", "typed-1024"])
def test_more_streams_than_the_machine_holds(pkg, oracle_mod, nfft, odd_stride):
    """1030 workgroups (the machine holds 256 to 512 of them at a time), 12 distinct rows tiled: every distinct row against the oracle, every
    copy bitwise its twin, and a second launch into a second buffer gives the same bits."""
    import torch
    ns, F, distinct = 1030, 50, 12
    iq, rows = tiled_rows(pkg, nfft, F, ns, 8000 + nfft, distinct)
    view = _place(torch, iq, 0, iq.shape[1] + (1 if odd_stride else 0))
    power = [_power(torch, ns, nfft) for _ in range(2)]
    torch.cuda.synchronize()
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=iq.shape[1]))
    for pw in power:
        assert sv.process_batch_device(view, pw) == F
        assert sv.kernel_name == (_typed_name(nfft) if odd_stride else _chain_name(nfft))
    sv.synchronize()
    want = oracle_rows(oracle_mod, nfft, rows, frames=F)
    _check_power(power[0], nfft, np.tile(want, ((ns + distinct - 1) // distinct, 1))[:ns], (nfft, odd_stride))
    assert torch.equal(power[0], power[1])
    sv.close()


# ---- e. 2048 and 4096 points through every call form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [2048, 4096])
def test_long_frames_through_every_call_form(pkg, oracle_mod, nfft):
    import torch
    ns, F = 5, 2 * fpr(nfft) + 3
    iq = case_rows(pkg, nfft, F, ns, 9000 + nfft, classes=("fm", "random", "counter", "const"))
    nbytes = iq.shape[1]
    want = oracle_rows(oracle_mod, nfft, iq, frames=F)
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=nbytes))
    # device rows at even and odd addresses, iq = 2 mod 4, even and odd strides; padded power rows
    for offset, stride_extra in ((0, 0), (1, 0), (2, 0), (0, 3), (3, 6)):
        view = _place(torch, iq, offset, nbytes + stride_extra)
        power = _power(torch, ns, nfft, pad=9)
        torch.cuda.synchronize()
        assert sv.process_batch_device(view, power) == F
        assert sv.kernel_name == _typed_name(nfft)
        sv.synchronize()
        _check_power(power, nfft, want, (nfft, offset, stride_extra))
    # the caller's stream, then back to the handle's own
    view = _place(torch, iq, 0, nbytes)
    power = _power(torch, ns, nfft)
    torch.cuda.synchronize()
    mine = torch.cuda.Stream()
    sv.set_stream(mine.cuda_stream)
    assert sv.process_batch_device(view, power) == F
    mine.synchronize()
    sv.set_stream(None)
    _check_power(power, nfft, want, (nfft, "caller's stream"))
    power = _power(torch, ns, nfft)
    torch.cuda.synchronize()
    assert sv.process_batch_device(view, power) == F
    sv.synchronize()
    _check_power(power, nfft, want, (nfft, "own stream again"))
    # host buffers: rows iq_stride > nbytes apart, and power rows power_stride > nfft apart
    wide = np.full((ns, nbytes + 10), 255, np.uint8)
    wide[:, :nbytes] = iq
    out = np.zeros((ns, nfft), np.float32)
    rc, n = _call(pkg, sv, wide.ctypes.data, wide.strides[0], nbytes, out.ctypes.data, nfft, 0)
    assert rc == pkg.lib.OK and n == F and sv.kernel_name == _typed_name(nfft)
    assert np.array_equal(_bits(out), _bits(want))
    out = np.full((ns, nfft + 3), -1.0, np.float32)
    rc, n = _call(pkg, sv, wide.ctypes.data, wide.strides[0], nbytes, out.ctypes.data, nfft + 3, 0)
    assert rc == pkg.lib.OK and n == F
    assert np.array_equal(_bits(out[:, :nfft]), _bits(want)) and np.all(out[:, nfft:] == -1.0)
    sv.close()


# ---- f. one handle, alternating calls -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [128, 512, 1024])
def test_one_handle_alternating_kernels_and_a_zero_frame_call(pkg, oracle_mod, nfft):
    """chained kernel, typed-load kernel, a zero-frame call on device pointers with padded power rows (it zeroes exactly the nfft columns),
    chained kernel again: the handle keeps no state, so every call equals the oracle of its own bytes, and kernel_name follows each launch"""
    import torch
    ns = 3
    Fs = (2 * fpr(nfft) + 1, fpr(nfft) + fpw(nfft) + 1, 0, 25 * fpw(nfft) - 1)
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=2 * (max(Fs) * nfft + 7)))
    assert sv.kernel_name == _chain_name(nfft)
    for step, (F, offset) in enumerate(zip(Fs, (0, 1, 2, 2))):
        iq = case_rows(pkg, nfft, F, ns, 10000 + nfft + 10 * step) if F else case_rows(pkg, nfft, 1, ns, 10500)[:, :2 * nfft - 2]
        view = _place(torch, iq, offset, iq.shape[1] + 6)
        power = _power(torch, ns, nfft)
        torch.cuda.synchronize()
        assert sv.process_batch_device(view, power) == F
        sv.synchronize()
        if F:
            assert sv.kernel_name == (_typed_name(nfft) if offset & 1 else _chain_name(nfft)), step
            _check_power(power, nfft, oracle_rows(oracle_mod, nfft, iq, frames=F), (nfft, step))
        else:
            _check_power(power, nfft, np.zeros((ns, nfft), np.float32), (nfft, step))
    sv.close()


# ---- g. refusals, all before any launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [256, 2048])
def test_refusals_leave_the_handle_usable(pkg, oracle_mod, nfft):
    import torch
    ns, F = 2, 3
    iq = case_rows(pkg, nfft, F, ns, 11000 + nfft, extra=0)
    nbytes = iq.shape[1]
    want = oracle_rows(oracle_mod, nfft, iq, frames=F)
    d_iq = _place(torch, iq, 0, nbytes)
    sv = pkg.SpectrumView(pkg.SpectrumConfig(nfft=nfft, n_streams=ns, max_bytes_per_call=nbytes))
    dev = pkg.lib.F_DEVICE_PTRS

    def normal_call(where):
        power = _power(torch, ns, nfft)
        torch.cuda.synchronize()
        assert sv.process_batch_device(d_iq, power) == F
        sv.synchronize()
        _check_power(power, nfft, want, (nfft, where))

    normal_call("before")
    power = _power(torch, ns, nfft)
    torch.cuda.synchronize()
    refusals = (
        ("power_stride = nfft - 1", (d_iq.data_ptr(), nbytes, nbytes, power.data_ptr(), nfft - 1, dev), pkg.lib.ECAPACITY),
        ("SDRFM_F_OVERLAP", (d_iq.data_ptr(), nbytes, nbytes, power.data_ptr(), nfft + 5, dev | pkg.lib.F_OVERLAP), pkg.lib.EINVAL),
        ("an unknown flag", (d_iq.data_ptr(), nbytes, nbytes, power.data_ptr(), nfft + 5, 4), pkg.lib.EINVAL),
        # rows 4 GiB apart: the batch's span does not fit the 32-bit buffer descriptor; refused at the span check, before any launch
        ("iq_stride = 2**32", (d_iq.data_ptr(), 2 ** 32, 2 * nfft, power.data_ptr(), nfft + 5, dev), pkg.lib.ECAPACITY),
    )
    for where, args, status in refusals:
        rc, _ = _call(pkg, sv, *args)
        assert rc == status, (where, rc)
        sv.synchronize()
        assert torch.all(power == -1.0), where                   # nothing was launched
        normal_call("after " + where)
    sv.close()
