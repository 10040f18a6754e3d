"""The kernels that run sdrfm_process_batch_pcm's calls after a stream's first — k_mfir_pcm and k_mix_pcm, the PCM = true instances of design Q — held to the
ORACLE: the audio they write (scaled error within TOL, and bit for bit what a plain handle given the same calls writes), the PCM (within 2 LSB of the host routine
sdrfm_pcm_deemph_s16 run over the oracle's audio) and the state the sink carries.  Every stream of every call is checked: a run that took a wrong carry spoils the
first 64 outputs of that run alone, and sampling streams could miss it.

The tests in tests/test_pcm_sink_gpu.py hold the PCM to the audio of the same launch; a PCM = true instance that computed wrong audio would pass them.  The
driver below (run_plan) is shared with tests/test_pcm_sink_lifecycle_gpu.py.

Tolerances:
  * audio: scaled_err <= TOL (the north-star tolerance; design Q's audio is measured within 1e-6 rad of the oracle);
  * PCM: <= 2 LSB.  The chain's blocked scan is within 1 LSB of the exact host routine over the SAME audio (tests/test_pcm_sink_gpu.py); design Q's audio error
    (<= 1e-6 rad measured) times gain (16 689) is 0.02 LSB, which may flip one more rounding.  A stale carry costs gain * |dy| for the run's first outputs:
    hundreds to thousands of LSB;
  * carried state: |d| <= 1e-6 * max(|st|, 0.25) + 1e-5 — the scan's relative bound plus the audio's error (de-emphasis is an average of the audio).
"""
import hashlib
import math

import numpy as np
import pytest

from conftest import TOL, scaled_err

PCM_LSB = 2
CANARY_PCM = 12345
CANARY_AUDIO = np.float32(1234.5)


def _params(pkg, tau=75e-6):
    lib = pkg.load_library()
    return float(lib.sdrfm_pcm_alpha(48000.0, tau)), float(np.float32(32767.0 / (2 * np.pi * 75e3 / 240e3)))


def state_tol(st):
    return 1e-6 * max(abs(float(st)), 0.25) + 1e-5


def pcm_bound(gain, audio_max):
    """The PCM tolerance at any gain, derived: 1 LSB for the scan against the exact chain, and the audio tolerance (TOL * max(1, |audio|) per output) through the
    de-emphasis — an average with weights that sum to 1, so the error of y is no larger — times |gain|, rounded up to whole steps.  At the default gain
    (16 689 x 1e-5 x pi = 0.52): 2, the PCM_LSB above."""
    return 1 + int(math.ceil(abs(float(gain)) * TOL * max(1.0, float(audio_max))))


# ---- reference helpers -------------------------------------------------------------------------------------------------------------------------------------
def oracle_calls(oracle_mod, h, g, rows, lens, D=10, Da=5):
    """The oracle's audio of each row of `rows` (one stream's whole capture per row: the calls' pieces, in order), run ONCE over the capture and split at each
    call's share of it: the outputs up to sample S of a stream that starts at phase 0 are floor(S / (D * Da)).  Returns one [n_rows, n_audio_k] array per call.
    The oracle's run over a capture is computed once and shared (read-only) by the tests that give it the same taps and bytes."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in (h, g, rows)) + repr((D, Da, rows.shape)).encode()).hexdigest()
    full = _ORACLE_MEMO.get(key)
    if full is None:
        full = np.stack([oracle_mod.Oracle(h, g, D, Da).process(r) for r in rows])
        full.setflags(write=False)
        if len(_ORACLE_MEMO) >= 4:
            _ORACLE_MEMO.pop(next(iter(_ORACLE_MEMO)))
        _ORACLE_MEMO[key] = full
    cum = np.concatenate([[0], np.cumsum(lens)]) // (D * Da)
    assert full.shape[1] == cum[-1], (full.shape, cum[-1])
    return [full[:, cum[k]:cum[k + 1]] for k in range(len(lens))]


_ORACLE_MEMO = {}


def host_pcm(pkg, auds, alpha, gain):
    """The host routine over a sink session's audio (one [n_rows, n_k] array per call, in the session's order), the state carried from call to call and started at
    0: (one int16 [n_rows, 2 n_k] array per call, the final state per row)."""
    nr = auds[0].shape[0]
    st = [0.0] * nr
    out = []
    for a in auds:
        p = np.zeros((nr, 2 * a.shape[1]), np.int16)
        for r in range(nr):
            p[r], st[r] = pkg.pcm_deemph_s16_host(a[r], alpha, gain, st[r])
        out.append(p)
    return out, np.array(st, np.float64)


def test_oracle_streams_piece_by_piece(pkg, oracle_mod):
    """oracle_calls runs the oracle over a stream's whole capture and splits it; the oracle is streaming, so piece-by-piece calls give the same audio, bit for
    bit — at the piece lengths the tests below use (whole numbers of 8 audio periods and lengths that are not)."""
    h, g = pkg.default_config(64)
    lens = [48000, 96000, 20000, 320000, 48000, 133200, 24200, 48400]
    rows = pkg.make_iq(3, sum(lens), mode="fm", first_id=7100)
    split = oracle_calls(oracle_mod, h, g, rows, lens)
    for r in range(rows.shape[0]):
        o = oracle_mod.Oracle(h, g)
        off = 0
        for k, n in enumerate(lens):
            piece = o.process(rows[r, 2 * off:2 * (off + n)])
            assert piece.view(np.uint32).tobytes() == split[k][r].view(np.uint32).tobytes(), (r, k)
            off += n


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------------
class PlanResult:
    def __init__(self):
        self.calls = []          # per call: dict(seg, n, na, ovl, audio, sink_sess, name, pcm, audio_t, twin_t, standalone)
        self.sessions = []       # per sink session: dict(calls=[call indices], state=None or np.ndarray, status)
        self.segments = []       # per handle stream: dict(rows, lens=[samples per call])

    @property
    def names(self):
        return [c["name"] for c in self.calls]


def run_plan(pkg, oracle_mod, ops, *, ns=256, nu=32, taps=64, fs=2.4e6, D=10, Da=5, first_id=8000, noisy_rows=(), bit_exact=False, host=False,
             astride=None, pstride=None, tau=75e-6, alpha=None, gain=None):
    """Runs `ops` on ONE demodulator handle (and, call for call, on a plain twin handle of the same configuration) and checks everything against the oracle.

    ops, in order:
      ("pcm", n, overlap, with_audio, sink)  sdrfm_process_batch_pcm on the next n samples of every stream, into sink `sink` ("A", "B", ...)
      ("plain+sink", n, sink)                after synchronising: a plain sdrfm_process_batch call, then the stand-alone sink kernel over its audio (then synchronised)
      ("sink_reset", sink)                   sdrfm_synchronize, sdrfm_pcm_sink_reset: the sink's PCM starts again from state 0
      ("sink_new", sink)                     sdrfm_synchronize, the sink destroyed and a new one created in its place
      ("dm_reset",)                          sdrfm_reset on both handles (and the sink's reset is up to the ops): the next call starts a new stream
      ("route", mask_of_rows)                dm.route() on both handles, the streams whose row is in the mask
    Stream s carries row s % nu of the capture; the capture of a handle stream is made of pieces from different generator ids, a new piece after every reset or
    replacement (replaying the same data would reproduce the same states and hide a stale one).  Every buffer is allocated before the first call.
    The sinks take alpha = sdrfm_pcm_alpha(48 kHz, tau) and the full-scale gain unless alpha or gain is given."""
    import torch
    alpha_d, gain_d = _params(pkg, tau)
    alpha = alpha_d if alpha is None else float(alpha)
    gain = gain_d if gain is None else float(gain)
    h, g = pkg.default_config(taps, fs=fs, fir_decim=D, audio_decim=Da) if (D, Da, fs) != (10, 5, 2.4e6) else pkg.default_config(taps)
    assert ns % nu == 0
    res = PlanResult()
    # ---- the plan: handle streams, their capture pieces, every call's place
    segs = [dict(pieces=[[]], lens=[])]
    for op in ops:
        if op[0] in ("pcm", "plain+sink"):
            segs[-1]["pieces"][-1].append(op[1])
            segs[-1]["lens"].append(op[1])
        elif op[0] in ("sink_reset", "sink_new"):
            if segs[-1]["pieces"][-1]:
                segs[-1]["pieces"].append([])
        elif op[0] == "dm_reset":
            segs.append(dict(pieces=[[]], lens=[]))
    fid = first_id
    for sg in segs:
        parts = []
        for pc in sg["pieces"]:
            if not pc:
                continue
            r = pkg.make_iq(nu, sum(pc), mode="fm", first_id=fid)
            for nr in noisy_rows:
                r[nr] = pkg.make_iq(1, sum(pc), mode="random", first_id=fid + 500 + nr)[0]
            parts.append(r)
            fid += 1000
        sg["rows"] = np.concatenate(parts, axis=1) if parts else np.zeros((nu, 0), np.uint8)
        res.segments.append(dict(rows=sg["rows"], lens=sg["lens"]))
    cfg = dict(fir_coeffs=h, audio_coeffs=g, n_streams=ns, fir_decim=D, audio_decim=Da, bit_exact=bit_exact,
               max_bytes_per_call=2 * max(max(sg["lens"]) for sg in segs if sg["lens"]))
    dev_iq = None
    if not host:
        dev_iq = [torch.from_numpy(sg["rows"]).cuda().repeat(ns // nu, 1) if sg["lens"] else None for sg in segs]
    # ---- buffers of every call, up front (a fill on torch's stream must not land on a call on the handle's)
    calls = []
    for si, sg in enumerate(segs):
        off = 0
        for n in sg["lens"]:
            na = n // (D * Da)
            a_s = na if astride is None else astride
            p_s = 2 * na if pstride is None else pstride
            assert a_s >= na and p_s >= 2 * na
            c = dict(seg=si, off=off, n=n, na_want=na)
            if not host:
                c["audio_t"] = torch.full((ns, a_s), float(CANARY_AUDIO), dtype=torch.float32, device="cuda")
                c["twin_t"] = torch.zeros((ns, a_s), dtype=torch.float32, device="cuda")
                c["pcm_t"] = torch.full((ns, p_s), CANARY_PCM, dtype=torch.int16, device="cuda")
                c["sa_t"] = torch.zeros((ns, a_s), dtype=torch.float32, device="cuda")
            calls.append(c)
            off += n
    if not host:
        torch.cuda.synchronize()
    # ---- the calls
    sinks, sess_of = {}, {}

    def new_session(name):
        sess_of[name] = len(res.sessions)
        res.sessions.append(dict(sink=name, calls=[], state=None, status=None))

    def close_session(name):
        s = res.sessions[sess_of[name]]
        s["status"] = sinks[name].synchronize_status()
        s["state"] = sinks[name].state() if s["calls"] and s["status"] == 0 else None   # (get_state answers the chain's error too)

    mk = lambda: pkg.FmDemod(pkg.FmConfig(**cfg))
    ci = 0
    seg = 0
    with mk() as dm, mk() as twin:
        try:
            for op in ops:
                kind = op[0]
                if kind in ("pcm", "plain+sink"):
                    c = calls[ci]
                    if c["seg"] != seg:
                        raise AssertionError("plan bookkeeping")
                    name = op[2] if kind == "plain+sink" else op[4]
                    if name not in sinks:
                        sinks[name] = pkg.PcmSink(ns, alpha, gain)
                        new_session(name)
                    sink = sinks[name]
                    if host:
                        chunk = np.ascontiguousarray(np.tile(res.segments[seg]["rows"][:, 2 * c["off"]:2 * (c["off"] + c["n"])], (ns // nu, 1)))
                        assert kind == "pcm"
                        if op[3]:
                            pcm, aud = dm.process_batch_pcm(sink, chunk, want_audio=True)
                            c["audio"] = aud
                        else:
                            pcm = dm.process_batch_pcm(sink, chunk)
                        c["name"] = dm.kernel_name
                        c["pcm"] = pcm
                        c["twin"] = twin.process_batch(chunk)
                        c["na"] = pcm.shape[1] // 2
                        c.update(ovl=False, with_audio=bool(op[3]), standalone=False)
                    else:
                        iq = dev_iq[seg][:, 2 * c["off"]:]
                        if kind == "pcm":
                            n, ovl, with_audio = op[1], op[2], op[3]
                            c["na"] = dm.process_batch_pcm_device(sink, iq, c["audio_t"] if with_audio else None, c["pcm_t"], nbytes=2 * n, overlap=ovl)
                            c["name"] = dm.kernel_name
                            c.update(ovl=ovl, with_audio=with_audio, standalone=False)
                        else:
                            n = op[1]
                            dm.synchronize()
                            sink.synchronize()
                            c["na"] = dm.process_batch_device(iq, c["audio_t"], nbytes=2 * n)
                            c["name"] = dm.kernel_name
                            dm.synchronize()
                            sink.process_batch_device(c["audio_t"], c["pcm_t"], c["na"])
                            sink.synchronize()
                            c.update(ovl=False, with_audio=True, standalone=True)
                        twin.process_batch_device(iq, c["twin_t"], nbytes=2 * op[1], overlap=c["ovl"])
                    res.sessions[sess_of[name]]["calls"].append(ci)
                    res.calls.append(c)
                    ci += 1
                elif kind in ("sink_reset", "sink_new"):
                    name = op[1]
                    dm.synchronize()
                    close_session(name)
                    if kind == "sink_reset":
                        sinks[name].reset()
                    else:
                        sinks[name].close()
                        sinks[name] = pkg.PcmSink(ns, alpha, gain)
                    new_session(name)
                elif kind == "dm_reset":
                    dm.synchronize()
                    twin.synchronize()
                    dm.reset()
                    twin.reset()
                    seg += 1
                elif kind == "route":
                    m = np.isin(np.arange(ns) % nu, np.asarray(op[1], dtype=np.int64)).astype(np.uint8)
                    dm.route(m)
                    twin.route(m)
                else:
                    raise AssertionError(op)
            dm.synchronize()
            twin.synchronize()
            for name in sinks:
                close_session(name)
            if not host:
                for c in res.calls:
                    c["pcm"] = c.pop("pcm_t").cpu().numpy()
                    c["audio"] = c.pop("audio_t").cpu().numpy()
                    c["twin"] = c.pop("twin_t").cpu().numpy()
        finally:
            for s in sinks.values():
                s.close()
    res.ns, res.nu, res.alpha, res.gain, res.h, res.g, res.D, res.Da = ns, nu, alpha, gain, h, g, D, Da
    res.oracle_mod, res.pkg = oracle_mod, pkg
    return res


def check_plan(res, derived_bound=False):
    """Every call's audio against the oracle and against the twin handle, every sink session's PCM (within PCM_LSB; derived_bound: within pcm_bound() of the sink's gain
    and the oracle's largest |audio|, which is PCM_LSB at the default gain) and carried state against the host routine over
    the oracle's audio, nothing written past a row's samples, no chain error.  Returns the worst PCM error in LSB (res.worst_state: the worst state difference)."""
    pkg, ns, nu = res.pkg, res.ns, res.nu
    res.worst_state = 0.0
    rows_of = np.arange(ns) % nu
    orc = [oracle_calls(res.oracle_mod, res.h, res.g, sg["rows"], sg["lens"], res.D, res.Da) if sg["lens"] else [] for sg in res.segments]
    per_seg_k = {}
    for i, c in enumerate(res.calls):
        k = per_seg_k.get(c["seg"], 0)
        per_seg_k[c["seg"]] = k + 1
        c["oracle"] = orc[c["seg"]][k]
        assert c["na"] == c["na_want"] == c["oracle"].shape[1], (i, c["na"], c["na_want"], c["oracle"].shape)
    for i, c in enumerate(res.calls):
        na = c["na"]
        if c["with_audio"]:
            got = c["audio"][:, :na]
            err = scaled_err(got, c["oracle"][rows_of])
            assert err <= TOL, "call %d (%s): audio %.3g off the oracle" % (i, c["name"], err)
            tw = c["twin"][:, :na]
            assert np.array_equal(got.view(np.uint32), tw.view(np.uint32)), \
                "call %d (%s): audio differs from the plain handle's (%d streams)" % (i, c["name"], int((got.view(np.uint32) != tw.view(np.uint32)).any(1).sum()))
            if c["audio"].shape[1] > na:
                assert (c["audio"][:, na:] == CANARY_AUDIO).all(), "call %d: audio written past the row's %d outputs" % (i, na)
        else:
            assert scaled_err(c["twin"][:, :na], c["oracle"][rows_of]) <= TOL, i
        assert c["pcm"].shape[1] >= 2 * na
        assert (c["pcm"][:, 2 * na:] == CANARY_PCM).all(), "call %d: PCM written past the row's %d samples" % (i, 2 * na)
    lsb = pcm_bound(res.gain, max(float(np.abs(c["oracle"]).max()) for c in res.calls)) if derived_bound else PCM_LSB
    res.lsb = lsb
    worst = 0
    for si, s in enumerate(res.sessions):
        assert s["status"] == 0, "sink session %d (%s): the sink reports a chain error" % (si, s["sink"])
        if not s["calls"]:
            continue
        want, st = host_pcm(pkg, [res.calls[i]["oracle"] for i in s["calls"]], res.alpha, res.gain)
        for j, i in enumerate(s["calls"]):
            c = res.calls[i]
            got = c["pcm"][:, :2 * c["na"]].astype(np.int32)
            assert got[:, 0::2].tobytes() == got[:, 1::2].tobytes(), "call %d: L != R" % i
            d = np.abs(got - want[j][rows_of].astype(np.int32))
            m = int(d.max()) if d.size else 0
            worst = max(worst, m)
            if m > lsb:
                bad = np.argwhere(d[:, 0::2] > lsb)
                streams = np.unique(bad[:, 0])
                raise AssertionError("sink session %d (%s), its call %d = call %d (%s): PCM %d LSB off the host routine over the oracle's audio; %d streams, "
                                     "first (stream, output) %s; outputs off %s" % (si, s["sink"], j, i, c["name"], m, streams.size, bad[:6].tolist(),
                                                                                  np.unique(bad[:, 1])[:16].tolist()))
        got_st = s["state"].astype(np.float64)
        for st_i in range(ns):
            w = st[rows_of[st_i]]
            assert abs(got_st[st_i] - w) <= state_tol(w), "sink session %d: stream %d carries %r, want %r" % (si, st_i, got_st[st_i], w)
            res.worst_state = max(res.worst_state, abs(got_st[st_i] - w))
    return worst


def _names_ok(res, *, overlap=None, chain=True):
    """The kernels the calls ran, asserted before any number: the first call of a stream is followed by the sink's own kernel, every later one holds the chain —
    or, with chain=False (a sink whose alpha the chain does not serve), no call holds it."""
    names = res.names
    if not chain:
        assert not any("+ pcm" in nm for nm in names), names
        return
    seg_first = [i == 0 or res.calls[i]["seg"] != res.calls[i - 1]["seg"] for i in range(len(res.calls))]
    for i, nm in enumerate(names):
        if seg_first[i]:
            assert "+ pcm" not in nm, (i, names)
        elif not res.calls[i]["standalone"]:
            assert "+ pcm" in nm, (i, names)
            if overlap is not None:
                assert ("overlapped" in nm) == (overlap and res.calls[i]["ovl"]), (i, names)


# ---- oracle parity of the "+ pcm" kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("with_audio", [True, False])
def test_pcm_kernels_against_the_oracle_at_configs2(pkg, oracle_mod, overlap, with_audio):
    """configs[2]'s shape: 256 streams x 0.1 s, 64 taps, nine calls (k_mfir_pcm<0 / 1, 5>), with and without an audio buffer, overlapped and not."""
    res = run_plan(pkg, oracle_mod, [("pcm", 240000, overlap, with_audio, "A")] * 9, first_id=8100)
    _names_ok(res, overlap=overlap)
    check_plan(res)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,decim,adecim,taps", [(2.048e6, 8, 8, 64), (3.2e6, 16, 5, 64), (2.4e6, 10, 5, 16)])
def test_pcm_kernels_against_the_oracle_at_the_other_front_end_rates(pkg, oracle_mod, fs, decim, adecim, taps):
    """The other instances with the chain: 2.048 MS/s / 8 / 8, 3.2 MS/s / 16 / 5, and 16 channel taps (test_pcm_chain_at_the_other_front_end_rates' parameters)."""
    nsamp = decim * adecim * 8 * 120
    res = run_plan(pkg, oracle_mod, [("pcm", nsamp, True, True, "A")] * 4, taps=taps, fs=fs, D=decim, Da=adecim, first_id=8200)
    _names_ok(res, overlap=True)
    check_plan(res)


@pytest.mark.gpu
def test_pcm_kernels_against_the_oracle_in_runs_that_flush_twice(pkg, oracle_mod):
    """0.133 s and longer per call (runs of more than the four audio stages design Q parks: the run is sunk in two goes)."""
    res = run_plan(pkg, oracle_mod, [("pcm", n, True, wa, "A") for n, wa in ((320000, True), (320000, True), (319600, False), (480000, True))],
                   first_id=8300)
    _names_ok(res, overlap=True)
    check_plan(res)


@pytest.mark.gpu
@pytest.mark.parametrize("nsamp,astride,pstride", [(48000, 961, 2 * 961), (48400, 1008, 2100), (288000, 5760, 11520)])
def test_pcm_kernels_against_the_oracle_at_odd_lengths_and_unaligned_rows(pkg, oracle_mod, nsamp, astride, pstride):
    """Rows that are not 16-byte aligned and odd lengths (test_pcm_chain_rows_that_are_not_16_byte_aligned_and_odd_lengths' shapes); nothing written past a
    row's 2 n_audio PCM samples or n_audio outputs."""
    res = run_plan(pkg, oracle_mod, [("pcm", nsamp, True, True, "A")] * 3, ns=64, nu=16, astride=astride, pstride=pstride, first_id=8400)
    _names_ok(res, overlap=True)
    check_plan(res)


@pytest.mark.gpu
@pytest.mark.parametrize("taps", [16, 64])
def test_pcm_kernels_against_the_oracle_for_one_dongle(pkg, oracle_mod, taps):
    """configs[1]'s shape: one stream, a second per call — hundreds of runs of one stream, each finishing its first outputs with its neighbour's state."""
    res = run_plan(pkg, oracle_mod, [("pcm", 2400000, True, True, "A")] * 3, ns=1, nu=1, taps=taps, first_id=8500)
    _names_ok(res, overlap=True)
    check_plan(res)


@pytest.mark.gpu
@pytest.mark.parametrize("with_audio", [True, False])
def test_pcm_kernels_against_the_oracle_in_mixed_launches(pkg, oracle_mod, with_audio):
    """k_mix_pcm: every 16th stream carries noise and is routed to design B inside design Q's launch (its PCM by the sink's list kernel behind it); routed and
    clean streams both against the oracle."""
    ops = [("pcm", 240000, True, with_audio, "A")] * 2 + [("route", (5, 21))] + [("pcm", 240000, True, with_audio, "A")] * 4
    res = run_plan(pkg, oracle_mod, ops, noisy_rows=(5, 21), first_id=8600)
    _names_ok(res, overlap=True)
    assert all("in one launch" in nm for nm in res.names[2:]), res.names
    check_plan(res)


@pytest.mark.gpu
def test_pcm_call_of_a_bit_exact_handle_against_the_oracle(pkg, oracle_mod):
    """A bit-exact handle: every call is followed by the sink's own kernel (no "+ pcm"); its audio and PCM against the oracle too."""
    res = run_plan(pkg, oracle_mod, [("pcm", 240000, True, wa, "A") for wa in (True, True, False, True, False, True)], ns=128, bit_exact=True,
                   first_id=8700)
    assert not any("+ pcm" in nm or nm.startswith("fast-q") for nm in res.names), res.names
    check_plan(res)


@pytest.mark.gpu
def test_pcm_call_on_host_buffers_against_the_oracle(pkg, oracle_mod):
    """Without SDRFM_F_DEVICE_PTRS, at a shape design Q serves (64 streams x 0.1 s): the chain inside the launch, the audio and the PCM against the oracle."""
    res = run_plan(pkg, oracle_mod, [("pcm", 240000, False, wa, "A") for wa in (True, True, False, True)], ns=64, nu=16, host=True, first_id=8800)
    _names_ok(res, overlap=False)
    check_plan(res)
