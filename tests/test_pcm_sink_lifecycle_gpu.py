"""The PCM sink's lifecycle on ONE demodulator handle: a sink reset in the middle of the handle's stream, a new sink in place of the old, two sinks used in turn,
stand-alone sink calls between calls with the chain inside the launch, a different call length on every call, a handle reset together with a sink reset.

What can break here: the per-run hand-off words of the chain (csrc/sdrfm_sink_chain.h, "Order between runs") belong to the handle and outlive any one sink; a
word an earlier session left must never pass for the predecessor's.  A run that took one would finish its first 64 outputs from a wrong carry: hundreds to
thousands of LSB, in whichever runs lost the race — so every stream of every call is checked, against the oracle (run_plan / check_plan in
tests/test_pcm_oracle_gpu.py, which also states the tolerances).  After each reset or replacement the capture continues with data from other generator ids:
replaying the same data would reproduce the same states and hide a stale one."""
import numpy as np
import pytest

from test_pcm_oracle_gpu import _names_ok, check_plan, run_plan

pytestmark = pytest.mark.gpu

N = 240000          # samples per call: 0.1 s at 2.4 MS/s


def _calls(k, ovl, sink="A", n=N, start=0):
    """k chain calls; every third one without an audio buffer (the PCM is all it leaves)."""
    return [("pcm", n, ovl, (start + j) % 3 != 2, sink) for j in range(k)]


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("n_before", range(1, 8))
def test_sink_reset_in_the_middle_of_a_stream(pkg, oracle_mod, n_before, overlap):
    """The stream's first call and n_before chain calls, then sdrfm_synchronize + sdrfm_pcm_sink_reset and eight more chain calls on the SAME handle: the
    demodulator goes on with its stream, the PCM starts again from state 0.  (Eight: the new session's calls 0 .. 7 meet every set of run words the old one
    left, whatever n_before.  Tagged by the sink's counter, the words were mistaken for the new session's in runs of its calls 1 .. n_before while n_before <= 6;
    at 7 the new calls 0 .. 3 overwrite every set first — the boundary case, kept.)"""
    ops = _calls(1 + n_before, overlap) + [("sink_reset", "A")] + _calls(8, overlap, start=1)
    res = run_plan(pkg, oracle_mod, ops, first_id=9000 + 100 * n_before)
    _names_ok(res, overlap=overlap)
    assert len(res.sessions) == 2 and len(res.sessions[1]["calls"]) == 8
    check_plan(res)


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("n_before", [1, 3, 6])
def test_a_new_sink_on_the_same_handle(pkg, oracle_mod, n_before, overlap):
    """The first sink destroyed after the stream's first call and n_before chain calls, a new one created and the stream continued into it."""
    ops = _calls(1 + n_before, overlap) + [("sink_new", "A")] + _calls(8, overlap, start=1)
    res = run_plan(pkg, oracle_mod, ops, first_id=9800 + 100 * n_before)
    _names_ok(res, overlap=overlap)
    check_plan(res)


def test_two_sinks_in_turn_on_one_handle(pkg, oracle_mod):
    """Overlapped calls into sink A and sink B in turn (12 calls): each sink's PCM is the host routine over the audio of ITS calls, its own state carried."""
    ops = [("pcm", N, True, k % 3 != 2, "AB"[k % 2]) for k in range(12)]
    res = run_plan(pkg, oracle_mod, ops, first_id=10500)
    _names_ok(res, overlap=True)
    assert [len(s["calls"]) for s in res.sessions] == [6, 6]
    check_plan(res)


def test_stand_alone_sink_calls_between_chain_calls(pkg, oracle_mod):
    """Chain calls, then (synchronised, as the header asks between the two styles) plain calls each followed by the sink's stand-alone kernel on its audio, then
    chain calls again — 14 sink calls, past the 8 slots of the per-stream word."""
    ops = _calls(4, True) + [("plain+sink", N, "A")] * 2 + _calls(4, True) + [("plain+sink", N, "A")] + _calls(3, True)
    res = run_plan(pkg, oracle_mod, ops, first_id=10600)
    _names_ok(res, overlap=True)
    assert len(res.sessions[0]["calls"]) == 14
    assert sum(c["standalone"] for c in res.calls) == 3
    check_plan(res)


@pytest.mark.parametrize("overlap", [False, True])
def test_a_different_length_on_every_call(pkg, oracle_mod, overlap):
    """Call lengths that change the runs per stream and the grid between calls that reuse a set of run words (48 000, 96 000, 20 000, 320 000, 48 000, 133 200
    samples ...), and the same after a sink reset."""
    lens = [48000, 96000, 20000, 320000, 48000, 133200, 96000, 20000, 48000]
    ops = [("pcm", n, overlap, True, "A") for n in lens] + [("sink_reset", "A")] + [("pcm", n, overlap, k % 2 == 0, "A") for k, n in enumerate(lens[::-1])]
    res = run_plan(pkg, oracle_mod, ops, first_id=10700)
    _names_ok(res)
    check_plan(res)


def test_handle_reset_together_with_sink_reset(pkg, oracle_mod):
    """sdrfm_reset and sdrfm_pcm_sink_reset: the next call starts a fresh stream — bit for bit what a fresh handle and a fresh sink make of the same capture, and
    against the oracle."""
    ops = _calls(5, True) + [("dm_reset",), ("sink_reset", "A")] + _calls(6, True)
    res = run_plan(pkg, oracle_mod, ops, first_id=10800)
    _names_ok(res, overlap=True)
    check_plan(res)
    fresh = run_plan(pkg, oracle_mod, _calls(6, True), first_id=10800 + 1000)     # (run_plan: the second handle stream's capture comes from first_id + 1000)
    _names_ok(fresh, overlap=True)
    check_plan(fresh)
    for k in range(6):
        a, b = res.calls[5 + k], fresh.calls[k]
        assert a["na"] == b["na"]
        assert a["pcm"].tobytes() == b["pcm"].tobytes(), k
        assert a["audio"].view(np.uint32).tobytes() == b["audio"].view(np.uint32).tobytes(), k


def test_sink_reset_on_host_buffers(pkg, oracle_mod):
    """The host-buffer form (no SDRFM_F_DEVICE_PTRS) at a shape design Q serves: three calls, a sink reset, four more."""
    ops = [("pcm", N, False, wa, "A") for wa in (True, False, True)] + [("sink_reset", "A")] + [("pcm", N, False, wa, "A") for wa in (True, True, False, True)]
    res = run_plan(pkg, oracle_mod, ops, ns=64, nu=16, host=True, first_id=10900)
    _names_ok(res, overlap=False)
    check_plan(res)
