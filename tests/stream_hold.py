"""Holding a caller's stream back, for the tests of the handles' stream-ordering contract (tests/test_stream_order_pcm_gpu.py,
tests/test_stream_order_front_gpu.py).  A plain module, imported the way pcm_mix_cases is.

hold(stream) enqueues a delay that ends by itself (torch.cuda._sleep, or a chain of large fills where that is missing) and returns a Hold whose
event lies behind the delay.  Nothing here gates a stream on an event the host records later, and no held stream waits on another: a control
call that waits for the stream always returns without help from the test.

Every test has two sides, and the two assertion helpers say which one failed:

  still_held(h, what)         the PRECONDITION: the delay was still pending when `what` was about to be made (or, for a call that must not wait,
                              when it returned).  A stream that was not held proves nothing, so this FAILS, as "inconclusive: stream not held".
  waited(h, ev, what)         the contract of a call that waits: the event recorded behind call A has completed when `what` returned.
  only_enqueued(h, what, ..)  the contract of a call that only enqueues: the delay is still pending when `what` returned.  Where it is not, the time
                              the call itself took tells a call that sat the delay out (the contract is broken) from a delay that was over too
                              soon (inconclusive again).

The length of the hold is measured, not guessed: tools/stream_order_hold.py runs both test files on streams that are NOT held (UNHELD = True:
hold() enqueues nothing and the helpers only keep the host time from hold() to the last assertion on it) and writes the longest such time to
profiles/stream_order_hold.txt.  HOLD_MS is twenty times that, rounded up to a whole millisecond; the factor is for a loaded host, and
still_held catches what it does not cover.

  measured on an MI355X host (profiles/stream_order_hold.txt): the longest script is the stereo sink's host-buffer call behind a pending device call,
  1.034 ms from the first enqueue to the return of the control call; the delay unit is 2 398 799 cycles of torch.cuda._sleep per millisecond;
  the hold is 20 x 1.034 ms rounded up = 21 ms, and the two files' 88 holds cost about two seconds.
"""
import time

HOLD_MS = 21                       # profiles/stream_order_hold.txt: 20 x the longest script's host time, rounded up to a whole millisecond
UNHELD = False                     # set by tools/stream_order_hold.py alone: measure the scripts' host time on streams that are not held
TIMES = {}                         # UNHELD: what -> the longest host time in seconds from hold() to the last assertion made on that hold

_unit = None                       # (cycles per millisecond of torch.cuda._sleep, or None where it is missing; ms per fill of the fallback)
_FILL_ELEMS = 1 << 26              # the fallback's launch: 256 MiB of int32 filled


def delay_unit():
    """(cycles of torch.cuda._sleep per millisecond, None) or (None, milliseconds per large fill): timed once per process with events"""
    global _unit
    if _unit is None:
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if hasattr(torch.cuda, "_sleep"):
            cycles = 20_000_000
            torch.cuda._sleep(1000)                                  # the kernel loaded
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            _unit = (cycles / max(a.elapsed_time(b), 1e-3), None)
        else:
            buf = torch.empty(_FILL_ELEMS, dtype=torch.int32, device="cuda")
            buf.fill_(0)
            torch.cuda.synchronize()
            a.record()
            for k in range(4):
                buf.fill_(k)
            b.record()
            b.synchronize()
            _unit = (None, max(a.elapsed_time(b) / 4, 1e-3))
    return _unit


class Hold:
    def __init__(self, event, t0, ms):
        self.event, self.t0, self.ms = event, t0, ms


def hold(stream, ms=None):
    """a self-terminating delay of ms (HOLD_MS) on a torch stream; the Hold's event is recorded behind it"""
    import torch
    ms = HOLD_MS if ms is None else ms
    per_ms, fill_ms = delay_unit()
    ev = torch.cuda.Event()
    if UNHELD:
        return Hold(ev, time.perf_counter(), 0.0)
    with torch.cuda.stream(stream):
        if per_ms is not None:
            torch.cuda._sleep(int(ms * per_ms))
        else:
            buf = torch.empty(_FILL_ELEMS, dtype=torch.int32, device="cuda")
            for k in range(int(ms / fill_ms) + 1):
                buf.fill_(k)
        ev.record(stream)
    return Hold(ev, time.perf_counter(), ms)


def record(stream):
    """an event behind whatever has been enqueued on the stream so far"""
    import torch
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def pending(event):
    return not event.query()


def _note(h, what):
    TIMES[what] = max(TIMES.get(what, 0.0), time.perf_counter() - h.t0)


def still_held(h, what):
    """the precondition: never passes on a stream that was not held"""
    if UNHELD:
        return _note(h, what)
    assert pending(h.event), ("inconclusive: stream not held — the delay of %g ms had already ended at '%s', %.3f ms of host time after it was "
                              "enqueued; the test proves nothing and is not passed" % (h.ms, what, 1e3 * (time.perf_counter() - h.t0)))


def only_enqueued(h, what, t_made=None, t_back=None):
    """the contract 'only enqueues / returns without synchronising': the delay in front of the call is still pending at its return.  t_made and
    t_back (time.perf_counter() around the call) tell a call that sat out the delay from a delay that was over too soon: the first took about
    as long as was left of the hold, the second did not — and is inconclusive, not a broken contract"""
    if UNHELD:
        return _note(h, what)
    if pending(h.event):
        return
    now = time.perf_counter()
    t_made, t_back = (now if t_made is None else t_made), (now if t_back is None else t_back)
    left = 1e-3 * h.ms - (t_made - h.t0)                            # of the hold when the call was made, by the host's clock
    assert left > 0 and t_back - t_made >= 0.5 * left, (
        "inconclusive: stream not held — the delay of %g ms was over when '%s' returned, %.3f ms of host time after it was enqueued, and the call "
        "itself took %.3f ms: it did not sit the delay out; the test proves nothing and is not passed" % (h.ms, what, 1e3 * (t_back - h.t0), 1e3 * (t_back - t_made)))
    raise AssertionError("contract: '%s' is documented to only enqueue, but it returned %.3f ms after it was made, with the %.3f ms that were left of the "
                         "stream's delay of %g ms over: the call waited for the stream" % (what, 1e3 * (t_back - t_made), 1e3 * left, h.ms))


def waited(h, event, what):
    """the contract 'waits for the stream': the event behind the pending call has completed at the call's return"""
    if UNHELD:
        return _note(h, what)
    assert not pending(event), "contract: '%s' is documented to wait for the handle's stream, but the call enqueued before it was still pending when it returned" % what
