#!/usr/bin/env python3
"""The length of the hold in tests/stream_hold.py, measured: runs the two stream-order test files on streams that are NOT held
(stream_hold.UNHELD: hold() enqueues nothing, the assertions on pending events are skipped, the results are still compared) and keeps, per
script, the host time from hold() to the return of the last control call asserted on it.  The hold is twenty times the longest, rounded up
to a whole millisecond.  Writes the figures, and the delay unit timed with events, to profiles/stream_order_hold.txt (or the path given).

    python tools/stream_order_hold.py [out.txt]          measure
    python tools/stream_order_hold.py --short MS         the two files with a hold of MS milliseconds: what a stream that is not held gives
"""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stream_hold as sh  # noqa: E402

FILES = [os.path.join(ROOT, "tests", f) for f in ("test_stream_order_pcm_gpu.py", "test_stream_order_front_gpu.py")]
FILES = [f for f in FILES if os.path.exists(f)]


def main(argv):
    if argv[:1] == ["--short"]:
        sh.HOLD_MS = float(argv[1])
        return pytest.main(["-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + FILES + argv[2:])
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "stream_order_hold.txt")
    sh.UNHELD = True
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + FILES)
    sh.UNHELD = False
    if not sh.TIMES:
        print("no script ran (exit %d)" % rc)
        return 1
    per_ms, fill_ms = sh.delay_unit()
    what, t = max(sh.TIMES.items(), key=lambda kv: kv[1])
    hold = int(math.ceil(20.0 * t * 1e3))
    lines = ["stream-order tests: the hold of tests/stream_hold.py, measured on unheld streams (pytest exit %d, %d scripts)" % (rc, len(sh.TIMES)),
             "longest script, host time from the first enqueue to the return of the control call: %.3f ms (%s)" % (1e3 * t, what),
             "delay unit: %s" % ("%.0f cycles of torch.cuda._sleep per millisecond" % per_ms if per_ms else "%.3f ms per 256 MiB fill" % fill_ms),
             "hold: 20 x %.3f ms rounded up = %d ms (HOLD_MS)" % (1e3 * t, hold), "", "per script, milliseconds:"]
    lines += ["  %8.3f  %s" % (1e3 * v, k) for k, v in sorted(sh.TIMES.items(), key=lambda kv: -kv[1])]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]))
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
