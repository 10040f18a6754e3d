"""What the CPU and the GPU files of the broadcast handle's hist call (sdrfm_bcast_process_batch_metered_hist) share, built
without a device: the step geometry of the hist kernels (Python copies of bcast_hist_lds and of how sdrfm_bcast_create chooses their step,
on top of tests/pilot_shape_cases.py's copies of the plain layout), the exact integer bracket that ties a call's rows to its records, the
top-of-range inputs and the one scenario that is held to tests/scan_ref.py from bytes (tests/scan_hist_cases.py's: no constant rows, the
unmodulated carriers in the middle of a bin)."""
import numpy as np

import pilot_shape_cases as ps
import scan_hist_cases as hc

BINS, SHIFT, ZERO_BIN, HIST_LDS_BYTES = hc.BINS, hc.SHIFT, hc.ZERO_BIN, hc.HIST_LDS_BYTES
MAX_TAPS = 256                                                  # SDRFM_MAX_TAPS: the audio and RDS tap counts the header accepts are 1 .. 256
DEFAULT = (64, 10, 101, 32, 5, 255, 25)                         # (T, D, P, Ta, Da, Tr, Dr)
LDS_LIMITED = [ps.BCAST_D64, (256, 16, 255, 256, 1, 256, 1)]
# the issue's table, to be asserted: shape -> {tuned: (plain NDT, hist NDT)}; the default shape: {tuned: (plain LDS, hist LDS)}
STEPS = {ps.BCAST_D64: {False: (205, 197), True: (201, 193)}, (256, 16, 255, 256, 1, 256, 1): {False: (753, 725), True: (739, 709)}}
TABLE_DEFAULT = (64, 10, 101, 64, 5, 255, 25)                   # the default front end with the table's Ta 64, Tr 255
DEFAULT_LDS = {False: (55452, 57504), True: (55708, 57760)}


# ---- the step geometry ----------------------------------------------------------------------------------------------------------------
def plain_lds(shape, tuned, ny, ndt):
    T, D, P, Ta, Da, Tr, Dr = shape
    return (ps.bcast_lds_tuned if tuned else ps.bcast_lds)(T, D, P, Ta, Tr, ny, ndt)


def bins_offset(shape, tuned, ny, ndt):
    """where the bins start: the next multiple of 16 at or behind the end of the plain layout"""
    return (plain_lds(shape, tuned, ny, ndt) + 15) & ~15


def hist_lds(shape, tuned, ny, ndt):
    return bins_offset(shape, tuned, ny, ndt) + HIST_LDS_BYTES


def hist_step(shape, tuned, generic=True):
    """dict(NY, NDT, lds, fast, H) of the hist kernels' step: the fast kernel's fixed step where the plain form is fast and the bins fit
    beside it, else the largest even NY whose LDS with the bins fits the budget"""
    plain = ps.bcast_step(shape, tuned, generic)
    lds = lambda ny, ndt: hist_lds(shape, tuned, ny, ndt)
    return dict(ps._step(lds, plain["fast"]), H=plain["H"])


def hist_name(shape, tuned, generic, blend=False):
    kind = "fast" if hist_step(shape, tuned, generic)["fast"] else "generic"
    return "bcast-%s%s T%d D%d P%d Ta%d Da%d Tr%d Dr%d%s + hist" % ((kind, "-tuned" if tuned else "") + tuple(shape) + (" blend" if blend else "",))


# ---- the bracket ----------------------------------------------------------------------------------------------------------------------
def check_rows(meters, hist, where=""):
    """what holds of every call, for any input: uint32 [ns, 512]; a row's sum is its record's n; every dq of bin b lies in
    [(b - 256) 2^18, (b - 255) 2^18), so the row brackets the record's freq_q.  Python integers: no float, no wrap"""
    assert hist.dtype == np.uint32 and hist.shape == (meters.size, BINS), (where, hist.dtype, hist.shape)
    for s in range(meters.size):
        row = [int(v) for v in hist[s]]
        n, fq = int(meters["n"][s]), int(meters["freq_q"][s])
        assert sum(row) == n, (where, s, sum(row), n)
        lo = sum(c * (b - ZERO_BIN) << SHIFT for b, c in enumerate(row))
        if n:
            assert lo <= fq < lo + (n << SHIFT), (where, s, lo, fq, lo + (n << SHIFT))
        else:
            assert fq == 0, (where, s, fq)


# ---- the scenario against the reference from bytes -----------------------------------------------------------------------------------
REF_CASE = hc.TUNED_CASES[0]                                    # the default front end, 7 streams: station / carrier / random / unmodulated


def ref_case(pkg):
    """tests/scan_hist_cases.py's first tuned case: dict(ns, names, cycles, iq, h, b, ctaps, rot, refs)"""
    return hc.tuned_case(pkg, REF_CASE)


# ---- the top of the range: T = D = 1, P = 5, Ta = Tr = Da = Dr = 1, one stream of 4 MiB -------------------------------------------------
TOP_SHAPE, TOP_BYTES = ps.MAG_BCAST_SHAPE, hc.TOP_BYTES


def top_rows():
    """(constant bytes: d = 0 exactly, every count in bin 256; the byte pairs (255, 254), (1, 2) in turn: d = +-(pi - 3.1e-5), the two
    extreme bins), each [1, 4 MiB]"""
    iq = hc.top_case()
    return iq[0:1], iq[1:2]
