"""The cases of tests/test_fm_exact_shapes_gpu.py as a table: the FM handle's bit-exact kernels — the generic kernel at every tile size fm_generic_tile
gives, every design-B instance the product selects across the classes fm_b_tiles cuts a stream into — with the call sequences and, per call, the class
it is meant to reach.  tests/test_fm_exact_cases_cpu.py runs every case through csrc/sdrfm_fm_call.h on the CPU (tests/native/fm_exact_cases.cpp, the
FmGeom of a bit-exact handle on a 256-CU device) and the GPU test asserts kernel_name against the same entries, so the two cannot drift apart.

All counts are samples per stream (2 bytes each)."""
from collections import namedtuple

import numpy as np

# ================================================================================================================================================
#  A. the generic kernel: shapes (T, D, Ta, Da) by the audio outputs per tile fm_generic_tile gives them (NA halves from 64 until the block fits 48 KiB)
# ================================================================================================================================================
GENERIC_SHAPES = (
    (64, (1, 1, 1, 1)), (64, (7, 3, 5, 4)), (64, (256, 1, 256, 1)), (64, (256, 64, 1, 1)), (64, (17, 5, 255, 2)),
    (32, (128, 16, 64, 6)), (32, (33, 64, 3, 2)),
    (16, (31, 7, 129, 33)),
    (8, (100, 20, 64, 16)), (8, (256, 64, 64, 3)),
    (4, (64, 10, 256, 64)), (4, (129, 31, 17, 33)),
    (2, (2, 64, 2, 64)), (2, (64, 64, 64, 16)),
    (1, (256, 64, 256, 64)), (1, (1, 64, 256, 64)), (1, (255, 63, 65, 31)),
)
STREAM_CLASSES = ("fm", "random", "counter", "const")           # stream s holds class s % 4: no lone const stream at 1, 3 or 7 streams
UNALIGNED_SHAPES = ((7, 3, 5, 4), (64, 10, 256, 64), (256, 64, 256, 64))   # the device-pointer form on unaligned rows: NA 64, 4 and 1, all multi-stream
UNALIGNED_LAYOUT = (3, 5)                                       # odd offset, odd stride: alignment class 1


def shape_id(shape):
    return "T%d-D%d-Ta%d-Da%d" % tuple(shape)


def generic_streams(shape):
    return (1, 3, 7)[[s for _, s in GENERIC_SHAPES].index(tuple(shape)) % 3]


def generic_na(shape):
    return next(na for na, s in GENERIC_SHAPES if s == tuple(shape))


def counts(phase_x, phase_d, n, D, Da):
    """(M, A, phase_x after, phase_d after) of a call of n samples: two decimators that count their inputs"""
    M = (phase_x + n) // D
    return M, (phase_d + M) // Da, (phase_x + n) % D, (phase_d + M) % Da


def _tiles_ok(A, M, NA, Ta, Da):
    """at least three generic tiles, the last one partial (it cannot be where a tile holds one output), and Ta + 2 Da decimated outputs"""
    return A >= 3 * NA + 1 and (A % NA != 0 or NA == 1) and M >= Ta + 2 * Da


# one call of a ragged sequence: samples, and what it is there for
Ragged = namedtuple("Ragged", "nsamp why")


def generic_calls(shape):
    """The ragged call list of a generic shape.  Small calls first — the classes a hand-over can get wrong, where the shape has them —, then the
    smallest long call that gives three tiles with a partial last one from the phases it starts at, then a tail that reads the long call's state
    and leaves the total odd, with the same three-tiles property for the whole stream in one call."""
    T, D, Ta, Da = shape
    NA = generic_na(shape)
    calls = [Ragged(0, "0-byte"), Ragged(1, "2-byte")]
    if D >= 2:
        calls.append(Ragged(1, "M=0,N>0"))                      # (the 2-byte call before it is one already)
    if T >= 3:
        calls.append(Ragged(T - 2, "N<T-1"))
    if Ta >= 3:
        calls.append(Ragged(max(1, (Ta - 1) // 2) * D, "0<M<Ta-1"))   # M = that many at any phase: the new d history mixes old and new
    px = sum(c.nsamp for c in calls) % D
    if D >= 2:
        calls.append(Ragged(next(n for n in range(1, 2 * D + 1) if (px + n) % D % 2 == 1), "phase_x-odd"))
    calls += [Ragged(D, "phase_d"), Ragged(D, "phase_d")]         # one decimated output each: phase_d moves on
    px = pd = 0
    for c in calls:
        _, _, px, pd = counts(px, pd, c.nsamp, D, Da)
    n = 1
    while True:
        M, A, _, _ = counts(px, pd, n, D, Da)
        if _tiles_ok(A, M, NA, Ta, Da):
            break
        n += 1
    calls.append(Ragged(n, "long"))
    tail = D * Da + 1
    while True:
        total = sum(c.nsamp for c in calls) + tail
        M, A, _, _ = counts(0, 0, total, D, Da)
        if total % 2 == 1 and _tiles_ok(A, M, NA, Ta, Da):
            break
        tail += 1
    calls.append(Ragged(tail, "tail"))
    return tuple(calls)


def generic_total(shape):
    return sum(c.nsamp for c in generic_calls(shape))


def generic_taps(shape):
    """Random and asymmetric: a reversed or shifted tap index changes the result.  h = N(0,1) / sqrt(T); g = N(0,1) over its absolute sum (sum|g| = 1 is
    what TOL is stated for)."""
    T, D, Ta, Da = shape
    rng = np.random.default_rng(1000 * T + 100 * D + 10 * Ta + Da)
    h = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    g = rng.standard_normal(Ta)
    return h, (g / np.abs(g).sum()).astype(np.float32)


def streams(pkg, ns, nsamp, first_id):
    """[ns, 2 nsamp] bytes: classes fm, random, counter and const in turn"""
    return np.concatenate([pkg.make_iq(1, nsamp, mode=STREAM_CLASSES[s % 4], first_id=first_id + s) for s in range(ns)])


def generic_rows(pkg, shape):
    """the streams tests/test_fm_exact_shapes_gpu.py feeds a generic shape"""
    return streams(pkg, generic_streams(shape), generic_total(shape), 21000 + shape[0] + shape[1])


# ================================================================================================================================================
#  B. design B: every instance the product selects (T, D, Da, R) at 32 audio taps, across the classes fm_b_tiles cuts a stream into
# ================================================================================================================================================
B_TA = 32
B_INSTANCES = ((64, 10, 5, 12), (32, 10, 5, 12), (16, 10, 5, 12), (64, 8, 8, 12), (16, 8, 8, 12), (64, 4, 8, 12), (64, 16, 5, 8))
# one call: samples, alignment class of the rows (device-pointer calls; host-buffer calls go through the staging rows, class 16), why it is there
BCall = namedtuple("BCall", "nsamp cls why")
# one handle: the instance, streams, host buffers or device pointers, the calls
BCase = namedtuple("BCase", "name T D Da R ns device calls")
# what a call must reach: kind 'b' / 'g', audio outputs per segment (generic: per tile), segments (tiles) per stream, fold_state, fm_short_first,
# the fix-up's tiles per stream (0: no fix-up), where the min_subtiles back-off ends (0: not design B)
Reach = namedtuple("Reach", "kind NA tiles fold short_first fixup min_subtiles")


def b_id(inst):
    return "T%d-D%d-Da%d" % tuple(inst[:3])


def b_taps(inst):
    T, D, Da, R = inst
    rng = np.random.default_rng(7000 + 100 * T + 10 * D + Da)
    h = (rng.standard_normal(T) / np.sqrt(T)).astype(np.float32)
    g = rng.standard_normal(B_TA)
    return h, (g / np.abs(g).sum()).astype(np.float32)


def y_aff(T, D):
    return (T + D - 1) // D + 1


def b_cases(inst):
    """The sizes are the D = 10, Da = 5 ones scaled per rate: in sub-tiles of NYT = 64 R decimated outputs.  None is a whole number of design S's lane
    segments (480 samples) at (64, 10) and (32, 10), and no handle has the streams design S asks for."""
    T, D, Da, R = inst
    NYT = 64 * R
    first = (y_aff(T, D) + B_TA) * D                            # the shortest first call design B serves: M = y_aff + Ta
    odd = 9 if Da == 8 else 1                                    # decimated outputs past whole sub-tiles that leave A no multiple of NA at this rate
    one, many = 62 * D, (10 * NYT + odd) * D                     # 620 and 76 810 samples at / 10
    seq = (BCall(first, 16, "first-b"), BCall(one, 16, "one-subtile"), BCall(many, 16, "many-short-last"), BCall(20 * D, 16, "no-fold"),
           BCall(one + 2, 16, "b"), BCall(one, 16, "even-phase"), BCall(one + 1, 16, "even-phase"), BCall(one, 16, "odd-phase"),
           BCall(one + D - 3, 16, "odd-phase"), BCall(one, 16, "back-on-b")) + tuple(BCall(61 * D, 16, "phase_d") for _ in range(Da))
    n3, n7 = (4 * NYT + 1) * D, (2 * NYT + odd) * D               # 30 730 and 15 370 samples at / 10; the second calls a little longer, so that theirs
    m3, m7 = n3 + 2 * Da * D, n7 + Da * D                         # is no whole number of segments either from the phase_d the first leaves
    tag = b_id(inst)
    out = [
        BCase("b-%s-one-stream" % tag, T, D, Da, R, 1, False, seq),
        # a first call one decimated output short of what design B needs: the generic kernel alone, then design B on the state it left — behind an odd
        # phase (a generic call between) and directly
        BCase("b-%s-short-first-odd" % tag, T, D, Da, R, 1, False, (BCall(first - 1, 16, "first-g"), BCall(one + 1, 16, "odd-phase"), BCall(one, 16, "back-on-b"))),
        BCase("b-%s-short-first-even" % tag, T, D, Da, R, 1, False, (BCall(first - 2, 16, "first-g"), BCall(one + 2, 16, "even-phase"), BCall(one, 16, "b"))),
        BCase("b-%s-3-streams" % tag, T, D, Da, R, 3, True, (BCall(n3, 16, "segments"), BCall(m3, 4, "segments"))),
        BCase("b-%s-7-streams" % tag, T, D, Da, R, 7, True, (BCall(n7, 4, "segments"), BCall(m7, 16, "segments"))),
    ]
    if inst == (64, 10, 5, 12):
        # the min_subtiles back-off (this instance only, because of memory).  520 x 15 400 has three sub-tiles a stream: the back-off ends at 1, not at 2
        # (520 x (3 / 2) = 520 segments are fewer than half of the 2048 wave slots); 23 100 samples have four, where it ends at 2
        out.append(BCase("b-%s-520-streams" % tag, T, D, Da, R, 520, True, (BCall(15400, 16, "back-off-1"), BCall(15400, 4, "back-off-1"), BCall(23100, 16, "back-off-2"))))
        out.append(BCase("b-%s-342-streams" % tag, T, D, Da, R, 342, True, (BCall(92200, 16, "back-off-4"), BCall(92200, 4, "back-off-4"))))
    return out


def all_b_cases():
    return [c for inst in B_INSTANCES for c in b_cases(inst)]


def b_case(name):
    return next(c for c in all_b_cases() if c.name == name)


DEV_R8_CASES = (                                                # development library, SDRFM_FAST_R=8 at (64, 10, 32, 5): instance b(64, 10, 8), which the product never selects
    BCase("b-dev-R8-one-stream", 64, 10, 5, 8, 1, False, (BCall(76810, 16, "many-short-last"), BCall(76810, 16, "many-short-last"))),
    BCase("b-dev-R8-7-streams", 64, 10, 5, 8, 7, False, (BCall(15370, 16, "segments"), BCall(15370, 16, "segments"))),
)

# ================================================================================================================================================
#  C. value edges through the kernels
# ================================================================================================================================================
VALUE_GENERIC = ((7, 3, 5, 4), (100, 20, 64, 16))               # generic shapes (NA 64 and 8), / 3 and / 20: y[0] holds no sample from before the stream
VALUE_B = ((64, 10, 5, 12), (16, 8, 8, 12))                     # design-B instances
ZERO_SHAPES = VALUE_GENERIC + tuple((T, D, B_TA, Da) for T, D, Da, _ in VALUE_B)


def value_nsamp(T, D, Da, R=0):
    """samples of a value-edge stream: 3 T of const at either end and as much noise between, 40 audio outputs at least; under design B more than two sub-tiles"""
    return max(9 * T, 40 * D * Da, (2 * 64 * R + 100) * D) + 1


def zero_sum_taps(T, Ta):
    """h = (0.5, -0.5, 0, ...): sums to exactly 0, and 0.5 x - 0.5 x is exactly +0 in the fmaf chain; g random with unit absolute sum"""
    h = np.zeros(T, np.float32)
    h[0], h[1] = 0.5, -0.5
    g = np.random.default_rng(40 + Ta).standard_normal(Ta)
    return h, (g / np.abs(g).sum()).astype(np.float32)


def zero_rows(T, D, Da, R=0):
    """[2, 2 n] bytes.  Row 0: a constant (I, Q): every y is exactly 0 under zero-sum taps, every d takes the re = im = 0 rule.  Row 1: the constant for
    3 T samples, noise, the constant again: into y = 0 and out of it, so that a d is taken with a zero y[m - 1]."""
    n = value_nsamp(T, D, Da, R)
    rows = np.empty((2, n, 2), np.uint8)
    rows[:, :, 0], rows[:, :, 1] = 200, 77
    lo, hi = 3 * T, n - 3 * T
    rows[1, lo:hi] = np.random.default_rng(n).integers(0, 256, (hi - lo, 2), dtype=np.uint8)
    return rows.reshape(2, 2 * n)


def fullscale_rows(T, D, Da, R=0):
    """[2, 2 n] bytes of 0x00 and 0xFF only: a square wave of period 7 samples on I and of period 11 on Q, the second row shifted"""
    n = value_nsamp(T, D, Da, R)
    k = np.arange(n)
    rows = np.empty((2, n, 2), np.uint8)
    for r, shift in enumerate((0, 3)):
        rows[r, :, 0] = np.where((k + shift) % 7 < 4, 255, 0)
        rows[r, :, 1] = np.where((k + 2 * shift) % 11 < 5, 255, 0)
    return rows.reshape(2, 2 * n)


# ---- what every call reaches (fm_bx on the 256-CU geometry; tests/test_fm_exact_cases_cpu.py re-derives every row) ---------------------------------
# ---- what every call reaches: fm_bx on the 256-CU geometry, written down here and re-derived row by row in tests/test_fm_exact_cases_cpu.py ---------------
R = Reach
REACH = {
    "b-T64-D10-Da5-one-stream": (
        R("b", 8, 1, 1, 0, 1, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 140, 11, 1, 0, 0, 1), R("b", 4, 1, 0, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 13, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T64-D10-Da5-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T64-D10-Da5-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T64-D10-Da5-3-streams": (
        R("b", 123, 5, 1, 0, 1, 1), R("b", 124, 5, 1, 0, 0, 1),
    ),
    "b-T64-D10-Da5-7-streams": (
        R("b", 103, 3, 1, 0, 1, 1), R("b", 103, 3, 1, 0, 0, 1),
    ),
    "b-T64-D10-Da5-520-streams": (
        R("b", 103, 3, 1, 0, 1, 1), R("b", 103, 3, 1, 0, 0, 1), R("b", 231, 2, 1, 0, 0, 2),
    ),
    "b-T64-D10-Da5-342-streams": (
        R("b", 615, 3, 1, 0, 1, 4), R("b", 615, 3, 1, 0, 0, 4),
    ),
    "b-T32-D10-Da5-one-stream": (
        R("b", 7, 1, 1, 0, 1, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 140, 11, 1, 0, 0, 1), R("b", 4, 1, 0, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 12, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T32-D10-Da5-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 13, 1, 1, 0, 0, 1),
    ),
    "b-T32-D10-Da5-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1),
    ),
    "b-T32-D10-Da5-3-streams": (
        R("b", 123, 5, 1, 0, 1, 1), R("b", 124, 5, 1, 0, 0, 1),
    ),
    "b-T32-D10-Da5-7-streams": (
        R("b", 103, 3, 1, 0, 1, 1), R("b", 103, 3, 1, 0, 0, 1),
    ),
    "b-T16-D10-Da5-one-stream": (
        R("b", 7, 1, 1, 0, 1, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 140, 11, 1, 0, 0, 1), R("b", 4, 1, 0, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 13, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T16-D10-Da5-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T16-D10-Da5-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T16-D10-Da5-3-streams": (
        R("b", 123, 5, 1, 0, 1, 1), R("b", 124, 5, 1, 0, 0, 1),
    ),
    "b-T16-D10-Da5-7-streams": (
        R("b", 103, 3, 1, 0, 1, 1), R("b", 103, 3, 1, 0, 0, 1),
    ),
    "b-T64-D8-Da8-one-stream": (
        R("b", 5, 1, 1, 0, 1, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 88, 11, 1, 0, 0, 1), R("b", 2, 1, 0, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D8-Da8-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D8-Da8-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D8-Da8-3-streams": (
        R("b", 77, 5, 1, 0, 1, 1), R("b", 78, 5, 1, 0, 0, 1),
    ),
    "b-T64-D8-Da8-7-streams": (
        R("b", 65, 3, 1, 0, 1, 1), R("b", 65, 3, 1, 0, 0, 1),
    ),
    "b-T16-D8-Da8-one-stream": (
        R("b", 4, 1, 1, 0, 1, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 88, 11, 1, 0, 0, 1), R("b", 2, 1, 0, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 8, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T16-D8-Da8-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 7, 1, 1, 0, 0, 1),
    ),
    "b-T16-D8-Da8-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1),
    ),
    "b-T16-D8-Da8-3-streams": (
        R("b", 77, 5, 1, 0, 1, 1), R("b", 78, 5, 1, 0, 0, 1),
    ),
    "b-T16-D8-Da8-7-streams": (
        R("b", 65, 3, 1, 0, 1, 1), R("b", 65, 3, 1, 0, 0, 1),
    ),
    "b-T64-D4-Da8-one-stream": (
        R("b", 6, 1, 1, 0, 1, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 88, 11, 1, 0, 0, 1), R("b", 2, 1, 0, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("g", 64, 1, 0, 0, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
        R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D4-Da8-short-first-odd": (
        R("g", 64, 1, 0, 1, 0, 0), R("g", 64, 1, 0, 0, 0, 0), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D4-Da8-short-first-even": (
        R("g", 64, 1, 0, 1, 0, 0), R("b", 7, 1, 1, 0, 0, 1), R("b", 8, 1, 1, 0, 0, 1),
    ),
    "b-T64-D4-Da8-3-streams": (
        R("b", 77, 5, 1, 0, 1, 1), R("b", 78, 5, 1, 0, 0, 1),
    ),
    "b-T64-D4-Da8-7-streams": (
        R("b", 65, 3, 1, 0, 1, 1), R("b", 65, 3, 1, 0, 0, 1),
    ),
    "b-T64-D16-Da5-one-stream": (
        R("b", 7, 1, 1, 0, 1, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 94, 11, 1, 0, 0, 1), R("b", 4, 1, 0, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("g", 32, 1, 0, 0, 0, 0), R("g", 32, 1, 0, 0, 0, 0), R("b", 12, 1, 1, 0, 0, 1),
        R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1), R("b", 12, 1, 1, 0, 0, 1),
    ),
    "b-T64-D16-Da5-short-first-odd": (
        R("g", 32, 1, 0, 1, 0, 0), R("g", 32, 1, 0, 0, 0, 0), R("b", 13, 1, 1, 0, 0, 1),
    ),
    "b-T64-D16-Da5-short-first-even": (
        R("g", 32, 1, 0, 1, 0, 0), R("b", 12, 1, 1, 0, 0, 1), R("b", 13, 1, 1, 0, 0, 1),
    ),
    "b-T64-D16-Da5-3-streams": (
        R("b", 82, 5, 1, 0, 1, 1), R("b", 83, 5, 1, 0, 0, 1),
    ),
    "b-T64-D16-Da5-7-streams": (
        R("b", 69, 3, 1, 0, 1, 1), R("b", 69, 3, 1, 0, 0, 1),
    ),
}
