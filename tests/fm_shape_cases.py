"""The cases of tests/test_fm_shapes_gpu.py as a table: which design the FM handle is expected to reach for every call, by geometry, stream count, call
sizes, alignment class of the rows and previous call.  tests/test_fm_shapes_cpu.py runs every case through csrc/sdrfm_fm_call.h on the CPU
(tests/native/fm_shape_cases.cpp) and the GPU test asserts kernel_name against the same entries, so the two cannot drift apart.

Shapes: the smallest the eligibility rules admit on 256 CUs.  Design Q needs n_streams * ceil(M / 128) >= 512 and calls of whole multiples of 8 D Da
samples: 264 streams x two steps (1600 samples at / 10 / 5).  Design S (64 or 32 channel taps, / 10 / 5 only) needs n_streams * waves >= 1024 and whole
lane segments of 480 samples: 1024 streams x 2400 samples, which design Q takes too (2400 = 6 x 400).  One stream: 656 000 samples (513 steps)."""
from collections import namedtuple

# (byte offset of the first row, bytes added to the row stride) by alignment class of (iq, iq_stride): multiples of 16, of 4 only, anything else
LAYOUTS = {
    16: ((0, 0), (16, 32)),
    4: ((4, 0), (0, 4), (12, 20)),
    1: ((2, 0), (0, 2), (6, 6), (1, 0), (0, 1), (3, 5)),
}
REPRESENTATIVE = {16: (16, 32), 4: (12, 20), 1: (3, 5)}        # one layout per class, for the tests that switch between classes


def align_class(ptr, stride):
    return 16 if ptr % 16 == 0 and stride % 16 == 0 else 4 if ptr % 4 == 0 and stride % 4 == 0 else 1


# one call: samples per stream, alignment class of its rows, SDRFM_F_OVERLAP, device pointers (False: host buffers), the kernel name's first word,
# whether the name says "overlapped", and for a call with routed streams "one" / "two" launches (None: no routed streams)
Call = namedtuple("Call", "nsamp cls overlap device expect overlapped mixed", defaults=(False, True, None, False, None))
# one handle and its calls in order (n_routed: streams sent to the bit-exact kernels by the test hook right before call route_at)
Case = namedtuple("Case", "name T D Da ns bit_exact calls n_routed route_at", defaults=(0, 1))

GEOMS = ((64, 10, 5), (16, 10, 5), (64, 8, 8))                 # design Q's linear ring (64 and 16 taps at / 10) and its swizzled ring (/ 8)


def _has_s(T, D, Da):
    return (T, D, Da) == (64, 10, 5)


def align_shape(T, D, Da):
    """(streams, the three call sizes) of test 1 at a geometry: 1024 streams where design S exists (it needs them), else 264"""
    unit = 8 * D * Da
    if _has_s(T, D, Da):
        return 1024, (2400, 4800, 2400)
    k = 128 // (8 * Da) + 1                                     # the fewest units with more than one step of 128 decimated outputs
    return 264, (k * unit, 2 * k * unit, k * unit)


def expect_word(cls, bit_exact, has_s=True):
    if cls == 16:
        return ("fast-s" if has_s else "fast-b") if bit_exact else "fast-q"
    return "fast-b" if cls == 4 else "generic"


def _t(T, D, Da):
    return "T%d-D%d-Da%d" % (T, D, Da)


# ---- 1. row alignment selects the kernel -----------------------------------------------------------------------------------------------------
def align_cases():
    out = []
    for T, D, Da in GEOMS:
        ns, sizes = align_shape(T, D, Da)
        for bit_exact in (False, True):
            for cls in (16, 4, 1):
                w = expect_word(cls, bit_exact, _has_s(T, D, Da))
                out.append(Case("align-%s-%s-al%d" % (_t(T, D, Da), "x" if bit_exact else "q", cls), T, D, Da, ns, bit_exact,
                                tuple(Call(n, cls, expect=w) for n in sizes)))
    return out


# ---- 2. layout changes under a running stream ------------------------------------------------------------------------------------------------
SWITCH_CLASSES = (16, 4, 1, 16, 4, 16)                          # Q -> B -> generic -> Q -> B -> Q (bit-exact handle: S in place of Q)
SWITCH_HOST_AT = 3                                              # the variant with a host-buffer call: made before this call


def switch_cases():
    out = []
    for tag, ns, nsamp, bit_exact in (("q", 264, 1600, False), ("s", 1024, 2400, True)):
        calls = [Call(nsamp, cls, expect=expect_word(cls, bit_exact)) for cls in SWITCH_CLASSES]
        out.append(Case("switch-%s-device" % tag, 64, 10, 5, ns, bit_exact, tuple(calls)))
        host = Call(nsamp, 16, device=False, expect=expect_word(16, bit_exact))     # (the staging rows are 256-byte aligned)
        out.append(Case("switch-%s-host" % tag, 64, 10, 5, ns, bit_exact, tuple(calls[:SWITCH_HOST_AT] + [host] + calls[SWITCH_HOST_AT:])))
    return out


# ---- 3. overlapped calls behind a different previous call -----------------------------------------------------------------------------------
TAIL = 777                                                      # every sequence ends with an odd-sized call without the flag (design B's: the phases are 0 before it)


def overlap_cases():
    """A call is overlapped only right behind a device-pointer call that design Q served (enqueue(): prev_by_q) and whose buffer can warm its runs up
    (fm_ovl_geometry_ok).  Behind a design-Q call the 16-byte alignment and the whole 16-byte pieces of that buffer always hold (design Q asks for
    aligned rows and multiples of 8 D Da samples), so only the length rule can decide there: "prev-short".  The cases with a 4-aligned previous
    buffer and with 3300 previous bytes are calls behind design B: the flag is refused for that reason first, and the two geometry terms are never
    the deciding ones — they are kept as sequences a host may produce, held bit for bit to the serial calls, not as cover of those terms."""
    q = lambda n, **kw: Call(n, 16, overlap=True, expect="fast-q", **kw)
    seqs = {
        # another size and another (16-multiple) stride: warmed up from that buffer
        "other-size-and-stride": (264, (Call(3200, 16, expect="fast-q"), q(1600, overlapped=True), q(2000, overlapped=True))),
        # the previous rows were 4-aligned only (design B's call)
        "prev-4-aligned": (264, (Call(1600, 16, expect="fast-q"), Call(1600, 4, expect="fast-b"), q(1600))),
        # the previous call is shorter than 2 D 128 bytes AND design Q's (512 streams x one step fill the machine): the length rule alone refuses the flag
        "prev-short": (512, (Call(1600, 16, expect="fast-q"), q(1200, overlapped=True), q(1600), q(1600, overlapped=True))),
        # 3300 bytes, nbytes % 16 = 4, both decimators back at phase 0 (design B's call)
        "prev-not-whole-pieces": (264, (Call(1600, 16, expect="fast-q"), Call(1650, 16, expect="fast-b"), q(1600))),
        # 200 streams x two steps do not fill the machine: design B serves 1600 samples, design Q the 3200 behind them.  That call is NOT overlapped: a warm-up
        # from design B's buffer would recompute the hand-over state with design Q's arithmetic and the first outputs would differ from the serial call's in
        # their last bits (what this case found: 1 ulp in outputs 0 .. 6 of most streams); the call behind it warms up from design Q's buffer
        "prev-served-by-b": (200, (Call(1600, 16, overlap=True, expect="fast-b"), q(3200), q(3200, overlapped=True))),
        # made through the host path: no device buffer to warm up from
        "prev-host": (264, (Call(1600, 16, expect="fast-q"), Call(1600, 16, device=False, expect="fast-q"), q(1600), q(1600, overlapped=True))),
        # the flag on an unaligned call: design B as if it were absent, and the aligned call behind it is not overlapped
        "flag-on-unaligned": (264, (Call(1600, 16, expect="fast-q"), Call(1600, 4, overlap=True, expect="fast-b"), q(1600), q(1600, overlapped=True))),
    }
    out = [Case("overlap-" + k, 64, 10, 5, ns, False, calls + (Call(TAIL, 16, expect="fast-b"),)) for k, (ns, calls) in seqs.items()]
    # design Q, design B, then a change of the assignment (which refills design Q's raw samples from design B's: hist_q_valid) right before the flagged
    # call: still a call behind design B, not overlapped; the one behind it is
    out.append(Case("overlap-prev-served-by-b-then-routed", 64, 10, 5, 264, False,
                    (Call(1600, 16, expect="fast-q"), Call(1600, 4, expect="fast-b"), q(1600, mixed="one"), q(1600, overlapped=True, mixed="one"),
                     Call(TAIL, 16, expect="fast-b")), 66, 2))
    return out


# ---- 4. canaries and odd-word audio rows ------------------------------------------------------------------------------------------------------
def canary_cases():
    q3 = tuple(Call(1600, 16, expect="fast-q") for _ in range(3))
    qo = (Call(1600, 16, expect="fast-q"),) + tuple(Call(1600, 16, overlap=True, expect="fast-q", overlapped=True) for _ in range(2))
    mix = lambda m: (Call(1600, 16, expect="fast-q"),) + tuple(Call(1600, 16, overlap=o, expect="fast-q", overlapped=o, mixed=m) for o in (False, True))
    return [
        Case("canary-q-first-and-steady", 64, 10, 5, 264, False, q3),
        Case("canary-q-overlapped", 64, 10, 5, 264, False, qo),
        Case("canary-mixed-one-launch", 64, 10, 5, 264, False, mix("one"), 66),
        Case("canary-mixed-two-launches", 48, 10, 5, 264, False, mix("two"), 66),
        Case("canary-s", 64, 10, 5, 1024, True, tuple(Call(2400, 16, expect="fast-s") for _ in range(2))),
        Case("canary-b-segments", 64, 10, 5, 8, True, tuple(Call(48000, 16, expect="fast-b") for _ in range(2))),
        Case("canary-generic", 64, 10, 5, 8, True, tuple(Call(48000, 1, expect="generic") for _ in range(2))),
    ]


# ---- 5. refused calls between valid ones ------------------------------------------------------------------------------------------------------
def refusal_cases():
    return [Case("refuse-q", 64, 10, 5, 264, False, tuple(Call(1600, 16, expect="fast-q") for _ in range(3))),
            Case("refuse-x", 64, 10, 5, 8, True, tuple(Call(n, 16, expect="fast-b") for n in (48000, 5008, 48000)))]


# ---- 6. one stream ------------------------------------------------------------------------------------------------------------------------------
ONE_NSAMP = 656000                                              # a multiple of 400 samples that holds 512 whole steps of 128 decimated outputs
ONE_OFFSETS = {0: 16, 4: 4, 6: 1}                               # byte offset of the row -> its class at iq_stride 0


def one_stream_cases():
    out = []
    for off, cls in ONE_OFFSETS.items():
        for bit_exact in (False, True):
            # (one stream never fills the machine for design S: design B serves the bit-exact handle's aligned row)
            w = expect_word(cls, bit_exact, has_s=False)
            out.append(Case("one-off%d-stride0-%s" % (off, "x" if bit_exact else "q"), 64, 10, 5, 1, bit_exact, (Call(ONE_NSAMP, cls, expect=w),)))
            # iq_stride 2 is no multiple of 4: the generic kernel whatever the offset
            out.append(Case("one-off%d-stride2-%s" % (off, "x" if bit_exact else "q"), 64, 10, 5, 1, bit_exact, (Call(ONE_NSAMP, 1, expect="generic"),)))
    return out


# ---- 7. the PCM call on unaligned input rows ---------------------------------------------------------------------------------------------------
PCM_NSAMP = 4400                                                # 14 quads of 32 decimated outputs: the fewest (>= 13) a run of the sink's chain needs, in whole units of 400
PCM_CLASSES = (16, 16, 4, 16, 1, 16)                            # "+ pcm" at calls 1, 3, 5 (the first call of a stream never holds the chain)


def pcm_cases():
    return [Case("pcm-switch", 64, 10, 5, 264, False, tuple(Call(PCM_NSAMP, cls, expect=expect_word(cls, False)) for cls in PCM_CLASSES))]


def all_cases():
    return align_cases() + switch_cases() + overlap_cases() + canary_cases() + refusal_cases() + one_stream_cases() + pcm_cases()


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
