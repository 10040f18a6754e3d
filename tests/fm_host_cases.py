"""The cases of tests/test_fm_host_paths_gpu.py as a table: one stream's bytes handed to the FM handle through its three host-buffer paths — mapped rows
(sdrfm_process up to 65 536 bytes), staged rows (above that, or SDRFM_CFG_NO_ZEROCOPY) and the pinned ring (sdrfm_ring_submit / _collect) — cut into
ladders of call sizes that are built from the rules of csrc/sdrfm_fm_call.h, with the first word of the kernel name each call is expected to reach.
tests/test_fm_host_cases_cpu.py runs every ladder of a 32-audio-tap geometry through those rules on the CPU (tests/native/fm_shape_cases.cpp) and checks
that each ladder still holds every class of call it was built for; the GPU test asserts kernel_name against the same entries.

All three paths hand enqueue() rows whose pointer and stride are multiples of 16 bytes (the mapped and staging rows are 256-byte aligned; the ring gives
its slots' allocated size as the stride), so one word stands for all three.  Design S never serves these calls: one stream needs 1024 waves of 63 lane
segments of 480 samples, 31 million samples in one call."""
from collections import namedtuple

import fm_shape_cases as fs

Geom = namedtuple("Geom", "T D Ta Da")
GEOMS = (Geom(64, 10, 32, 5),                                    # designs Q and B and the generic kernel
         Geom(16, 10, 32, 5),
         Geom(64, 8, 32, 8),                                     # (design Q's swizzled ring: no one-stream call here is long enough for it)
         Geom(7, 3, 5, 4),                                       # generic only
         Geom(128, 16, 64, 6))
FLAGS = ("default", "bit_exact", "force_generic")
N_CU = 256                                                       # the device the words are stated for
ZC_MAX = 65536                                                   # sdrfm.hip: SDRFM_ZC_MAX, the mapped path's largest call
STEP_OUT = 128                                                   # sdrfm_fm_call.h: SDRFM_FM_Q_STEP_OUT


def names_words(g):
    """the table names a kernel word where tests/native/fm_shape_cases.cpp can check it: it plans at 32 audio taps"""
    return g.Ta == 32


def y_aff(g):
    return (g.T + g.D - 1) // g.D + 1                            # fm_y_aff


def slot_stride(slot_bytes):
    """the stride sdrfm_ring_submit passes: the slot's allocated size (a multiple of 256)"""
    return (slot_bytes + 255) & ~255


# one call of a ladder: bytes, the counts and the state before it, the expected word (None: the table names none, or N = 0), the classes it stands for
Call = namedtuple("Call", "nbytes N M A phase_x phase_d n_seen word tags")


class Walk:
    """One stream's state carried from call to call as enqueue() carries it (fm_counts), and the word fm_serve / fm_bx reach for one stream on 16-aligned rows."""

    def __init__(self, g, flags):
        self.g, self.flags = g, flags
        self.phase_x = self.phase_d = self.n_seen = 0
        self.calls = []

    def counts(self, nbytes):
        g, N = self.g, nbytes // 2
        M, px = divmod(self.phase_x + N, g.D)
        A, pd = divmod(self.phase_d + M, g.Da)
        return N, M, A, px, pd

    def word(self, nbytes, cls=16):
        g = self.g
        N, M, A, _, _ = self.counts(nbytes)
        if N == 0 or not names_words(g):
            return None
        if self.flags == "force_generic":
            return "generic"
        start = self.n_seen + 1 < g.T
        short_first = start and M < y_aff(g) + g.Ta               # fm_short_first (every 32-audio-tap geometry here has design B)
        fast_ok = A > 0 and self.phase_x % 2 == 0 and cls >= 4 and not short_first
        q_fit = (self.flags == "default" and A > 0 and self.phase_x == 0 and self.phase_d == 0 and N % (8 * g.D * g.Da) == 0 and cls == 16 and M >= g.Ta
                 and (not start or M >= y_aff(g) + g.Ta) and (M + STEP_OUT - 1) // STEP_OUT >= 2 * N_CU)
        return "fast-q" if q_fit else "fast-b" if fast_ok else "generic"

    def add(self, nbytes):
        assert nbytes % 2 == 0
        g = self.g
        N, M, A, px, pd = self.counts(nbytes)
        tags = set()
        if N == 0:
            tags.add("zero")
        else:
            if A == 0:
                tags.add("no-audio")
            if self.n_seen == 0 and N == 1:
                tags.add("one-sample")
            if self.n_seen + 1 < g.T:
                tags.add("start-kept" if self.n_seen + N + 1 < g.T else "start-crossed")
            if self.n_seen == 0 and M == y_aff(g) + g.Ta - 1:
                tags.add("short-first-below")
            if self.n_seen == 0 and M == y_aff(g) + g.Ta:
                tags.add("short-first-at")
            if N % 2:
                tags.add("odd-count")
            if self.phase_x % 2:
                tags.add("odd-phase")
                if px % 2 == 0:
                    tags.add("phase-restored")
            if self.n_seen + 1 >= g.T and self.phase_x % 2 == 0 and A > 0:   # a call design B takes on 4-aligned rows: the stride's class decides
                tags.add("ring-2mod4" if nbytes % 4 == 2 else "ring-%dmod16" % (nbytes % 16))
            if nbytes in (ZC_MAX - 2, ZC_MAX, ZC_MAX + 2):
                tags.add("switch-%d" % nbytes)
        word = self.word(nbytes)
        if word == "fast-q":
            tags.add("design-q")
        self.calls.append(Call(nbytes, N, M, A, self.phase_x, self.phase_d, self.n_seen, word, frozenset(tags)))
        self.n_seen += N
        self.phase_x, self.phase_d = px, pd

    def to_parity(self, parity, around=1):
        """the smallest call of at least `around` samples that leaves phase_x with this parity"""
        n = next(n for n in range(around, around + 2 * self.g.D + 2) if (self.phase_x + n) % self.g.D % 2 == parity)
        self.add(2 * n)

    def even(self):
        if self.phase_x % 2:
            self.to_parity(0)


BASE = 4000                                                      # a steady call: 2000 samples, a multiple of 16 bytes
CLASS_TAGS = ("ring-0mod16", "ring-4mod16", "ring-8mod16", "ring-12mod16", "ring-2mod4")
MAIN_TAGS = ("one-sample", "start-kept", "start-crossed", "zero", "no-audio", "odd-count", "odd-phase", "phase-restored",
             "switch-65534", "switch-65536", "switch-65538") + CLASS_TAGS


def main_ladder(g, flags):
    w = Walk(g, flags)
    # the start of a stream: one sample, calls that keep n_seen + 1 < T (the last one leaves phase_x even where a size does), the call that crosses it
    # with M >= y_aff + Ta — the fast kernel and the generic fix-up of the first tiles —, then nothing at all
    w.add(2)
    small = max(1, (g.T - 3) // 3)
    w.add(2 * small)
    fits = [n for n in (small + 1, small, small + 2, small - 1) if n >= 1 and w.n_seen + n + 1 < g.T]
    w.add(2 * next((n for n in fits if (w.phase_x + n) % g.D % 2 == 0), fits[0]))
    w.add(2 * g.D * (y_aff(g) + g.Ta + g.Da))
    w.add(0)
    # every alignment class of a chunk's own length, each at an even phase_x
    for r in (0, 4, 8, 12):
        w.even()
        w.add(BASE + r)
    # an odd sample count: the next call starts at an odd phase_x (a small call makes it odd where the decimation is odd and did not), which
    # fm_fast_ok refuses; that call brings the phase back to even
    w.even()
    w.add(BASE + 2)
    if w.phase_x % 2 == 0:
        w.to_parity(1, 3)
    w.to_parity(0, BASE // 2 + 3)
    w.add(4)                                                     # samples, no audio
    # the switch from mapped to staged rows
    for nbytes in (ZC_MAX - 2, ZC_MAX, ZC_MAX + 2):
        w.even()
        w.add(nbytes)
    w.even()
    w.add(BASE + 96)
    return w.calls


def short_first_ladder(g, flags, at):
    """a fresh stream whose first call has M = y_aff + Ta - 1 (generic entirely) or y_aff + Ta (the fast kernel and the fix-up), and the stream behind it"""
    w = Walk(g, flags)
    w.add(2 * g.D * (y_aff(g) + g.Ta - 1 + (1 if at else 0)))
    w.even()
    w.add(BASE)
    w.even()
    w.add(BASE + 2)
    if w.phase_x % 2 == 0:
        w.to_parity(1, 3)
    w.to_parity(0, 3)
    w.add(BASE + 8)
    return w.calls


def q_ladder(g, flags):
    w = Walk(g, flags)
    for _ in range(2):
        w.add(2 * fs.ONE_NSAMP)                                   # 513 steps: the smallest one-stream call design Q accepts on 256 CUs
    return w.calls


Case = namedtuple("Case", "name geom flags ladder mode calls must")


def _name(g, flags, ladder, mode):
    return "T%d-D%d-Ta%d-Da%d-%s-%s-%s" % (g.T, g.D, g.Ta, g.Da, flags, ladder, mode)


def all_cases():
    out = []
    for g in GEOMS:
        for flags in FLAGS:
            if flags == "force_generic" and g != GEOMS[0]:
                continue
            ladders = [("main", main_ladder(g, flags), MAIN_TAGS),
                       ("below", short_first_ladder(g, flags, False), ("short-first-below", "odd-phase", "phase-restored")),
                       ("at", short_first_ladder(g, flags, True), ("short-first-at", "odd-phase", "phase-restored"))]
            for ladder, calls, must in ladders:
                modes = ("fm", "random", "const") if (ladder, flags) == ("main", "default") else ("fm",)
                out += [Case(_name(g, flags, ladder, m), g, flags, ladder, m, tuple(calls), must) for m in modes]
    g = GEOMS[0]
    out.append(Case(_name(g, "default", "q", "fm"), g, "default", "q", "fm", tuple(q_ladder(g, "default")), ("design-q",)))
    return out


def slot_bytes(case):
    return max(c.nbytes for c in case.calls)


def n_slots(case):
    """3 slots; 2 where the ladder has no more calls than that (a submit must meet a full ring)"""
    return 3 if sum(1 for c in case.calls if c.N) > 3 else 2


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
