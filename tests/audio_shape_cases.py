"""The cases tests/test_bcast_audio_shapes_gpu.py holds the conditioned broadcast kernels to their reference on, built
without a device so that tests/test_audio_shapes_cpu.py can look at the reference side alone.

A case is a shape of tests/pilot_shape_cases.py with that module's streams, rows, tuning, threshold and ragged cuts.  Before the row's first
byte every stream is put at a blend and a gain of its own by a jump that a reset completes, and then sent towards targets of its own —
distinct between the streams, none a power of two — at the handle's one slew:

    bt[s] = (5000 + 7001 s) mod 32769,           b0[s] = (bt[s] + 16384 + 300 s) mod 32769,
    vt[s] = (32768 - 3000 - 9001 s) mod 32769,   v0[s] = (vt[s] + 16384 + 500 s) mod 32769,        slew = max(1, 32768 div (A_long div 2))

with A_long the audio outputs of the case's long call.  A long call of fewer than SHORT = 64 audio outputs would take slew 32768 / 8; none
of the present shapes has one (the shortest, Da 64 at D 64, has 410: the long call is sized for 64 workgroups of two steps each).  Every
ramp of the seven streams covers 13885 units at the least and 19384 at the most, so it is moving at the long call's first output and over before its last, and
the longer of a stream's two is still moving two workgroup spans into it at every split the device may choose.  test_audio_shapes_cpu asserts all of that instead of
trusting the formula.

Two things here come from the condition test_audio_shapes_cpu holds the cases to — the right expectation must be more than 2 TOL away from
each wrong one somewhere in every stream — and not from taste:
  - the starts differ between the streams because ramps that leave one value at one slew are equal until the first arrives, and a
    counter and a const row of the D 64 shape carry audio in their first six outputs alone; and every gain ramp is long because many
    rows (carrier, counter, const, random) have as = 0, where the blend shows nothing;
  - the shape T1 D1 ... Da1 takes slew 4 instead of 1 (SLEW_FLOOR): its station and carrier rows stay below 0.3 rad, and one unit of a
    ramp moves an output by 2^-15 of that, 9e-6.
One stream cannot meet it by any choice: the const row of the D 64 shape, tuned half a cycle a sample away, has |am| + |as| <= 1.5e-8
throughout, so no blend or gain, right or wrong, moves its outputs by 2 TOL.  silent_streams names such streams from the reference alone.

The expected rows are tests/audio_ref.py's blend, every rounding on its own, of the am and as_ rows tests/tuned_ref.py's bcast_ref returns
for the case, under the b and v an audio_ref.AudioState gives when it is walked over the case's calls.  Beside them stand the two wrong
expectations the GPU comparison must be able to tell from the right one: the ramps one output further along (J + 1), and the streams'
records rotated by one (stream s under the starts and targets of stream s + 1)."""
import numpy as np

import audio_ref as ar
import pilot_shape_cases as ps
from test_bcast_shapes_gpu import _split

ONE = ar.ONE
SHORT, SHORT_SLEW = 64, ONE // 8
SLEW_FLOOR = {(1, 1, 1, 1, 1, 1, 1): 4}
WRONG = ("J + 1", "records rotated")

_ramps, _cases = {}, {}


def starts(ns):
    """(b0, v0) int64 [ns]"""
    s = np.arange(ns, dtype=np.int64)
    bt, vt = targets(ns)
    return (bt + ONE // 2 + 300 * s) % (ONE + 1), (vt + ONE // 2 + 500 * s) % (ONE + 1)


def targets(ns):
    """(bt, vt) int64 [ns]"""
    s = np.arange(ns, dtype=np.int64)
    return (5000 + 7001 * s) % (ONE + 1), (ONE - 3000 - 9001 * s) % (ONE + 1)


def call_bounds(shape, cuts):
    """the audio output index at which every call starts, and the row's count behind the last: the decimators run on from call to call"""
    D, Da = shape[1], shape[4]
    samples = np.concatenate([[0], np.cumsum([c // 2 for c in cuts])])
    return [int(n) // D // Da for n in samples]


def slew_of(shape, a_long):
    """(slew, which rule gave it)"""
    if a_long < SHORT:
        return SHORT_SLEW, "short"
    slew = max(1, ONE // (a_long // 2))
    if slew < SLEW_FLOOR.get(shape, 1):
        return SLEW_FLOOR[shape], "the shape's floor"
    return slew, "half the long call"


def state_at_start(ns, b0, v0, bt, vt, slew):
    """the AudioState of a handle put at (b0, v0) by a jump, reset, and set to (bt, vt) at the slew"""
    ref = ar.AudioState(ns)
    ref.set(b0, v0, ONE)
    ref.complete()
    ref.set(bt, vt, slew)
    return ref


def _walk(ns, b0, v0, bt, vt, slew, counts, J0=0):
    """(b, v) [ns, outputs] of that state, the set J0 outputs ago, walked over calls of `counts` outputs"""
    ref = state_at_start(ns, b0, v0, bt, vt, slew)
    ref.J = J0
    parts = [ref.call(c) for c in counts]
    return np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1)


def case_ramps(shape):
    """dict(ns, b0, v0, bt, vt, slew, rule, cuts, bounds, counts, a0, a1: the long call's first output and the one behind its last, span: the most
    audio outputs two workgroup spans of the long call cover at any split, b, v [ns, A] and wrong: {name: (b, v)}): integers alone, made
    once"""
    if shape not in _ramps:
        T, D, P, Ta, Da, Tr, Dr = shape
        idx = ps.BCAST_SHAPES.index(shape)
        ns = ps.BCAST_STREAMS[idx]
        steps = [ps.bcast_step(shape, tuned) for tuned in (False, True)]
        cuts, long_ = ps.ragged_cuts(D, steps[0]["H"], steps[0]["NDT"], ns, (Da, Dr), 700 + idx)      # bcast_case's own
        bounds = call_bounds(shape, cuts)
        counts = [int(v) for v in np.diff(bounds)]
        k = cuts.index(long_)
        a0, a1 = bounds[k], bounds[k + 1]
        slew, rule = slew_of(shape, a1 - a0)
        (b0, v0), (bt, vt) = starts(ns), targets(ns)
        M_long = long_ // 2 // D
        span_d = max(_split(M_long, st["NDT"], st["H"], ns, per_cu * ps.CUS)[1] for st in steps for per_cu in ps.PER_CU)
        b, v = _walk(ns, b0, v0, bt, vt, slew, counts)
        wrong = {WRONG[0]: _walk(ns, b0, v0, bt, vt, slew, counts, 1),
                 WRONG[1]: _walk(ns, *(np.roll(a, -1) for a in (b0, v0, bt, vt)), slew, counts)}
        for a in (b, v) + wrong[WRONG[0]] + wrong[WRONG[1]]:
            a.setflags(write=False)
        _ramps[shape] = dict(ns=ns, b0=b0, v0=v0, bt=bt, vt=vt, slew=slew, rule=rule, cuts=cuts, bounds=bounds, counts=counts, a0=a0, a1=a1,
                             span=-(-2 * span_d // Da), b=b, v=v, wrong=wrong)
    return _ramps[shape]


def _blend_rows(refs, b, v):
    rows = [ar.blend(r["stereo"]["am"], r["stereo"]["as_"], b[s], v[s]) for s, r in enumerate(refs)]
    out = np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows])
    for a in out:
        a.setflags(write=False)
    return out


def audio_case(pkg, shape):
    """dict(case: pilot_shape_cases.bcast_case, ramps: case_ramps, L, R: the expected rows float32 [ns, A], wrong: {name: (L, R)}), made
    once; the rows of bcast_case are shared with the unconditioned sweeps and left as they are"""
    if shape not in _cases:
        case, rm = ps.bcast_case(pkg, shape), case_ramps(shape)
        assert rm["cuts"] == case["cuts"] and rm["ns"] == case["ns"] and rm["b"].shape == (case["ns"], case["refs"][0]["L"].size)
        L, R = _blend_rows(case["refs"], rm["b"], rm["v"])
        _cases[shape] = dict(case=case, ramps=rm, L=L, R=R, wrong={k: _blend_rows(case["refs"], *rm["wrong"][k]) for k in WRONG})
    return _cases[shape]


def refs_blended(ac, L, R):
    """the case's per-stream references with L and R replaced (bb and the gate are what they were: blending touches neither)"""
    return [dict(r, L=L[s], R=R[s]) for s, r in enumerate(ac["case"]["refs"])]


def silent_streams(ac, keep_a):
    """the streams no conditioning can move by 2 TOL: |am| + |as| <= 2e-5 on every kept output (|beta|, |mu| <= 1 bound L and R by it)"""
    out = []
    for s, r in enumerate(ac["case"]["refs"]):
        level = np.abs(r["stereo"]["am"].astype(np.float64)) + np.abs(r["stereo"]["as_"].astype(np.float64))
        if not (level[keep_a[s]] > 2e-5).any():
            out.append(s)
    return out
