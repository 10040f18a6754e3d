"""Design Q's stage-aligned runs (csrc/sdrfm_fm_call.h: fm_q_runs' trailing inputs): an overlapped plain call is cut into fewer, longer runs than a serial call of
the same size.  Design Q's y is exact, so the audio must not depend on the cut: at 516 streams x the shortest calls whose count the rule changes (found with a
restatement of the rule below, on the library's own constants; tests/test_fm_runs_cpu.py pins the function itself), overlapped calls equal serial calls bit for
bit, both are the oracle's at the tolerance the design-Q tests hold, and a capture cut into two or three calls gives the same bits.
Rows (tests/test_q_taps_gpu.py: _rows): carriers, noise, constant bytes, a counter and the 127 / 128 row that sends every lane to the repair path.
The PCM-chain and mixed call forms keep the count they had (sdrfm.hip: the rule serves overlapped plain calls only); their own tests stand unchanged."""
import functools
import os
import re

import numpy as np
import pytest

import q_tap_sets as qt
import test_q_taps_gpu as tq
from conftest import scaled_err, TOL

pytestmark = pytest.mark.gpu

NS, ND = 516, 12
N_CU = 256
# per rate on an MI355X: the waves per CU a launch is cut for and the waves a CU holds by LDS (tests/native/fm_runs_check.cpp pins the planned geometry's figures)
Q_WAVES = {10: 12, 8: 12, 16: 11}
LDS_WAVES = {10: 15, 8: 14, 16: 11}


def _define(header, name):
    """the value of an unsigned #define of csrc/<header>: the constants below are the library's own, not copies"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"^#define %s (\d+)u" % name, open(os.path.join(root, "stm32f7-rtlsdr_amd", "csrc", header)).read(), re.M)
    assert m, name
    return int(m.group(1))


PARK = _define("sdrfm_q_host.h", "SDRFM_Q_PARK_STAGES")
RUN_VALU, STAGE_VALU, STEP_VALU = (_define("sdrfm_fm_call.h", "SDRFM_FM_Q_%s_VALU" % k) for k in ("RUN", "STAGE", "STEP"))


def _shape(M, runs, Da):
    """an overlapped call's longest run: quads, steps, stages (fm_q_run_shape)"""
    quads = -(-(((M + 7) // 8 + 3) // 4 + runs) // runs)
    steps = -(-quads // 4)
    return quads, steps, -(-steps // Da)


def _counts(M, ns, D):
    """-> runs per stream of a serial and of an overlapped plain call (fm_q_runs, the chain apart)"""
    Da = qt.RATES[D][0]
    steps, q_total = -(-M // 128), Q_WAVES[D] * N_CU
    min_steps = 4 if ns * (steps // 4) >= q_total // 2 else 2
    fill = max(1, min(q_total // ns, steps // min_steps))
    if min_steps != 4 or ns == 1 or fill == 1:
        return fill, fill
    best, best_cost, fill_stages = fill, None, _shape(M, fill, Da)[2]
    for r in range(fill, max(1, -(-LDS_WAVES[D] * N_CU // (2 * ns))) - 1, -1):
        _, sp, st = _shape(M, r, Da)
        if st > fill_stages or st > PARK:
            break
        cost = r * (RUN_VALU + STAGE_VALU * st + STEP_VALU * sp)
        if best_cost is None or cost < best_cost:
            best, best_cost = r, cost
    return fill, best


@functools.lru_cache(maxsize=None)
def _shortest(D, kind):
    """the shortest call (samples) at the rate whose count the rule changes and whose runs' last stage is full / one step short / the PARK-th / any"""
    Da = qt.RATES[D][0]
    want = {"full": lambda s, st: s % Da == 0, "short": lambda s, st: s % Da == Da - 1, "park": lambda s, st: st == PARK, "rate": lambda s, st: True}[kind]
    for k in range(1, 4000):
        M = 8 * Da * k
        was, now = _counts(M, NS, D)
        _, steps, stages = _shape(M, now, Da)
        if now != was and want(steps, stages):
            return 8 * D * Da * k
    raise AssertionError(kind)


CASES = [(64, 10, "full"), (64, 10, "short"), (64, 10, "park"), (26, 10, "park"), (27, 10, "short"), (64, 8, "rate"), (64, 16, "rate")]


@pytest.mark.parametrize("T,D,kind", CASES, ids=["T%d-D%d-%s" % c for c in CASES])
def test_overlapped_runs_of_another_length_give_the_same_bits(pkg, oracle_mod, T, D, kind):
    import torch
    assert int(torch.cuda.get_device_properties(0).multi_processor_count) == N_CU
    Da = qt.RATES[D][0]
    n = _shortest(D, kind)
    was, now = _counts(n // D, NS, D)
    assert now < was and _shape(n // D, now, Da)[2] <= PARK, (n, was, now)        # a shape at which the rule picks another count than the filling one
    print("T %d D %d %s: %d samples per call, %d runs per stream in a serial call, %d in an overlapped one (%d steps, %d stages)" % (
        (T, D, kind, n, was, now) + _shape(n // D, now, Da)[1:]))
    h, g = qt.plain_taps(pkg, T, D)
    rows = tq._rows(D, 3 * n)
    iq = np.tile(rows, (NS // ND, 1))
    d_iq = torch.from_numpy(iq).cuda()
    A = n // (D * Da)
    kw = dict(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=NS, max_bytes_per_call=4 * n)
    cuts = {"serial": [n, n, n], "three": [n, n, n], "two": [n, 2 * n]}
    out = {}
    for tag, cut in cuts.items():
        bufs = [torch.full((NS, c // (D * Da)), float("nan"), dtype=torch.float32, device="cuda") for c in cut]
        # (every call reads its own contiguous buffer: the previous call's stays intact beside it)
        parts, pos = [], 0
        for c in cut:
            parts.append(d_iq[:, 2 * pos:2 * (pos + c)].contiguous())
            pos += c
        torch.cuda.synchronize()
        with pkg.FmDemod(pkg.FmConfig(**kw)) as dm:
            names = []
            for part, buf in zip(parts, bufs):
                assert dm.process_batch_device(part, buf, overlap=(tag != "serial")) == buf.shape[1]
                names.append(dm.kernel_name)
            dm.flush()
            dm.synchronize()
        assert all(nm.startswith("fast-q") for nm in names), names
        assert all(("overlapped" in nm) == (tag != "serial") for nm in names[1:]), (tag, names)
        out[tag] = np.concatenate([b.cpu().numpy() for b in bufs], axis=1)
        assert out[tag].shape == (NS, 3 * A) and np.isfinite(out[tag]).all(), tag
    bits = {tag: np.ascontiguousarray(a).view(np.uint32) for tag, a in out.items()}
    assert np.array_equal(bits["three"], bits["serial"]), "overlapped calls differ from serial calls"
    assert np.array_equal(bits["two"], bits["serial"]), "a capture cut into two calls differs from the same capture cut into three"
    assert all(np.array_equal(bits["serial"][s_::ND], np.tile(bits["serial"][s_], (NS // ND, 1))) for s_ in range(ND)), "tiled copies differ"
    want = np.stack([oracle_mod.Oracle(h, g, D, Da).process(rows[s_]) for s_ in range(ND)])
    err = [scaled_err(out["three"][s_], want[s_]) for s_ in range(ND)]
    print("worst scaled error per row %s" % ["%.2g" % e for e in err])
    assert max(err) <= TOL, err
