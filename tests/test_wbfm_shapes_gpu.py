"""GPU sweep of the WBFM handle (sdrfm_wbfm_*) over prototype lengths and resampler ratios: every (P, Tg, L, M) below against
oracle.WbfmOracle on every stream, band and sample, ragged chunked calls bitwise one call, the kernel each case is meant to reach
(k_wbfm_steps, k_wbfm_fused, the generic pair) and the fused kernels bitwise the generic pair; two long runs of a few hundred calls."""
from contextlib import closing

import numpy as np
import pytest

from conftest import scaled_err
from test_wbfm_gpu import _check_all

pytestmark = pytest.mark.gpu

FS = 3.2e6
STEPS, FUSED, GENERIC = "k_wbfm_steps", "k_wbfm_fused", "wbfm-generic"
CASES = [  # (P, Tg, L, M), the kernel that must serve a call of >= 64 channelizer steps
    ((128, 60, 6, 24), STEPS),      # 4 L = M
    ((128, 20, 2, 8), STEPS),
    ((128, 40, 4, 25), STEPS),
    ((128, 7, 3, 256), STEPS),
    ((128, 510, 51, 204), STEPS),   # HD = 10 and 10 L <= 512 both at their edge
    ((128, 60, 6, 23), FUSED),      # 4 L just above M
    ((128, 30, 3, 2), FUSED),       # L > M
    ((128, 10, 1, 1), FUSED),
    ((128, 5, 1, 7), FUSED),
    ((128, 66, 6, 25), GENERIC),    # HD = 11
    ((128, 512, 52, 256), GENERIC),  # 10 L > 512
    ((16, 1, 1, 1), GENERIC),
    ((144, 60, 6, 25), GENERIC),
    ((512, 512, 64, 1), GENERIC),   # every maximum, 64x upsampling
]


def _taps(pkg, P, Tg, L, M):
    p = pkg.lowpass_taps(P, 0.5 / 16 * 0.8)
    g = pkg.lowpass_taps(Tg, 0.5 / max(L, M) * 0.8) * np.float32(L)
    return p, g


def _inputs(pkg, ns, nsamp, first_id):
    """fm and random streams in turn"""
    return np.stack([pkg.make_iq(1, nsamp, mode=("fm", "random")[s % 2], fs=FS, first_id=first_id + s)[0] for s in range(ns)])


def _demod(pkg, p, g, L, M, ns, nbytes, **kw):
    return closing(pkg.WbfmDemod(pkg.WbfmConfig(proto_coeffs=p, resamp_coeffs=g, resamp_up=L, resamp_down=M, n_streams=ns,
                                        max_bytes_per_call=nbytes, **kw)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _against_oracle(oracle_mod, got, iq, p, g, L, M, where):
    worst = 0.0
    for s in range(iq.shape[0]):
        want = oracle_mod.WbfmOracle(p, g, L, M).process(iq[s])
        _check_all(got[s], want, "%s stream %d" % (where, s))
        worst = max(worst, scaled_err(got[s], want))
    return worst


def _ragged(rng, nbytes):
    """even chunk sizes that cover nbytes: 0 and 2 bytes, calls shorter than 64 channelizer steps (2048 bytes), long ones"""
    sizes, pos = [0, 2, 30, 2046, 2048, 2050], 0
    while sum(sizes) < nbytes:
        sizes.append(2 * int(rng.choice([int(rng.integers(0, 1024)), int(rng.integers(1024, 12000))])))
    out = []
    for c in sizes:
        c = min(c, nbytes - pos)
        out.append(c)
        pos += c
    return out


@pytest.mark.parametrize("case,kernel", CASES, ids=["P%d-Tg%d-L%d-M%d" % c for c, _ in CASES])
def test_ratio_against_oracle_chunks_and_kernels(pkg, oracle_mod, case, kernel):
    P, Tg, L, M = case
    idx = [c for c, _ in CASES].index(case)
    ns = (1, 5, 8)[idx % 3]
    nsamp = 16 * (1500 if L > 32 else 4000) + 2 * idx + 1       # an odd number of samples: a partial channelizer step at the end
    nbytes = 2 * nsamp
    p, g = _taps(pkg, P, Tg, L, M)
    iq = _inputs(pkg, ns, nsamp, 200 + 10 * idx)
    with _demod(pkg, p, g, L, M, ns, nbytes) as dm:
        assert kernel in dm.kernel_name, (dm.kernel_name, case)            # what the configuration selects
        one = dm.process_batch(iq)
        name = dm.kernel_name
        assert kernel in name, (name, case)                                # what served the call
        worst = _against_oracle(oracle_mod, one, iq, p, g, L, M, name)
        # ragged chunks == one call
        dm.reset()
        parts, pos, names = [], 0, set()
        for c in _ragged(np.random.default_rng(idx), nbytes):
            parts.append(dm.process_batch(iq[:, pos:pos + c]))
            pos += c
            if c:
                names.add(dm.kernel_name)
        assert pos == nbytes
        got = np.concatenate(parts, axis=2)
        assert got.shape == one.shape and np.array_equal(_bits(got), _bits(one)), (name, len(parts))
        assert any(kernel in n for n in names) and any(GENERIC in n for n in names), names
    if kernel != GENERIC:
        with _demod(pkg, p, g, L, M, ns, nbytes, force_generic=True) as gen:
            other = gen.process_batch(iq)
            assert gen.kernel_name.startswith(GENERIC), gen.kernel_name
        assert np.array_equal(_bits(other), _bits(one)), name
    print("%s P%d Tg%d L%d/M%d: %d streams x 16 bands x %d samples, worst scaled error %.3g; %d ragged calls bitwise one call%s" % (
        name, P, Tg, L, M, ns, one.shape[2], worst, len(parts), "" if kernel == GENERIC else "; bitwise the generic pair"))


@pytest.mark.parametrize("case,kernel", [((128, 40, 4, 25), STEPS), ((128, 30, 3, 2), FUSED)], ids=["steps-4-25", "fused-3-2"])
def test_long_run_of_calls(pkg, oracle_mod, case, kernel):
    """>= 200 calls of varied length (short ones on the generic pair, long ones on the fused kernel) == one call, bitwise; the oracle on
    the whole stream"""
    P, Tg, L, M = case
    ns = 5
    rng = np.random.default_rng(L * 100 + M)
    sizes = [2 * int(rng.choice([int(rng.integers(0, 1024)), int(rng.integers(1024, 3000))])) for _ in range(240)]
    nbytes = sum(sizes)
    p, g = _taps(pkg, P, Tg, L, M)
    iq = _inputs(pkg, ns, nbytes // 2, 900)
    with _demod(pkg, p, g, L, M, ns, nbytes) as dm:
        one = dm.process_batch(iq)
        assert kernel in dm.kernel_name, dm.kernel_name
        dm.reset()
        parts, pos, served = [], 0, 0
        for c in sizes:
            parts.append(dm.process_batch(iq[:, pos:pos + c]))
            pos += c
            served += kernel in dm.kernel_name and c > 0
    got = np.concatenate(parts, axis=2)
    assert got.shape == one.shape and np.array_equal(_bits(got), _bits(one))
    assert served >= 50, served
    worst = _against_oracle(oracle_mod, got, iq, p, g, L, M, "long run")
    print("%s L%d/M%d: %d calls (%d on the fused kernel) bitwise one call; %d x 16 x %d samples, worst scaled error %.3g" % (
        kernel, L, M, len(sizes), served, ns, got.shape[2], worst))
