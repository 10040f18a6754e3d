"""CPU checks of the plain-C RDS helpers (csrc/rds.c): the check word / syndrome identity, and the streaming decoder sdrfm_rds_sync_* on
synthetic basebands — one flipped bit costs exactly its block, no pilot and noise give no groups, any cut into pushes gives the same
groups, a reset forgets."""
import ctypes as C

import numpy as np
import pytest

from rds_ref import check_blocks

FS_BB = 9600.0
OFFSET_WORDS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)


def _baseband(pkg, bits, axis=0.7, amp=9e-3, noise=1e-3, seed=0, lead=300):
    """the complex baseband a station's bits leave behind the 57 kHz mixer: `lead` samples of noise, then amp r(t) e^{j axis} + noise,
    r the standard's data signal (siggen.rds_waveform) sampled at 9600 Hz"""
    ov = 128
    w = pkg.siggen.rds_waveform(bits, ov)
    n = int(len(bits) * FS_BB / 1187.5)
    pos = np.arange(n) * (1187.5 / FS_BB) * ov
    i0 = np.floor(pos).astype(np.int64)
    fr = pos - i0
    r = w[i0 % w.size] * (1 - fr) + w[(i0 + 1) % w.size] * fr
    rng = np.random.default_rng(seed)
    sig = np.concatenate([np.zeros(lead), amp * r]) * np.exp(1j * axis)
    sig = sig + noise * (rng.standard_normal(sig.size) + 1j * rng.standard_normal(sig.size))
    return sig.astype(np.complex64)


def _bits(pkg, groups, n_groups):
    return [b for i in range(n_groups) for b in pkg.rds_group_bits(groups[i % len(groups)])]


@pytest.fixture(scope="module")
def sent(pkg):
    return pkg.rds_encode_groups(0xABCD, "SYNCTEST", "one flipped bit.", pty=5)


def test_syndrome_of_a_block_is_its_offset_word(pkg):
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    infos = [0, 1, 0x8000, 0xFFFF, 0x5B9] + [int(v) for v in rng.integers(0, 1 << 16, 3000)]
    for off in range(5):
        for info in infos:
            cw = lib.sdrfm_rds_checkword(info, off)
            assert cw < 1024 and cw == pkg.rds_checkword(info, off)
            assert lib.sdrfm_rds_syndrome((info << 10) | cw) == OFFSET_WORDS[off], (info, off)
    assert lib.sdrfm_rds_checkword(1, 5) == 0xFFFF and lib.sdrfm_rds_checkword(1, -1) == 0xFFFF
    assert lib.sdrfm_rds_syndrome(0) == 0 and lib.sdrfm_rds_syndrome(1 << 10) == 0x5B9 & 0x3FF
    assert lib.sdrfm_rds_syndrome((0xFFFFFFFF << 26) & 0xFFFFFFFF) == 0          # only 26 bits count


def test_clean_baseband_decodes_on_any_axis(pkg, sent):
    for k, axis in enumerate((0.0, 0.7, np.pi / 2, 2.5, -1.2)):
        with pkg.RdsSync(FS_BB) as sync:
            got = sync.push(_baseband(pkg, _bits(pkg, sent, 14), axis=axis, seed=k))
        check_blocks(sent, got, 14, "axis %.2f" % axis)
        assert pkg.rds_parse(got) == dict(pi=0xABCD, pty=5, ps="SYNCTEST", text="one flipped bit.")


@pytest.mark.parametrize("block,bit", [(0, 0), (1, 15), (2, 16), (3, 25), (1, 7)])
def test_one_flipped_bit_clears_that_blocks_ok_bit_and_no_other(pkg, sent, block, bit):
    n_groups, hit = 12, 6
    bits = _bits(pkg, sent, n_groups)
    bits[104 * hit + 26 * block + bit] ^= 1
    with pkg.RdsSync(FS_BB) as sync:
        got = sync.push(_baseband(pkg, bits, seed=10 + block))
        st = sync.stats()
    assert len(got) == n_groups, [g.ok_mask for g in got]              # (acquisition takes the first block or two, never a whole group here)
    for i in range(2, n_groups):
        want = 0xF ^ (1 << block) if i == hit else 0xF
        assert got[i].ok_mask == want, (i, bin(got[i].ok_mask))
        for k in range(4):
            if got[i].ok_mask >> k & 1:
                assert got[i].blocks[k] == sent[i % len(sent)][k]
    assert st["blocks_failed"] == 1 and st["in_sync"]


# A false acquisition needs a window whose syndrome is one of the 5 offset words (5 of 1024) and, 26 bits later, the one word that follows
# it in the sequence (1 of 1024; 2 for B -> C | C'): 5.7e-6 per bit, 1.4 % for the 2400 bits of a 2 s capture of noise.  Without the
# sequence rule every capture would "synchronise" a dozen times.  The seeds are fixed, so the outcome is too.
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noise_gives_no_groups(pkg, seed):
    rng = np.random.default_rng(seed)
    n = int(2.05 * FS_BB)
    w = (9e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    with pkg.RdsSync(FS_BB) as sync:
        got = sync.push(w)
        st = sync.stats()
    assert got == [] and st["groups"] == 0 and not st["in_sync"], (got, st)
    assert st["bits"] >= 2400


def test_silence_behind_a_ramp_up_gives_no_groups(pkg):
    """what a mono station leaves: a few samples while the pilot filter ramps up, then exact zeros"""
    rng = np.random.default_rng(3)
    w = np.zeros(int(2.05 * FS_BB), np.complex64)
    w[:12] = 1e-3 * (rng.standard_normal(12) + 1j * rng.standard_normal(12))
    with pkg.RdsSync(FS_BB) as sync:
        assert sync.push(w) == [] and sync.stats()["groups"] == 0


def test_any_cut_into_pushes_gives_the_same_groups(pkg, sent):
    bits = _bits(pkg, sent, 20)
    bits[104 * 9 + 30] ^= 1
    w = _baseband(pkg, bits, axis=1.9, noise=2e-3, seed=20)
    with pkg.RdsSync(FS_BB) as sync:
        whole = sync.push(w)
        st_whole = sync.stats()
    assert len(whole) == 20
    rng = np.random.default_rng(21)
    for trial in range(4):
        cuts = np.sort(rng.integers(0, w.size, 40 if trial else 3))
        cuts = [0, 0] + [int(c) for c in cuts] + [w.size] if trial == 1 else [0] + [int(c) for c in cuts] + [w.size]
        with pkg.RdsSync(FS_BB) as sync:
            got = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                got += sync.push(w[a:b])
            assert got == whole and sync.stats() == st_whole, trial
    with pkg.RdsSync(FS_BB) as sync:                              # one sample per push
        got = []
        for i in range(0, 6000):
            got += sync.push(w[i:i + 1])
        got += sync.push(w[6000:])
        assert got == whole


def test_reset_forgets(pkg, sent):
    w = _baseband(pkg, _bits(pkg, sent, 10), seed=30)
    with pkg.RdsSync(FS_BB) as sync:
        first = sync.push(w)
        sync.push(w[: w.size // 3])
        assert sync.stats()["bits"] > 0
        sync.reset()
        st = sync.stats()
        assert st == dict(bits=0, blocks_ok=0, blocks_failed=0, in_sync=False, groups=0)
        assert sync.push(w) == first


def test_arguments(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    n = C.c_uint32()
    for rate in (0.0, 1000.0, 4749.0, 76001.0, float("nan"), float("inf")):
        assert lib.sdrfm_rds_sync_create(rate, C.byref(h)) == pkg.lib.EINVAL and not h.value
    assert lib.sdrfm_rds_sync_create(9600.0, None) == pkg.lib.EINVAL
    assert lib.sdrfm_rds_sync_reset(None) == pkg.lib.EINVAL
    assert lib.sdrfm_rds_sync_push(None, None, 0, None, 0, C.byref(n)) == pkg.lib.EINVAL
    assert lib.sdrfm_rds_sync_stats(None, None) == pkg.lib.EINVAL
    lib.sdrfm_rds_sync_destroy(None)
    assert lib.sdrfm_rds_sync_create(9600.0, C.byref(h)) == pkg.lib.OK
    assert lib.sdrfm_rds_sync_push(h, None, 4, None, 0, C.byref(n)) == pkg.lib.EINVAL
    assert lib.sdrfm_rds_sync_push(h, None, 0, None, 0, C.byref(n)) == pkg.lib.OK and n.value == 0
    lib.sdrfm_rds_sync_destroy(h)
    for rate in (4750.0, 19000.0, 76000.0):                       # 4 .. 64 samples per bit
        with pkg.RdsSync(rate) as sync:
            assert sync.stats()["bits"] == 0
