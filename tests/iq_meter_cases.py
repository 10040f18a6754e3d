"""Rows and shapes the raw-capture IQ meter's CPU and GPU tests share.  The shapes sit on the edges of the launch geometry in
csrc/sdrfm_iq_meter.h: the 16-byte vector, the 4096-byte step of a workgroup, and a workgroup's whole share of a row."""
import numpy as np

VEC, CHUNK = 16, 4096                                    # IQM_VEC, IQM_CHUNK
SMALL = (2, 4, 14, 16, 18, 30, 32, 34)                   # around one and two vectors
STEP = (CHUNK - 2, CHUNK, CHUNK + 2)                     # one step of a workgroup, and that +- 2
OFFSETS = tuple(range(18))                               # row start offsets in bytes: every residue of 16, and both parities twice
CUTS = (2, 0, 16, 4098)                                  # a capture cut into calls of these sizes and the rest


def random_rows(seed, n_streams, nbytes):
    """uint8 [n_streams, nbytes]: uniform bytes with the rails made likelier (one byte in 16 is forced to 0 or 255)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n_streams, nbytes), dtype=np.uint8)
    force = rng.integers(0, 16, size=x.shape) == 0
    x[force] = np.where(rng.integers(0, 2, size=int(force.sum())) == 0, 0, 255).astype(np.uint8)
    return x


def ramp():
    """all 65536 (I, Q) byte pairs, I the slow index: uint8 [131072]"""
    k = np.arange(65536, dtype=np.uint32)
    out = np.empty(131072, np.uint8)
    out[0::2], out[1::2] = k >> 8, k & 255
    return out


def constant(value, nbytes):
    return np.full(nbytes, value, np.uint8)


def share_bytes(geometry, n_streams, steps=3):
    """nbytes at which a workgroup's share of a row of n_streams is exactly `steps` steps and every workgroup has one: bps * steps * CHUNK, with
    bps what the geometry then gives"""
    nbytes = CHUNK * steps
    for _ in range(64):
        bps, share = geometry(n_streams, nbytes)
        if share == steps * 256 and bps * share * VEC == nbytes:
            return nbytes
        nbytes = bps * steps * CHUNK
    raise AssertionError("no such shape")


# ---- impaired captures for the report's recovery checks -------------------------------------------------------------------------------------------
IMPAIR = dict(dc_i=2.3, dc_q=-1.7, gain_q=1.05, skew_rad=np.deg2rad(3.0))
N_PAIRS = 240000


def stations_capture(pkg, seed):
    """three off-centre stations plus noise, 0.1 s at 2.4 MS/s, through IMPAIR: uint8 [2 N_PAIRS]"""
    groups = pkg.rds_encode_groups(0x3000 + seed, "IQMETER%d" % (seed % 10))
    st = [dict(offset_hz=off, amplitude=amp, left_hz=lh, right_hz=rh, groups=groups)
          for off, amp, lh, rh in ((-600e3, 34.0, 1e3, 3.1e3), (250e3, 28.0, 700.0, 2.3e3), (820e3, 22.0, 1.9e3, 440.0))]
    return pkg.impair_iq(pkg.make_iq_stations(N_PAIRS, st, seed=seed)[0], **IMPAIR)


def noise_capture(pkg, seed):
    """noise only, sigma 20 LSB per component, through IMPAIR: uint8 [2 N_PAIRS]"""
    rng = np.random.default_rng(1000 + seed)
    x = np.clip(np.rint(127.5 + rng.normal(0.0, 20.0, size=2 * N_PAIRS)), 0, 255).astype(np.uint8)
    return pkg.impair_iq(x, **IMPAIR)
