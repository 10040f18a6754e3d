"""The raw-capture IQ meter's definition (include/sdrfm.h) restated in numpy with int64 and Python integers: the record, the
histogram row, and the two reports.  Nothing here calls the library."""
import math

import numpy as np

FIELDS = ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq", "rail_i", "rail_q")
REPORT_FIELDS = ("dc_i", "dc_q", "rms_dbfs", "total_dbfs", "rail_share_i", "rail_share_q", "gain_db", "skew_rad", "image_rejection_db")
# absolute floor of the 1e-9 bound, in each field's own unit
REL = 1e-9


def record(iq):
    """the record of one row of bytes [2n] as a tuple of Python ints in FIELDS' order (int64 sums: 2^25 pairs x 65025 < 2^42)"""
    b = np.asarray(iq, dtype=np.uint8).astype(np.int64)
    assert b.ndim == 1 and b.size % 2 == 0
    i, q = b[0::2], b[1::2]
    return (int(i.size), int(i.sum()), int(q.sum()), int((i * i).sum()), int((q * q).sum()), int((i * q).sum()),
            int(((i == 0) | (i == 255)).sum()), int(((q == 0) | (q == 255)).sum()))


def hist(iq):
    """the row of one row of bytes: int64 [512], the counts of bI = 0 .. 255 and then of bQ = 0 .. 255"""
    b = np.asarray(iq, dtype=np.uint8)
    return np.concatenate([np.bincount(b[0::2], minlength=256), np.bincount(b[1::2], minlength=256)]).astype(np.int64)


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def rec_tuple(r):
    """a numpy record of IQ_METER_DTYPE as a tuple of Python ints"""
    return tuple(int(r[f]) for f in FIELDS)


def ties(rec, row):
    """the four ties between a record (tuple) and a row (integers [512]): True when all hold"""
    h = [int(x) for x in row]
    b = range(256)
    ok = sum(h[:256]) == rec[0] and sum(h[256:]) == rec[0]
    ok = ok and sum(k * h[k] for k in b) == rec[1] and sum(k * h[256 + k] for k in b) == rec[2]
    ok = ok and sum(k * k * h[k] for k in b) == rec[3] and sum(k * k * h[256 + k] for k in b) == rec[4]
    return ok and h[0] + h[255] == rec[6] and h[256] + h[511] == rec[7]


def _db(x):
    return 10.0 * math.log10(x) if x > 0 else -math.inf


def report(rec):
    """sdrfm_iq_meter_report from a record tuple: dict of floats.  The central moments are exact integers divided once."""
    n, si, sq, sii, sqq, siq, ri, rq = rec
    if n == 0:
        return {f: math.nan for f in REPORT_FIELDS}
    vi, vq, cv = n * sii - si * si, n * sqq - sq * sq, n * siq - si * sq
    var_i, var_q, cov = vi / (n * n), vq / (n * n), cv / (n * n)
    out = {"dc_i": (2 * si - 255 * n) / (2 * n), "dc_q": (2 * sq - 255 * n) / (2 * n), "rail_share_i": ri / n, "rail_share_q": rq / n}
    out["rms_dbfs"] = _db((var_i + var_q) / 127.5 ** 2)
    out["total_dbfs"] = _db((var_i + var_q + out["dc_i"] ** 2 + out["dc_q"] ** 2) / 127.5 ** 2)
    if vi == 0 or vq == 0:
        out.update(gain_db=math.nan, skew_rad=math.nan, image_rejection_db=math.nan)
        return out
    rho = max(-1.0, min(1.0, cov / math.sqrt(var_i * var_q)))
    g = math.sqrt(var_q / var_i)
    out["gain_db"] = 10.0 * math.log10(var_q / var_i)
    out["skew_rad"] = math.asin(rho)
    c = 2.0 * g * math.cos(out["skew_rad"])
    den = 1.0 - c + g * g
    out["image_rejection_db"] = 10.0 * math.log10((1.0 + c + g * g) / den) if den > 0 else math.inf
    return out


def hist_report(row):
    """sdrfm_iq_hist_report from an accumulated row (integers [512]): dict"""
    h = [int(x) for x in row]
    n = sum(h[:256])
    assert n == sum(h[256:])
    out = {"n": n}
    for c, name in ((0, "i"), (1, "q")):
        hh = h[256 * c:256 * c + 256]
        if n == 0:
            out.update({"peak_" + name: math.nan, "level999_" + name: math.nan, "codes_" + name: math.nan, "headroom_db_" + name: math.nan})
            continue
        lev = [hh[127 - k] + hh[128 + k] for k in range(128)]          # level (2k + 1) / 255
        peak = max(k for k in range(128) if lev[k])
        cum, k999 = 0, None
        for k in range(128):
            cum += lev[k]
            if cum * 1000 >= n * 999:
                k999 = k
                break
        out["peak_" + name] = (2 * peak + 1) / 255
        out["level999_" + name] = (2 * k999 + 1) / 255
        out["codes_" + name] = float(sum(1 for x in hh if x))
        out["headroom_db_" + name] = -20.0 * math.log10((2 * k999 + 1) / 255)
    return out


def close(got, want):
    """the tests' bound on a report field: 1e-9 relative, or absolute in the field's own unit, whichever is larger — a deliberately loose bound
    on a few dozen double roundings over identical integers; NaN and infinities must agree exactly"""
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= REL * max(1.0, abs(want))
