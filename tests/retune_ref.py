"""Loader of tests/native/retune_ref.c — the scalar-C definition of a re-tuned stream's d: one stream from its first byte
under a list of events — and the composition of that d with tests/tuned_ref.py's bcast_ref into the broadcast handle's L, R and bb across
the events.  The C file is compiled once per process into a temporary directory (gcc -O2 -ffp-contract=off).

An event is a dict: n0 (the input sample before which it acts; or m0, the d before which it acts: n0 = m0 D), hz (2T floats, (hr[k], hi[k])
pairs), rot, carry ((cr, ci), (1, 0) by default), restart (False by default).  Events are given in the order they are made."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import tuned_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def _load():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="retune_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libretune_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-Wall", "-fPIC", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "native", "retune_ref.c"), "-lm"], check=True, cwd=ROOT, capture_output=True, text=True)
        lib = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        lib.retune_ref_d.argtypes = [vp, u32, u32, u32, u32, vp, C.c_int, C.c_float, u32, vp, vp, vp, vp, vp, vp, vp]
        lib.retune_ref_d.restype = u32
        _lib = lib
    return _lib


def event(hz, rot, m0=None, n0=None, carry=(1.0, 0.0), restart=False):
    assert (m0 is None) != (n0 is None)
    return dict(n0=int(n0) if n0 is not None else None, m0=int(m0) if m0 is not None else None, hz=np.ascontiguousarray(hz, np.float32).reshape(-1),
                rot=np.float32(rot), carry=np.asarray(carry, np.float32).reshape(2), restart=bool(restart))


def _n0(ev, D):
    return ev["n0"] if ev["n0"] is not None else ev["m0"] * D


def retune_d(iq, D, H, events, h=None, hz=None, rot=0.0):
    """(d[0 .. M), views [len(events), M], m0 of every event): the stream starts with the real taps h, or with the tuned taps hz and rot;
    views[e][:m0[e]] is what the stages behind d see of the earlier d's after event e"""
    iq = np.ascontiguousarray(iq, np.uint8)
    assert (h is None) != (hz is None)
    t0 = np.ascontiguousarray(h if h is not None else hz, np.float32).reshape(-1)
    T = t0.size if h is not None else t0.size // 2
    M, n = iq.size // 2 // D, len(events)
    n0 = np.array([_n0(e, D) for e in events], np.uint32)
    assert (np.diff(n0.astype(np.int64)) >= 0).all() and (n == 0 or n0[-1] <= iq.size // 2), n0
    ev_hz = np.ascontiguousarray(np.stack([e["hz"] for e in events]) if n else np.zeros((1, 2 * T)), np.float32)
    assert ev_hz.shape[1] == 2 * T
    ev_rot = np.array([e["rot"] for e in events] or [0], np.float32)
    ev_carry = np.ascontiguousarray(np.stack([e["carry"] for e in events]) if n else np.zeros((1, 2)), np.float32)
    ev_restart = np.array([e["restart"] for e in events] or [0], np.uint8)
    d, views = np.empty(M, np.float32), np.zeros((max(n, 1), M), np.float32)
    got = _load().retune_ref_d(iq.ctypes.data, iq.size // 2, T, D, H, t0.ctypes.data, int(h is not None), float(np.float32(rot)), n, n0.ctypes.data,
                               ev_hz.ctypes.data, ev_rot.ctypes.data, ev_carry.ctypes.data, ev_restart.ctypes.data, d.ctypes.data, views.ctypes.data)
    assert got == M
    return d, views[:n], (n0 // D).astype(np.int64)


def retune_bcast(iq, shape, taps, pilot_min, events, h=None, hz=None, rot=0.0):
    """the broadcast handle's outputs of one stream across the events: dict(d, L, R, bb, keep_a, keep_r, n_amb, count, m0).  The outputs
    whose newest d lies in [m0[e], m0[e + 1]) are tuned_ref.bcast_ref's on views[e][:m0[e]] followed by d[m0[e]:]; keep_a / keep_r flag the
    outputs none of whose d's is gate-ambiguous in that segment's reference (tuned_ref.ambiguous, clean_outputs), n_amb counts those d's,
    count the d's the gate is open for and lo those of them that are not ambiguous, each in the segment it belongs to."""
    T, D, P, Ta, Da, Tr, Dr = shape
    _, ga, gr, b, dg, rg = taps
    H = P - 1 + max(Ta, Tr) - 1
    d, views, m0 = retune_d(iq, D, H, events, h=h, hz=hz, rot=rot)
    M = d.size
    starts = [0] + [int(m) for m in m0] + [M + 1]
    out = None
    for k in range(len(starts) - 1):
        lo, hi = (0 if k == 0 else starts[k]), starts[k + 1]
        if hi <= lo:
            continue                                               # (an event directly behind another: no d between them)
        dk = d if k == 0 else np.concatenate([views[k - 1][:lo], d[lo:]])
        r = tuned_ref.bcast_ref(dk, b, ga, gr, pilot_min, dg, rg, Da, Dr)
        amb = tuned_ref.ambiguous(r["rds"])
        ka, kr = tuned_ref.clean_outputs(amb, r["L"].size, Ta, Da), tuned_ref.clean_outputs(amb, r["bb"].size, Tr, Dr)
        on = r["rds"]["pw"] >= r["rds"]["pmin2"]
        if out is None:
            out = dict(d=d, L=r["L"].copy(), R=r["R"].copy(), bb=r["bb"].copy(), keep_a=ka.copy(), keep_r=kr.copy(), n_amb=0, count=0, lo=0, m0=m0)
        na, nr = (np.arange(r["L"].size) + 1) * Da - 1, (np.arange(r["bb"].size) + 1) * Dr - 1
        sa, sr_ = (na >= lo) & (na < hi), (nr >= lo) & (nr < hi)
        for name in ("L", "R"):
            out[name][sa] = r[name][sa]
        out["bb"][sr_] = r["bb"][sr_]
        out["keep_a"][sa], out["keep_r"][sr_] = ka[sa], kr[sr_]
        seg = slice(lo, min(hi, M))
        out["n_amb"] += int(amb[seg].sum())
        out["count"] += int(on[seg].sum())
        out["lo"] += int((on & ~amb)[seg].sum())
    return out
