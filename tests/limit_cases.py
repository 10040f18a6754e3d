"""The cases the look-ahead PCM limiter's two forms are held to at every shape they accept, as pure numpy: the shapes, the
skewed interpolator tables, the rows that reach the largest sums, the lengths, and the host routine kept beside a device handle.  Shared by
tests/test_limit_cases_cpu.py (the host routines against the numpy definition, and the case list against the library's own refusals) and
tests/test_pcm_limit_shapes_gpu.py (the device against both).  Nothing here imports the package: what needs it takes `pkg` as an argument."""
import functools

import numpy as np

import limit_ref as ref
import limit_tp_ref as tpref
from limit_ref import CORNERS, CUTS, random_full_range  # noqa: F401  (re-exported for the tests)

TILE = 5120                                        # pairs of a tile of the kernels; the tests assert it is pkg.limit.TILE
HALF_MAX = 65535                                   # the bound of sdrfm_truepeak_check_coef on a half-row's sum of |coef|
SUM_MAX = 2 * HALF_MAX << 19                       # the largest |A| a table can give: 2 * 65535 * 2^19 < 2^36
PHASES = (2, 4, 8)
TAPS = tuple(range(4, 65, 4))
# per-stream (ceiling, release, gain): stream s of a batch takes corner s % 5
PARS = [(c, d, g) for c, g, d in CORNERS]


def sample_shapes():
    """every log2_window the sample form accepts"""
    return list(range(2, 9))


def tp_shapes():
    """every (lw, P, NT) the true-peak form accepts: P in {2, 4, 8}, NT a multiple of 4 in 4 .. 64, 2 <= lw <= 8 with 2^lw >= NT / 2"""
    return [(lw, P, NT) for P in PHASES for NT in TAPS for lw in range(2, 9) if (1 << lw) >= NT // 2]


def _half_row(rng, h, at_bound):
    """h magnitudes with a sum <= 65535, exactly 65535 with at_bound, and which of them have to be negative (only -32768 reaches 32768)"""
    if h == 2 and at_bound:                                               # 32767 + 32768 is the one way to 65535 with two taps
        m = np.array([32767, 32768] if rng.integers(0, 2) else [32768, 32767], np.int64)
        return m, m == 32768
    w = rng.random(h) ** 3 + 1e-3                                         # sizes over three decades
    m = np.minimum((w * (HALF_MAX if at_bound else rng.integers(20000, HALF_MAX + 1)) / w.sum()).astype(np.int64), 32767)
    if at_bound:
        for k in rng.permutation(h):                                      # what flooring and the cap of 32767 left over
            m[k] += min(HALF_MAX - int(m.sum()), 32767 - int(m[k]))
    return m, np.zeros(h, bool)


def skew_table(P, NT, seed, at_bound=False):
    """int16 [P, NT] with seeded random signs and sizes, asymmetric on purpose: no row is a row (itself included) reversed, so a detector that read
    the taps in the wrong order, or the rows in the wrong order, gives other values.  Every half-row's sum of |coef| is <= 65535, and exactly
    65535 with at_bound."""
    rng = np.random.default_rng([int(seed), P, NT, int(at_bound)])
    rows = []
    while len(rows) < P:
        halves = [_half_row(rng, NT // 2, at_bound) for _ in range(2)]
        m, neg = np.concatenate([h[0] for h in halves]), np.concatenate([h[1] for h in halves])
        row = np.where(neg | (rng.integers(0, 2, NT) > 0), -m, m)
        if not any(np.array_equal(row[::-1], r) for r in rows + [row]):
            rows.append(row)
    c = np.array(rows, dtype=np.int64)
    assert -32768 <= c.min() and c.max() <= 32767
    return np.ascontiguousarray(c, dtype=np.int16)


def table_is_skewed(c):
    c = np.asarray(c, dtype=np.int64)
    return not np.array_equal(c, c[::-1, ::-1]) and not any(np.array_equal(c[p], c[q][::-1]) for p in range(c.shape[0]) for q in range(c.shape[0]))


def half_sums(c):
    """the sums sdrfm_truepeak_check_coef bounds: int64 [P, 2]"""
    c = np.abs(np.asarray(c, dtype=np.int64))
    return c.reshape(c.shape[0], 2, c.shape[1] // 2).sum(axis=2)


def rail_burst(coef):
    """NT pairs on the rails, int16 [2 NT] interleaved: L's signs are row 0's taps', newest first (the last pair meets tap 0), so that under a gain
    of 65536 row 0's sum at the burst's last pair is sum_k |coef[0][k]| x 2^19 but for the positive rail's one LSB; R is the opposite"""
    c0 = np.asarray(coef, dtype=np.int64)[0][::-1]
    out = np.empty((c0.size, 2), np.int16)
    out[:, 0] = np.where(c0 < 0, -32768, 32767)
    out[:, 1] = np.where(c0 < 0, 32767, -32768)
    return out.reshape(-1)


def lengths(L, tile=TILE):
    """the smallest lengths at which a shape of latency L matters: one pair, around the lead-in, and a second tile of one pair"""
    return sorted({1, max(L - 1, 1), L, L + 1, tile + 1})


def table_for(kind, P, NT, seed=7):
    """(what the library is given, what the numpy definition is given) for a table named 'default', 'skew' or 'bound'"""
    if kind == "default":
        assert (P, NT) == (4, 12)
        return None, tpref.BS1770
    c = skew_table(P, NT, seed, kind == "bound")
    return c, c


# the cases both suites run against the numpy definition: (form, lw, P, NT, table)
DEFINITION_CASES = [("sample", 2, 0, 0, None), ("sample", 5, 0, 0, None), ("sample", 8, 0, 0, None),
                    ("truepeak", 2, 8, 4, "skew"), ("truepeak", 3, 4, 12, "default"), ("truepeak", 5, 2, 64, "bound"), ("truepeak", 8, 8, 64, "bound")]
DEFINITION_SECOND = 1500                           # pairs of the second call, from the carried state


def latency(lw, NT=0):
    return (1 << lw) - 1 + NT // 2


@functools.lru_cache(maxsize=None)
def definition_case(form, lw, P, NT, table, tile=TILE):
    """One call of tile + L + 2 pairs and one of 1500 from the carried state, the five CORNERS as five streams, a rail burst straddling pair `tile`,
    through the numpy definition: dict(x int16 [5, 2 n], cuts, coef (for the library), par [(C, delta, G, G)], out [call] int16 [5, 2 n_c],
    state [call] int32 [5, words], rec [call] the JOINED record tuples, peak: the definition's largest T (0 for the sample form)).  Computed once."""
    L = latency(lw, NT)
    cuts = (tile + L + 2, DEFINITION_SECOND)
    lib_c, ref_c = table_for(table, P, NT) if form == "truepeak" else (None, tpref.BS1770)
    burst = rail_burst(ref_c)
    rng = np.random.default_rng([91, lw, P, NT])
    x = random_full_range(rng, (len(CORNERS), 2 * sum(cuts)))
    at = tile - burst.size // 4
    x[:, 2 * at:2 * at + burst.size] = burst
    par = [(c, d, g, g) for c, d, g in PARS]
    out, state, rec, peak = [[], []], [[], []], [[], []], 0
    for s in range(len(CORNERS)):
        st, joined, a = None, None, 0
        for k, n in enumerate(cuts):
            xs = x[s, 2 * a:2 * (a + n)]
            r = ref.process(xs, lw, 1, 0, par[s], st) if form == "sample" else tpref.process(xs, lw, 1, 0, par[s], st, coef=ref_c)
            st = r[1]
            joined = r[2] if joined is None else ref.join(joined, r[2])
            out[k].append(r[0]), state[k].append(r[1]), rec[k].append(joined)
            if form == "truepeak":
                peak = max(peak, int(r[4].max()))
            a += n
    x.setflags(write=False)
    return dict(x=x, cuts=cuts, coef=lib_c, par=par, out=[np.stack(o) for o in out], state=[np.stack(s) for s in state], rec=rec, peak=peak)


class Host:
    """the host routine of either form beside a PcmLimiter: the parameters, J, the state and the records the handle should hold.  NT == 0 is the
    sample form; coef None with NT == 12 the default table."""

    def __init__(self, pkg, ns, lw, slew=1, NT=0, coef=None):
        self.pkg, self.ns, self.lw, self.slew, self.nt, self.coef = pkg, ns, lw, slew, NT, coef
        self.par = np.array([ref.DEFAULT] * ns, dtype=pkg.limit.LIMIT_PARAMS_DTYPE)
        self.J = 0
        self.reset()

    def reset(self):
        lim = self.pkg.limit
        self.state = lim.limit_tp_state_init(self.lw, self.nt, self.ns) if self.nt else lim.limit_state_init(self.lw, self.ns)
        self.rec = lim.limit_identity(self.ns)

    def set_params(self, ceiling=None, release=None):
        if ceiling is not None:
            self.par["ceiling"] = ceiling
        if release is not None:
            self.par["release"] = release

    def now(self):
        """the gain of every stream where its ramp has got to"""
        return [ref.ramp(int(p["gain0"]), int(p["gain_t"]), self.slew, self.J) for p in self.par]

    def set_gain(self, gain, jump=False):
        gain = np.broadcast_to(np.asarray(gain, np.uint32), (self.ns,))
        self.par["gain0"] = gain if jump else self.now()
        self.par["gain_t"] = gain
        self.J = 0

    def run(self, x, par=None, J=None):
        """the host routine on x from the state held, which stays: (out, state, records)"""
        par, J = self.par if par is None else par, self.J if J is None else J
        if self.nt:
            return self.pkg.pcm_limit_tp_host(x, self.lw, self.slew, J, par, self.state, self.rec, coef=self.coef)
        return self.pkg.pcm_limit_host(x, self.lw, self.slew, J, par, self.state, self.rec)

    def frozen(self, x):
        """what the call would give with every ramp frozen at the value of the call's first pair: the host routine under a jump to that value"""
        par = self.par.copy()
        par["gain0"] = par["gain_t"] = [ref.ramp(int(p["gain0"]), int(p["gain_t"]), self.slew, min(65536, self.J + 1)) for p in self.par]
        return self.run(x, par)[0]

    def call(self, x):
        out, self.state, self.rec = self.run(x)
        self.J = min(65536, self.J + x.shape[1] // 2)
        return out

    def holds(self, lim):
        """the handle's parameters, J, every state word and the four record fields are the host's"""
        par, J = lim.get_params()
        return (par.tobytes() == self.par.tobytes() and J == self.J and np.array_equal(lim.state(), self.state)
                and lim.read().tobytes() == self.rec.tobytes())


def pair(pkg, ns, lw, slew=1, NT=0, coef=None, pars=True):
    """a device handle and the host beside it, the streams taking the parameter corners in turn by a jump"""
    lim = pkg.PcmLimiter(ns, lw, slew, detect="truepeak", coef=coef) if NT else pkg.PcmLimiter(ns, lw, slew)
    host = Host(pkg, ns, lw, slew, NT, coef)
    if pars:
        p = [PARS[s % len(PARS)] for s in range(ns)]
        for k in (lim, host):
            k.set_params([c for c, _, _ in p], [d for _, d, _ in p])
            k.set_gain([g for _, _, g in p], jump=True)
    return lim, host


def under_ceiling(out, host):
    return bool((np.abs(np.asarray(out).astype(np.int64)).max(axis=1, initial=0) <= host.par["ceiling"]).all())
