"""The shapes, rows, slot tables and call scripts the PCM mix bus's CPU and GPU tests share.  Every shape is the smallest at which
k_pcm_mix can still go wrong: around one workgroup's SPAN = 2048 pairs (a lane's eight pairs, the last wave's ragged end, a second and a third
workgroup), every slot count's ends, every mode, dead slots beside live ones, and rows at every address a 4-byte aligned row can have mod 16."""
import numpy as np

SPAN = 2048                                    # SDRFM_PCM_MIX_SPAN
ONE = 32768
NONE = 0xFFFFFFFF
N_VALUES = (0, 1, 2, 3, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3, 4800)
SHAPES = ((1, 1, 1), (3, 2, 2), (2, 5, 8), (7, 3, 3))          # (n_in, n_bus, n_slots)
SLEWS = (1, 7, 32768)
IDENTITY_SLEWS = (1, 2, 3, 7, 255, 256, 32767, 32768)
OFFSETS = (0, 4, 8, 12)                        # a row's address mod 16, in bytes
CANARY = 0x5A5B


def cuts(n):
    """the cut of a run of n pairs into calls: (0, 1, SPAN - 1, SPAN + 2, rest)"""
    head = (0, 1, SPAN - 1, SPAN + 2)
    assert n > sum(head)
    return head + (n - sum(head),)


def rows(seed, n_in, n, kind="random"):
    """int16 [n_in, 2n]: random over the full range, or one of the two constant rails"""
    if kind == "random":
        return np.random.default_rng(seed).integers(-32768, 32768, (n_in, 2 * n), dtype=np.int64).astype(np.int16)
    return np.full((n_in, 2 * n), {"rail_lo": -32768, "rail_hi": 32767}[kind], np.int16)


def slot_table(seed, n_in, n_bus, n_slots, first_mode=0):
    """[n_bus][n_slots] of (src, mode, g0, gt): the modes in turn from first_mode; of every four slots the third has no source and the fourth a
    source but no gain; slot 1 of bus 0 shares slot 0's source; the gains are 0, 32768 or anywhere between, at rest or on their way"""
    rng = np.random.default_rng(1000 + seed)
    table = []
    for b in range(n_bus):
        bus = []
        for k in range(n_slots):
            src = int(rng.integers(n_in))
            mode = (first_mode + b * n_slots + k) % 5
            g0, gt = (int(v) for v in rng.choice([0, ONE, int(rng.integers(1, ONE)), int(rng.integers(1, ONE))], 2))
            if k % 4 == 2:
                src = NONE
            elif k % 4 == 3:
                g0 = gt = 0
            elif g0 == 0 and gt == 0:
                gt = ONE
            if b == 0 and k == 1:
                src = bus[0][0]
            bus.append((src, mode, g0, gt))
        table.append(bus)
    return table


def as_arrays(table):
    """a slot table -> (src, mode, g0, gt) as uint32 [n_bus, n_slots] each"""
    a = np.array(table, dtype=np.uint64).astype(np.uint32)
    return a[..., 0].copy(), a[..., 1].copy(), a[..., 2].copy(), a[..., 3].copy()


class HostMixer:
    """the handle's bookkeeping on plain values around the C host routine (pkg.pcm_mix_host): what a PcmMixer must equal call for call"""

    def __init__(self, pkg, n_in, n_bus, n_slots, slew, curve=None):
        self.pkg, self.n_in, self.n_bus, self.n_slots, self.slew, self.curve = pkg, n_in, n_bus, n_slots, slew, curve
        self.slots = np.zeros((n_bus, n_slots), pkg.MIX_SLOT_DTYPE)
        self.slots["src"] = NONE
        self.J = 0
        self.rec = np.zeros(n_bus, pkg.MIX_DTYPE)

    def set_routes(self, src=None, mode=None):
        if src is not None:
            self.slots["src"] = np.broadcast_to(np.asarray(src, dtype=np.uint32), self.slots.shape)
        if mode is not None:
            self.slots["mode"] = np.broadcast_to(np.asarray(mode, dtype=np.uint32), self.slots.shape)

    def set_gains(self, target, jump=False):
        import pcm_mix_ref as ref
        target = np.broadcast_to(np.asarray(target, dtype=np.uint32), self.slots.shape)
        for idx in np.ndindex(self.slots.shape):
            g0, gt = int(self.slots["g0"][idx]), int(self.slots["gt"][idx])
            self.slots["g0"][idx] = int(target[idx]) if jump else ref.ramp(g0, gt, self.slew, self.J)
            self.slots["gt"][idx] = int(target[idx])
        self.J = 0

    def load(self, table):
        """a slot table as create + set_routes + two set_gains leave it: the ramps at g0, on their way to gt, J = 0"""
        src, mode, g0, gt = as_arrays(table)
        self.set_routes(src, mode)
        self.set_gains(g0, jump=True)
        self.set_gains(gt)

    def crossfade(self, bus, src, mode="stereo"):
        k, srcs, modes, target = self.pkg.mix.crossfade_plan(self.slots, self.J, self.slew, bus, src, mode)
        self.set_routes(srcs, modes)
        self.set_gains(target)
        return k

    def holds(self, mixer):
        """the device handle's slots and J are this one's"""
        sl, J = mixer.slots()
        return sl.tobytes() == self.slots.tobytes() and J == self.J

    def process_batch(self, x):
        out, self.rec = self.pkg.pcm_mix_host(x, self.slots, self.slew, self.J, self.curve, acc=self.rec)
        self.J = min(65536, self.J + x.shape[1] // 2)
        return out

    def read(self, reset=False):
        rec = self.rec.copy()
        if reset:
            self.rec[:] = 0
        return rec


def load(mixer, table):
    """the same on a PcmMixer"""
    src, mode, g0, gt = as_arrays(table)
    mixer.set_routes(src, mode)
    mixer.set_gains(g0, jump=True)
    mixer.set_gains(gt)
