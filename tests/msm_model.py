"""A plain model of the MSM's indexing (csrc/msm.hpp, csrc/group.hip): signed
window digits, the (bucket, entry) pair of every (point, window), the bucket
offsets, and how the accumulate's chunks cut the buckets.  Pure Python/numpy,
no GPU and no library: the GPU tests compare the device's grouping with it
and derive from it the accumulate units T that give a wanted chunk length.

The window width c is an argument: the model does not re-implement the cost
rule that picks it (msm_make_plan); the tests read the device's c back and
compare it with the c their table assumed.

Plan kinds (msm.hpp):
  window   one bucket range per digit window over the bases as they are: key
           boff[w] + |d| - 1, a zero digit key G (sorted after every bucket
           and not part of M), entry = the point index;
  shared   every window into ONE bucket set over window-shifted base copies
           2^(c w) P_i: key |d| - 1, a zero digit is the dummy entry in
           bucket 0, entry = w n + i;
  grouped  S copies kept: window w reads copy w mod S into bucket set w // S,
           key = set base + |d| - 1 (zero digit: the dummy in bucket 0 of its
           set), entry = (w mod S) n + i;
  batch    up to 4 independent MSMs of 64-bit scalars (segments), each a
           shared plan in its own bucket set: segment k's keys from k << s,
           its entries ioff + w wstride + i.
The sign of a digit is bit 31 of the entry.
"""
import numpy as np

DUMMY = 0x7FFFFFFF          # MSM_DUMMY
SIGN = 0x80000000
FIX_MAX = 8                 # MSM_FIX_MAX: the rule
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def chunk_len(M, T):
    """msm.hip chunk_len: ceil(M / T) rounded up to a multiple of 4, 4 when M = 0."""
    return ((M + T - 1) // T + 3) // 4 * 4 if M else 4


def units_for(M, K):
    """The T that cuts M entries into chunks of K: ceil(M / K), at least 1."""
    return max(1, (M + K - 1) // K)


def merge_levels(T):
    """msm_back_impl: the smallest l with 4^l >= T (0 for T = 1: no merge launch)."""
    l = 0
    while 4 ** l < T:
        l += 1
    return l


class Plan:
    """The bucket layout of one plan.  kind in window / shared / grouped /
    batch; bits in {64, 255}; c the window width; copies (grouped) the base
    copies kept; nseg (batch) the segments."""

    def __init__(self, kind, bits, c, copies=0, nseg=1):
        assert kind in ("window", "shared", "grouped", "batch") and bits in (64, 255)
        self.kind, self.bits, self.c = kind, bits, c
        self.sw = 1 if bits == 64 else 4
        self.nwin = (bits + c - 1) // c
        self.top = bits - c * (self.nwin - 1)          # width of the unsigned top window
        self.nseg = 1
        if kind == "window":
            self.shared = 0
            self.nb = [1 << (c - 1)] * (self.nwin - 1) + [1 << self.top]
            self.boff = [0]
            for v in self.nb:
                self.boff.append(self.boff[-1] + v)
            self.G = self.boff[-1]
            self.copies, self.nsets, self.setsize = 1, self.nwin, 0
            return
        self.shared = 1
        k = max(c - 1, self.top)                       # signed digits <= 2^(c-1), the top one <= 2^top
        self.setsize = 1 << k
        self.copies, self.nsets = self.nwin, 1
        if kind == "grouped" and 0 < copies < self.nwin:
            self.copies = copies
            self.nsets = (self.nwin + copies - 1) // copies
        if kind == "batch":
            assert bits == 64 and 1 <= nseg <= 4
            self.nseg, self.nsets = nseg, nseg
        self.G = self.nsets * self.setsize

    def set_weight_exp(self, t):
        """The host tail weighs bucket set t by 2^this (a batch's sets are separate sums)."""
        return 0 if self.kind == "batch" else self.c * self.copies * t


def limbs_of(values):
    """Python ints -> (n, 4) uint64 little-endian limbs."""
    return np.array([[(int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values],
                    dtype=np.uint64).reshape(-1, 4)


def ints_of(limbs):
    return [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in np.asarray(limbs, dtype=np.uint64)]


def _window(limbs, off, width):
    """Bits [off, off + width) of every scalar (msm.hpp scal_window)."""
    wd, sh = off >> 6, off & 63
    lo = limbs[:, wd] >> np.uint64(sh)
    if sh + width > 64 and wd + 1 < limbs.shape[1]:
        lo = lo | (limbs[:, wd + 1] << np.uint64(64 - sh))
    return (lo & np.uint64((1 << width) - 1)).astype(np.int64)


def digits(plan, limbs):
    """Signed digits (group.hip gs_digit): (mag, neg), each (n, nwin).  A
    window value v = bits + carry above 2^(c-1) becomes -(2^c - v) with a carry
    into the next window; the top window is unsigned and takes the last carry."""
    limbs = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    n, c = len(limbs), plan.c
    mag = np.zeros((n, plan.nwin), dtype=np.int64)
    neg = np.zeros((n, plan.nwin), dtype=bool)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(plan.nwin):
        top = w == plan.nwin - 1
        v = _window(limbs, c * w, plan.top if top else c) + carry
        flip = (v > (1 << (c - 1))) & (not top)
        mag[:, w] = np.where(flip, (1 << c) - v, v)
        neg[:, w] = flip
        carry = flip.astype(np.int64)
    return mag, neg


def digits_value(plan, mag, neg):
    """sum_w +-mag[w] 2^(c w) per scalar, as Python ints."""
    out = []
    for m, s in zip(mag.tolist(), neg.tolist()):
        out.append(sum((-d if f else d) << (plan.c * w) for w, (d, f) in enumerate(zip(m, s))))
    return out


class Grouping:
    """Every entry of one MSM under a plan, and what the device derives from
    them.  segs (batch only): [(limbs, ioff, wstride)], wstride 0 = the
    segment's own length; otherwise limbs is the one scalar vector."""

    def __init__(self, plan, limbs=None, segs=None):
        self.plan = plan
        if plan.kind != "batch":
            segs = [(limbs, 0, 0)]
        assert len(segs) == plan.nseg
        keys, ents = [], []
        self.n = 0
        for k, (sl, ioff, wstride) in enumerate(segs):
            sl = np.asarray(sl, dtype=np.uint64).reshape(-1, 4)
            n = len(sl)
            self.n += n
            mag, neg = digits(plan, sl)
            i = np.arange(n, dtype=np.int64)[:, None]
            w = np.arange(plan.nwin, dtype=np.int64)[None, :]
            sign = np.where(neg, SIGN, 0).astype(np.int64)
            if plan.kind == "window":
                key = np.where(mag > 0, np.array(plan.boff[:-1], dtype=np.int64)[None, :] + mag - 1, plan.G)
                ent = (i + 0 * w) | sign
            else:
                ws = wstride if wstride else n
                base = (k if plan.kind == "batch" else w // plan.copies) * plan.setsize
                key = base + np.where(mag > 0, mag - 1, 0)
                ent = np.where(mag > 0, (ioff + (w % plan.copies) * ws + i) | sign, DUMMY)
            keys.append(key.reshape(-1))
            ents.append(ent.reshape(-1))
        key = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
        ent = np.concatenate(ents) if ents else np.zeros(0, dtype=np.int64)
        live = key < plan.G                       # a per-window plan's zero digits sort after every bucket
        key, ent = key[live], ent[live]
        order = np.lexsort((ent, key))            # by bucket; inside a bucket by entry (a multiset's canonical order)
        self.key = key[order].astype(np.uint32)
        self.ent = ent[order].astype(np.uint32)
        self.M = len(self.key)
        self.off = np.zeros(plan.G + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.key, minlength=plan.G), out=self.off[1:])
        self.off = self.off.astype(np.uint32)

    def spans(self, T):
        """(K, P) with P[b] = chunks bucket b spans under T units (0: empty)."""
        K = chunk_len(self.M, T)
        off = self.off.astype(np.int64)
        lo, hi = off[:-1], off[1:]
        P = np.where(hi > lo, (hi - 1) // K - lo // K + 1, 0)
        return K, P

    def chunking(self, T, fix_max=FIX_MAX):
        """What the back of the MSM does under (T, fix_max)."""
        K, P = self.spans(T)
        return {"K": K, "T": T, "nbig": int((P > fix_max).sum()), "max_span": int(P.max()) if len(P) else 0,
                "split": int((P > 1).sum()), "by_boundary": self.plan.G > T, "nlevels": merge_levels(T),
                "spans": P}


def canonical(key, ent):
    """(key, ent) in the model's order: by bucket, inside a bucket by entry."""
    key, ent = np.asarray(key, dtype=np.uint32), np.asarray(ent, dtype=np.uint32)
    order = np.lexsort((ent, key))
    return key[order], ent[order]


def bucket_sum(plan, grouping, bases, r=R, seg=None):
    """The MSM over integers mod r in place of points, through the model's
    buckets: sum_sets 2^(c S t) sum_b (b + 1) sum_entries +-base.  bases: the
    integers b_i (a batch: the list of every segment's, and seg names the
    segment whose sum is wanted).  A shared plan's entry j n + i names copy j of
    base i, 2^(c j) b_i."""
    def copies_of(b):
        n = len(b)
        return [(int(b[i]) << (plan.c * j)) % r for j in range(plan.copies) for i in range(n)]

    total = 0
    key, ent = grouping.key.astype(np.int64), grouping.ent.astype(np.int64)
    if plan.kind == "window":
        win = np.searchsorted(np.array(plan.boff, dtype=np.int64), key, side="right") - 1
        for g, e, w in zip(key.tolist(), ent.tolist(), win.tolist()):
            v = int(bases[e & 0x7FFFFFFF])
            total += (g - plan.boff[w] + 1) * (-v if e & SIGN else v) << (plan.c * w)
        return total % r
    ext = copies_of(bases[seg]) if plan.kind == "batch" else copies_of(bases)
    for g, e in zip(key.tolist(), ent.tolist()):
        t, b = divmod(g, plan.setsize)
        if e == DUMMY or (plan.kind == "batch" and t != seg):
            continue
        v = ext[e & 0x7FFFFFFF]
        total += ((b + 1) * (-v if e & SIGN else v)) << plan.set_weight_exp(t)
    return total % r
