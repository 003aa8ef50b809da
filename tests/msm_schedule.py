"""The scalar side of the MSM restated in Python integers and numpy (test infrastructure; tests/test_msm_schedule_host.py pins it,
tests/test_msm_schedule.py compares the five paths of the product's schedule with it).  Nothing of the product is used.

A scalar s < r is cut into nwin = BITS / c + 1 windows of c bits, least significant first: d = low c bits + carry; d > 2^(c-1) becomes d - 2^c with a
carry.  Digits lie in [-(2^(c-1) - 1), 2^(c-1)] and sum_w d_w 2^(c w) = s.  A non-zero digit d of scalar i in window w is one entry of bucket
(shared ? 0 : w 2^(c-1)) + |d| - 1; the entry is the word (d < 0) << 31 | (shared ? w << 24 : 0) | i.  counts = entries per bucket, offsets = their
exclusive prefix sum, sorted[offsets[b] .. offsets[b] + counts[b]) = the entries of bucket b in any order."""
import functools
import random

import numpy as np

import msm_edges
import oracle_lib as orc
from oracle_lib import FR

EMPTY = 0xFFFFFFFF                      # what cg_msm_schedule_dev leaves where no kernel wrote
PART_TILE = ITEM_TILE = 16384           # csrc/launchers.hpp, csrc/msm_sort_kernels.hpp: entries / items per workgroup of the partition sort
REGION = 512                            # buckets per region
ITEM_WINDOW = 2048                      # buckets an item tile histograms in LDS, from the region of its first item


def modulus(curve):
    return orc.MODULI[(curve, FR)]


def nwin_of(curve, c):
    return modulus(curve).bit_length() // c + 1


def nbuckets_of(c, nwin, shared):
    return (1 if shared else nwin) << (c - 1)


# ------------------------------------------------------------------------------------------------ digits
def digits_of_int(s, c, nwin):
    """(signed digits of s, least significant window first; the carry out of the top window) in Python integers"""
    half, out, carry = 1 << (c - 1), [], 0
    for w in range(nwin):
        d = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if d > half else 0
        out.append(d - (carry << c))
    return out, carry


def limbs_of(values):
    """(n, 4) uint64 little-endian limbs of integers below 2^256"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def window_bits(limbs, c, w):
    """bits [c w, c w + c) of every row of `limbs` as int64"""
    word, sh = divmod(c * w, 64)
    if word >= limbs.shape[1]:
        return np.zeros(limbs.shape[0], dtype=np.int64)
    v = limbs[:, word] >> np.uint64(sh)
    if sh + c > 64 and word + 1 < limbs.shape[1]:
        v = v | (limbs[:, word + 1] << np.uint64(64 - sh))
    return (v & np.uint64((1 << c) - 1)).astype(np.int64)


def signed_digits(limbs, c, nwin):
    """((nwin, n) int64 signed digits, (n,) carries out of the top window): digits_of_int for every row at once"""
    half = 1 << (c - 1)
    digs = np.empty((nwin, limbs.shape[0]), dtype=np.int64)
    carry = np.zeros(limbs.shape[0], dtype=np.int64)
    for w in range(nwin):
        d = window_bits(limbs, c, w) + carry
        carry = (d > half).astype(np.int64)
        digs[w] = d - (carry << c)
    return digs, carry


class Schedule:
    """the expected schedule of canonical scalars `limbs`: per entry its bucket and payload word (window-major, as enumerated), counts, offsets"""

    def __init__(self, limbs, c, nwin, shared):
        n = limbs.shape[0]
        assert n <= 1 << 24 or not shared
        digs, carry = signed_digits(limbs, c, nwin)
        assert not carry.any(), "a scalar below r never carries out of the top window"
        w, i = np.nonzero(digs)
        d = digs[w, i]
        self.c, self.nwin, self.shared, self.n = c, nwin, bool(shared), n
        self.nbuckets = nbuckets_of(c, nwin, shared)
        self.bucket = (0 if shared else w << (c - 1)) + np.abs(d) - 1
        self.payload = (i | ((w << 24) if shared else 0) | ((d < 0).astype(np.int64) << 31)).astype(np.uint32)
        self.counts = np.bincount(self.bucket, minlength=self.nbuckets).astype(np.uint32)
        self.total = int(self.bucket.size)
        self.offsets = exclusive_scan(self.counts)
        self._by_bucket = None

    def by_bucket(self):
        """the payload words ordered by (bucket, word): what a schedule's segments hold once each is sorted (computed once)"""
        if self._by_bucket is None:
            self._by_bucket = self.payload[np.lexsort((self.payload, self.bucket))]
        return self._by_bucket

    def direct_items(self):
        """entries that take the out-of-window branch of k_items_hist / k_items_scatter(_staged).  The partition groups the entries by region of 512
        buckets in region order, so which regions an item tile of 16384 holds follows from the counts alone: the window starts at the region of
        the tile's first item and covers four regions."""
        per_region = np.add.reduceat(self.counts.astype(np.int64), np.arange(0, self.nbuckets, REGION))
        ends = np.cumsum(per_region)
        starts = ends - per_region
        out = 0
        for t0 in range(0, self.total, ITEM_TILE):
            t1 = min(t0 + ITEM_TILE, self.total)
            first = int(np.searchsorted(ends, t0, side="right"))                 # region of item t0
            far = first + ITEM_WINDOW // REGION                                   # regions from here on are outside the window
            if far < len(starts):
                out += max(0, t1 - max(t0, int(starts[far])))
        return out


def exclusive_scan(counts):
    c = np.cumsum(counts, dtype=np.uint64)
    assert c.size == 0 or int(c[-1]) < 1 << 32
    return np.concatenate([np.zeros(1, dtype=np.uint64), c[:-1]]).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ comparisons (exact)
def first_bad(mask):
    return int(np.flatnonzero(mask)[0])


def check_dense(exp, counts, offsets, sorted_, what=""):
    """counts and offsets equal; bucket b's segment of `sorted_` holds bucket b's entries as a multiset; nothing was written behind the last entry"""
    bad = counts != exp.counts
    assert not bad.any(), f"{what}: counts[{first_bad(bad)}] = {counts[first_bad(bad)]}, expected {exp.counts[first_bad(bad)]} ({int(bad.sum())} buckets differ)"
    bad = offsets != exp.offsets
    assert not bad.any(), f"{what}: offsets[{first_bad(bad)}] = {offsets[first_bad(bad)]}, expected {exp.offsets[first_bad(bad)]} ({int(bad.sum())} buckets differ)"
    assert sorted_.size == exp.nwin * exp.n
    tail = sorted_[exp.total:] != EMPTY
    assert not tail.any(), f"{what}: position {exp.total + first_bad(tail)} behind the {exp.total} entries was written: {sorted_[exp.total + first_bad(tail)]:#x}"
    at = np.repeat(np.arange(exp.nbuckets, dtype=np.int64), exp.counts)            # the bucket that owns each position
    got = sorted_[:exp.total]
    got = got[np.lexsort((got, at))]
    bad = got != exp.by_bucket()
    if bad.any():
        k = first_bad(bad); b = int(at[k])
        lo, hi = int(exp.offsets[b]), int(exp.offsets[b]) + int(exp.counts[b])
        raise AssertionError(f"{what}: bucket {b} holds {sorted(hex(int(v)) for v in sorted_[lo:hi])[:8]}.., expected "
                             f"{sorted(hex(int(v)) for v in exp.payload[exp.bucket == b])[:8]}.. ({int(bad.sum())} entries differ)")


def check_direct(exp, cap, counts, offsets, sorted_, overflow, what=""):
    """one-pass scatter: true counts, offsets = exclusive scan of min(count, cap), the flag set exactly when a count exceeds cap; a bucket within cap
    holds its multiset in its first `count` slots, a bucket over cap holds cap distinct members; every other slot untouched"""
    bad = counts != exp.counts
    assert not bad.any(), f"{what}: counts[{first_bad(bad)}] = {counts[first_bad(bad)]}, expected {exp.counts[first_bad(bad)]}"
    kept = np.minimum(exp.counts, cap)
    want_off = exclusive_scan(kept)
    bad = offsets != want_off
    assert not bad.any(), f"{what}: offsets[{first_bad(bad)}] = {offsets[first_bad(bad)]}, expected {want_off[first_bad(bad)]} (scan of min(count, cap))"
    over = exp.counts > cap
    assert (overflow != 0) == bool(over.any()), f"{what}: overflow flag {overflow} with {int(over.sum())} buckets over cap = {cap}"
    slots = sorted_.reshape(exp.nbuckets, cap)
    filled = np.arange(cap)[None, :] < kept[:, None]
    assert (slots[~filled] == EMPTY).all(), f"{what}: a slot behind a bucket's entries was written"
    # buckets within cap: multisets, all at once
    inside = filled & ~over[:, None]
    b_of = np.broadcast_to(np.arange(exp.nbuckets, dtype=np.int64)[:, None], slots.shape)
    got, at = slots[inside], b_of[inside]
    order = np.lexsort((got, at))
    got, at = got[order], at[order]
    sel = ~over[exp.bucket]
    wb, wp = exp.bucket[sel], exp.payload[sel]
    want = wp[np.lexsort((wp, wb))]
    assert got.size == want.size
    bad = got != want
    assert not bad.any(), f"{what}: bucket {int(at[first_bad(bad)])} does not hold its entries ({int(bad.sum())} differ)"
    for b in np.flatnonzero(over):
        have, members = [int(v) for v in slots[b]], set(int(v) for v in exp.payload[exp.bucket == b])
        assert len(set(have)) == cap and set(have) <= members, f"{what}: overflowing bucket {b} does not hold {cap} distinct entries of its own"


# ------------------------------------------------------------------------------------------------ scalars
def from_digits(curve, c, digits):
    """the scalar with these signed window digits (least significant first; the representation is unique, so they are the digits it decomposes
    into), top digits dropped until it lies in [0, r)"""
    r, digits = modulus(curve), list(digits)
    assert all(-((1 << (c - 1)) - 1) <= d <= 1 << (c - 1) for d in digits)
    while True:
        v = sum(d * (1 << (c * w)) for w, d in enumerate(digits))
        if 0 <= v < r:
            return v
        digits[max(w for w, d in enumerate(digits) if d)] = 0


class Scalars:
    """canonical limbs for the restatement and Montgomery limbs (msm_edges.scalars_from_ints) for the device, for `index` into distinct values"""

    def __init__(self, curve, values, index=None):
        index = np.arange(len(values)) if index is None else np.asarray(index)
        self.limbs = limbs_of(values)[index]
        self.mont = np.ascontiguousarray(msm_edges.scalars_from_ints(curve, values)[index])
        self.n = len(index)


@functools.lru_cache(maxsize=None)
def uniform_pool(curve, n=1 << 18):
    rnd, r = random.Random(7100 + curve), modulus(curve)
    return Scalars(curve, [rnd.randrange(r) for _ in range(n)])


def take(pool, n, start=0):
    s = Scalars.__new__(Scalars)
    s.limbs, s.mont, s.n = pool.limbs[start:start + n], np.ascontiguousarray(pool.mont[start:start + n]), n
    assert s.limbs.shape[0] == n
    return s


def carry_scalars(curve, c, nwin):
    """a 2^c - 1 digit under a carry (d = 2^c: digit 0 and a carry), one to five such windows in a row, behind a first window that carries; and the
    same run started by a 2^(c-1) + 1 digit in window 1"""
    r, full, half, out = modulus(curve), (1 << c) - 1, 1 << (c - 1), []
    for first in (0, 1):
        for run in range(1, 6):
            v = ((half + 1) << (c * first)) + sum(full << (c * w) for w in range(first + 1, first + 1 + run)) + (3 << (c * (first + 1 + run)))
            if v < r and first + 1 + run < nwin:
                out.append(v)
    return out


def distribution(name, curve, c, nwin, n, boundary=None):
    """the named scalar vector of length n (see tests/test_msm_schedule.py)"""
    half = 1 << (c - 1)
    i = np.arange(n)
    if name == "uniform":
        return take(uniform_pool(curve), n)
    if name == "all equal":
        return Scalars(curve, [int.from_bytes(uniform_pool(curve).limbs[-1].tobytes(), "little")], np.zeros(n, dtype=np.int64))
    if name == "all zero":
        return Scalars(curve, [0], np.zeros(n, dtype=np.int64))
    if name == "boundary":
        return Scalars(curve, boundary, i % len(boundary))
    if name == "hot bucket":                               # 2^(c-1): the one digit that reaches the last bucket of a set, always positive
        return Scalars(curve, [from_digits(curve, c, [half] * nwin)], np.zeros(n, dtype=np.int64))
    if name == "staircase":                                # scalar i: digit (i mod 2^(c-1)) + 1 in every window
        k = min(n, half)
        return Scalars(curve, [from_digits(curve, c, [j + 1] * nwin) for j in range(k)], i % k)
    if name == "far regions":                              # digits 1, 2^(c-1) and -(2^(c-1) - 1): the first and the last region of every bucket set, two thirds in the last
        return Scalars(curve, [from_digits(curve, c, [(1, half, 1 - half)[(j + w) % 3] for w in range(nwin)]) for j in range(3)], i % 3)
    if name == "near regions":                             # digits 1 .. min(2048, 2^(c-1)): the first four regions of every bucket set
        k = min(ITEM_WINDOW, half)
        m = min(n, k)
        return Scalars(curve, [from_digits(curve, c, [(j * 7 + w * 131) % k + 1 for w in range(nwin)]) for j in range(m)], i % m)
    raise KeyError(name)
