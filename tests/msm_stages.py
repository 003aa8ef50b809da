"""The point side of the MSM restated in Python integers and numpy (test infrastructure; tests/test_msm_stages_host.py pins it against the oracle,
tests/test_msm_stages.py compares what cg_msm_stages_dev downloads with it).  Written from DESIGN.md §3, "The point side's intermediate format";
nothing of the product is used.

Row j of a test table is k_j G with known k_j (k_j = 0: the point at infinity), so every bucket, piece and partial sum is (an integer mod r) G.  The
restatement computes those integers; `points_of` turns them into packed affine records with ONE oracle multiplication per distinct value."""
import random

import numpy as np

import msm_edges
import msm_schedule as ms
import oracle_lib as orc
from oracle_lib import FR

EMPTY = 0xFFFFFFFF
SEGMENTS, BITSUM, GRID = 0, 1, 2                                  # reduction kinds of the geometry record
KINDS = {SEGMENTS: "segments", BITSUM: "bit sums", GRID: "grid"}
UNTOUCHED = 2                                                     # state of a continuation piece no kernel wrote


# ------------------------------------------------------------------------------------------------ integers -> points
_points = {}


def points_of(curve, group, values):
    """packed affine records (len(values), words) of value G; 0 (mod r) is infinity = the all-zero record.  Each distinct value is multiplied once."""
    r = ms.modulus(curve)
    values = [int(v) % r for v in values]
    cache = _points.setdefault((curve, group), {0: np.zeros(orc.point_words(curve, group), dtype=np.uint64)})
    new = sorted(set(values) - cache.keys())
    if new:
        g = orc.generator_mul(curve, group, msm_edges.scalars_from_ints(curve, [1])[0])
        out = orc.points_mul(curve, group, np.broadcast_to(g, (len(new), g.size)).copy(), msm_edges.scalars_from_ints(curve, new))
        cache.update(zip(new, out))
    if not values:
        return np.zeros((0, orc.point_words(curve, group)), dtype=np.uint64)
    return np.stack([cache[v] for v in values])


class Table:
    """rows k_j G"""

    def __init__(self, curve, group, ks):
        r = ms.modulus(curve)
        self.curve, self.group, self.ks = curve, group, [int(k) % r for k in ks]
        self.rows = len(self.ks)

    def points(self):
        return points_of(self.curve, self.group, self.ks)

    def has_infinity(self):
        return 0 in self.ks


def random_table(curve, group, rows=256, seed=1, infinity_every=0):
    rnd, r = random.Random(9000 + seed + 7 * curve), ms.modulus(curve)
    return Table(curve, group, [0 if infinity_every and j % infinity_every == 1 else rnd.randrange(1, r) for j in range(rows)])


def degenerate_table(curve, group, rows=256):
    """equal, opposite and infinite operands at every stage: k = 1, 1, r - 1, 2, 0 repeated"""
    r = ms.modulus(curve)
    return Table(curve, group, [(1, 1, r - 1, 2, 0)[j % 5] for j in range(rows)])


# ------------------------------------------------------------------------------------------------ schedules
class StageSchedule:
    """counts, offsets and sorted of ONE schedule in the format of DESIGN §3 (compact: cap = 0; padded: bucket b owns slots [b cap, b cap + min(count,
    cap))), and `entries` = its entry words bucket by bucket, as lists"""

    def __init__(self, curve, c, shared, per_bucket, cap=0):
        self.curve, self.c, self.shared, self.cap = curve, c, bool(shared), cap
        self.nwin = ms.nwin_of(curve, c)
        self.nb = 1 << (c - 1)
        self.nbuckets = ms.nbuckets_of(c, self.nwin, shared)
        assert len(per_bucket) == self.nbuckets
        self.per_bucket = per_bucket                                   # list of uint32 arrays: ALL entries of each bucket
        self.counts = np.array([len(e) for e in per_bucket], dtype=np.uint32)
        self.kept = np.minimum(self.counts, cap) if cap else self.counts.copy()   # the entries that exist
        self.offsets = ms.exclusive_scan(self.kept)
        self.total = int(self.kept.sum(dtype=np.uint64))
        if cap:
            self.sorted = np.full(self.nbuckets * cap, EMPTY, dtype=np.uint32)
            for b in np.flatnonzero(self.counts):
                k = int(self.kept[b])
                self.sorted[b * cap:b * cap + k] = per_bucket[b][:k]
        else:
            self.sorted = np.concatenate([np.asarray(e, dtype=np.uint32) for e in per_bucket] + [np.zeros(0, dtype=np.uint32)])
        self.words = self.sorted if not cap else np.concatenate([np.asarray(per_bucket[b][:int(self.kept[b])], dtype=np.uint32) for b in range(self.nbuckets)] + [np.zeros(0, dtype=np.uint32)])
        self.bucket_of = np.repeat(np.arange(self.nbuckets, dtype=np.int64), self.kept)   # the bucket that owns each list position

    def arrays(self):
        return self.counts, self.offsets, self.sorted

    def padded(self, cap):
        return StageSchedule(self.curve, self.c, self.shared, self.per_bucket, cap)

    def values(self, table):
        """the integer every existing entry adds, by list position: +- k_index, times 2^(c window) when the windows share the bucket set"""
        r = ms.modulus(self.curve)
        w = self.words.astype(np.int64)
        idx = w & (0xFFFFFF if self.shared else 0x7FFFFFFF)
        win = (w >> 24) & 0x7F if self.shared else np.zeros_like(w)
        neg = (w >> 31) & 1
        assert idx.size == 0 or int(idx.max()) < table.rows
        out = []
        for j, ww, n in zip(idx.tolist(), win.tolist(), neg.tolist()):
            v = table.ks[j] << (self.c * ww)
            out.append((-v if n else v) % r)
        return out


def from_counts(curve, c, shared, counts, table_rows, rng, pool=0):
    """a schedule with exactly these bucket sizes and random payloads (index, sign, and the window when the windows share the set).  pool > 0: the
    buckets draw their payload lists at random from `pool` lists, so that large bucket sets have few distinct expected points."""
    nwin = ms.nwin_of(curve, c)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.size == ms.nbuckets_of(c, nwin, shared)

    def payload(k):
        w = rng.integers(0, table_rows, k, dtype=np.int64) | (rng.integers(0, 2, k, dtype=np.int64) << 31)
        if shared:
            w |= rng.integers(0, nwin, k, dtype=np.int64) << 24
        return w.astype(np.uint32)

    if pool:
        longest = int(counts.max()) if counts.size else 0
        lists = [payload(longest) for _ in range(pool)]
        pick = rng.integers(0, pool, counts.size)
        per_bucket = [lists[p][:k] for p, k in zip(pick.tolist(), counts.tolist())]
    else:
        flat = payload(int(counts.sum()))
        per_bucket = np.split(flat, np.cumsum(counts)[:-1]) if counts.size else []
    return StageSchedule(curve, c, shared, per_bucket)


def from_scalars(curve, c, shared, sc):
    """the schedule of the scalars `sc` (msm_schedule.Scalars): ms.Schedule's entries bucket by bucket"""
    nwin = ms.nwin_of(curve, c)
    s = ms.Schedule(sc.limbs, c, nwin, shared)
    order = np.argsort(s.bucket, kind="stable")
    flat = s.payload[order]
    return StageSchedule(curve, c, shared, np.split(flat, np.cumsum(s.counts.astype(np.int64))[:-1]))


# ------------------------------------------------------------------------------------------------ expected values
class Expected:
    """what every stage holds for `sched` over `table`, chunk length L, list length `entries`: integers mod r"""

    def __init__(self, sched, table, L, entries):
        r = self.r = ms.modulus(sched.curve)
        self.sched, self.L = sched, L
        total, nbk = sched.total, sched.nbuckets
        assert total <= entries and L >= 1
        vals = sched.values(table)
        self.nchunks = max(1, -(-entries // L))
        offs, kept, owner = sched.offsets.astype(np.int64), sched.kept.astype(np.int64), sched.bucket_of
        # the accumulation's pieces
        self.acc = [0] * nbk                                            # buckets[b]: the part of b inside the chunk that holds its first entry
        self.cont = {}                                                  # q -> cont[q], where chunk q starts inside a bucket begun earlier
        self.cont_bucket = np.full(self.nchunks, EMPTY, dtype=np.uint32)
        self.pieces = {}                                                # b -> the chunks that continue it
        for q in range(min(self.nchunks, -(-total // L))):
            pos, end = q * L, min((q + 1) * L, total)
            first = True
            while pos < end:
                b = int(owner[pos])
                stop = min(int(offs[b] + kept[b]), end)
                v = sum(vals[pos:stop]) % r
                if int(offs[b]) == pos:
                    self.acc[b] = v
                else:
                    assert first, "only the leading part of a chunk can continue an earlier bucket"
                    self.cont[q] = v; self.cont_bucket[q] = b
                    self.pieces.setdefault(b, []).append(q)
                first = False
                pos = stop
        # after the merges: all entries of a bucket
        self.merged = [0] * nbk
        csum = np.concatenate([[0], np.cumsum(kept)])
        for b in np.flatnonzero(kept).tolist():
            self.merged[b] = sum(vals[int(csum[b]):int(csum[b + 1])]) % r
        self._sets = [self.merged[w * sched.nb:(w + 1) * sched.nb] for w in range(nbk // sched.nb)]

    def pieces_sum(self, b):
        return (self.acc[b] + sum(self.cont[q] for q in self.pieces.get(b, []))) % self.r

    # ---- partial sums by kind, indexed through the geometry record only
    def window_sums(self):
        """classic: sum w = sum_b (b + 1) B[w][b]"""
        return [sum((b + 1) * v for b, v in enumerate(B) if v) % self.r for B in self._sets]

    def bit_sums(self, c):
        """one shared set: sum k = the buckets whose weight b + 1 has bit k set"""
        B = self._sets[0]
        return [sum(v for b, v in enumerate(B) if v and ((b + 1) >> k) & 1) % self.r for k in range(c)]

    def grid_sums(self, log_l, log_h):
        """(column bit totals, k = 0 .. log_l; row bit totals, k = 0 .. log_h - 1) with b = hi 2^log_l + lo: columns weigh lo + 1, rows weigh hi"""
        B = np.array(self._sets[0], dtype=object).reshape(1 << log_h, 1 << log_l)
        col, row = B.sum(axis=0), B.sum(axis=1)
        cols = [sum(int(v) for lo, v in enumerate(col) if ((lo + 1) >> k) & 1) % self.r for k in range(log_l + 1)]
        rows = [sum(int(v) for hi, v in enumerate(row) if (hi >> k) & 1) % self.r for k in range(log_h)]
        return cols, rows

    def group_sums(self, ngroups):
        """segments of one shared set: group g = sum (b + 1) B_b over its nb / ngroups consecutive buckets"""
        B = self._sets[0]
        per = len(B) // ngroups
        return [sum((b + 1) * B[b] for b in range(g * per, (g + 1) * per)) % self.r for g in range(ngroups)]

    def folded(self):
        """sum_b (b + 1) B_b per bucket set, the sets combined as windows: sum_w 2^(c w) S_w"""
        return sum(s << (self.sched.c * w) for w, s in enumerate(self.window_sums())) % self.r

    # ---- the folds of the other kinds, as DESIGN states them (the host test holds them to `folded`)
    def fold_bits(self, sums):
        return sum(s << k for k, s in enumerate(sums)) % self.r

    def fold_grid(self, cols, rows, log_l):
        return (sum(s << k for k, s in enumerate(cols)) + sum(s << (log_l + k) for k, s in enumerate(rows))) % self.r


def reduction_kind(shared, c):
    """the kind DESIGN §3 gives a bucket set of 2^(c-1) buckets"""
    if not shared:
        return SEGMENTS
    nb = 1 << (c - 1)
    return BITSUM if 128 <= nb <= 1 << 16 else GRID if nb > 1 << 16 else SEGMENTS


# ------------------------------------------------------------------------------------------------ placed boundaries
class Placer:
    """lays buckets down one after the other and keeps the list position, so that a bucket can be put at a chosen place in the chunking"""

    def __init__(self, nbuckets, L):
        self.counts, self.b, self.pos, self.L = np.zeros(nbuckets, dtype=np.int64), 0, 0, L

    def empty(self, k=1):
        self.b += k

    def bucket(self, n):
        assert n >= 1
        self.counts[self.b] = n; self.b += 1; self.pos += n

    def to_chunk_start(self):
        """a bucket that ends exactly at a chunk end: the next one starts exactly at a chunk start"""
        self.bucket(self.L - self.pos % self.L)

    def to_chunk(self, q_mod, modulus=64):
        """short buckets (no continuation run of their own beyond one piece) until the position lies in the last slot of a chunk q with q + 1 = q_mod
        (mod modulus): a bucket placed here has its first continuation piece in a chunk = q_mod"""
        self.to_chunk_start()
        while (self.pos // self.L + 1) % modulus != q_mod % modulus:
            self.bucket(self.L)
        if self.L > 1:
            self.bucket(self.L - 1)

    def run(self, pieces, tail):
        """a bucket with exactly `pieces` continuation pieces whose last piece holds tail + 1 entries (0 <= tail < L)"""
        first = self.pos
        last = (first // self.L + pieces) * self.L + tail
        self.bucket(last - first + 1)


def situations(sched, L, entries):
    """what the chunking of this schedule contains, from counts and offsets alone (the GPU tests assert the situations they were built for)"""
    kept, offs, total = sched.kept.astype(np.int64), sched.offsets.astype(np.int64), sched.total
    full = np.flatnonzero(kept)
    first, last = offs[full], offs[full] + kept[full] - 1
    pieces = last // L - first // L
    gaps = np.diff(full) - 1                                             # empty buckets between two non-empty ones
    inside = (first[1:] % L) != 0                                        # ... whose neighbours' entries meet inside one chunk
    long_ = pieces > 12
    return dict(ends_at_chunk_end=bool(((last + 1) % L == 0).any()), starts_at_chunk_start=bool(((first % L == 0) & (first > 0)).any()),
                empty_runs_inside_a_chunk=set(gaps[inside & (gaps > 0)].tolist()), empty_first=int(full[0]) if full.size else sched.nbuckets,
                empty_last=bool(kept[-1] == 0), total_mod_4=total % 4, trailing_chunks=max(1, -(-entries // L)) - -(-total // L),
                pieces=set(pieces.tolist()), long_run_starts_mod_64=set(((first[long_] // L + 1) % 64).tolist()),
                long_run_ends_at_last_chunk=bool((last[long_] // L == (total - 1) // L).any()) if total else False)
