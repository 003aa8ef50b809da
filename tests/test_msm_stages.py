"""The MSM's point side on the GPU, stage by stage, against the Python restatement (tests/msm_stages.py; pinned by test_msm_stages_host.py).
cg_msm_stages_dev runs the launchers an MSM call uses (msm_accumulate_batch, msm_reduce_batch) over hand-built schedules and an explicit chunk length
and downloads (a) every bucket, continuation piece and tag after the accumulation, (b) every bucket after the three merge kernels, (c) the partial
sums the reduction hands the host and (d) the host's fold.  Every comparison is exact, on affine limbs, over everything that was requested; every
case asserts the reduction kind and the chunk count the geometry record reports, so none can silently take another path.

Tables have 256 rows k_j G: `random` (k_j random) and `degenerate` (k_j = 1, 1, r - 1, 2, 0 repeated: equal, opposite and infinite operands at every
stage).  Schedules built from n scalars index row i mod 256."""
import functools

import numpy as np
import pytest

import msm_schedule as ms
import msm_stages as st
import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, G1, G2
from product import cg, ensure_built

pytestmark = pytest.mark.gpu
GROUPS = [(BN254, G1), (BN254, G2), (BLS12_381, G1), (BLS12_381, G2)]
IDS = ["bn254-g1", "bn254-g2", "bls12_381-g1", "bls12_381-g2"]
G1S, G2S = ([g for g in GROUPS if g[1] == G1], IDS[0::2]), ([g for g in GROUPS if g[1] == G2], IDS[1::2])
ROWS = 256
ALL = ("acc", "merged", "partials", "folded")


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    for b in _bases.values():
        b.release()
    _bases.clear()
    c.close()


_tables, _bases = {}, {}


def table_of(curve, group, kind):
    key = (curve, group, kind)
    if key not in _tables:
        _tables[key] = {"random": lambda: st.random_table(curve, group, ROWS), "degenerate": lambda: st.degenerate_table(curve, group, ROWS),
                        "quarter infinity": lambda: st.random_table(curve, group, ROWS, infinity_every=4),
                        "filled": lambda: st.Table(curve, group, [k or 12345 + j for j, k in enumerate(st.random_table(curve, group, ROWS, infinity_every=4).ks)])}[kind]()
    return _tables[key]


def bases_of(ctx, curve, group, kind, pre_c=0):
    """the registered table (precomputed with window pre_c: one shared bucket set), once per module"""
    key = (curve, group, kind, pre_c)
    if key not in _bases:
        b = ctx.register_bases(curve, group, table_of(curve, group, kind).points())
        if pre_c:
            ctx.precompute_bases(b, pre_c)
        _bases[key] = b
    return _bases[key]


def wrap_rows(sched):
    """a schedule built from more scalars than the table has rows: entry i -> row i mod 256"""
    per = [(e & np.uint32(0xFF000000)) | ((e & np.uint32(0xFFFFFF)) % np.uint32(ROWS)) for e in sched.per_bucket]
    return st.StageSchedule(sched.curve, sched.c, sched.shared, per, sched.cap)


def same(got, want, what, unit):
    bad = (got != want).any(axis=-1) if got.ndim > 1 else got != want
    assert not bad.any(), f"{what}: {unit} {int(np.flatnonzero(bad)[0])} differs ({int(bad.sum())} of {bad.size})"
    np.testing.assert_array_equal(got, want, err_msg=what)


def affine(curve, group, jac):
    return np.stack([cg.point_to_affine(curve, group, p) for p in jac])


def add_all(curve, group, pts):
    acc = np.zeros_like(pts[0])
    for p in pts:
        acc = orc.point_add(curve, group, acc, p)
    return acc


def check(ctx, bases, table, scheds, L, entries, kind, cap=0, want=ALL, what=""):
    """one call over `scheds` (one per set), every requested stage of every set against the restatement; returns the result and the expectations"""
    curve, group, c = table.curve, table.group, scheds[0].c
    res = ctx.msm_stages(bases, c, entries, L, [s.arrays() for s in scheds], cap=cap, want=want)
    g = res.geom
    what = f"{what} c={c} L={L} cap={cap}"
    assert g.kind == kind, f"{what}: the {st.KINDS[g.kind]} reduction ran, not {st.KINDS[kind]}"
    assert g.nchunks == max(1, -(-entries // L)) and g.chunk_len == L and g.nb == 1 << (c - 1) and g.nsets == (1 if scheds[0].shared else scheds[0].nwin), f"{what}: {g}"
    exps = []
    for s, sched in enumerate(scheds):
        exp = st.Expected(sched, table, L, entries)
        exps.append(exp)
        tag = f"{what} set {s}"
        pts = lambda values: st.points_of(curve, group, values)
        if "acc" in want:
            same(res.acc_buckets[s], pts(exp.acc), f"{tag}, after k_msm_accumulate{'' if cap else '_pf'}", "bucket")
            same(res.cont_bucket[s], exp.cont_bucket, f"{tag}, tags after the accumulation", "chunk")
            tagged = exp.cont_bucket != st.EMPTY
            want_cont = np.full_like(res.acc_cont[s], 0xFFFFFFFFFFFFFFFF)
            want_cont[tagged] = pts([exp.cont[q] for q in np.flatnonzero(tagged).tolist()])
            want_state = np.where(tagged, (~want_cont.any(axis=1)).astype(np.uint32), np.uint32(st.UNTOUCHED)).astype(np.uint32)
            same(res.cont_state[s], want_state, f"{tag}, state of the continuation pieces (0 point, 1 infinity, 2 not written)", "chunk")
            same(res.acc_cont[s], want_cont, f"{tag}, continuation pieces after the accumulation", "chunk")
        if "merged" in want:
            same(res.merged_buckets[s], pts(exp.merged), f"{tag}, after the merges (k_msm_merge_direct / _cont_l1 / _cont)", "bucket")
        if "partials" in want:
            got = affine(curve, group, res.partials[s])
            if kind == st.SEGMENTS and not sched.shared:
                same(got, pts(exp.window_sums()), f"{tag}, window sums (k_msm_reduce_segments seg_len={g.seg_len} / k_msm_window_sum)", "window")
            elif kind == st.SEGMENTS:
                same(got, pts(exp.group_sums(g.ngroups)), f"{tag}, group sums (k_msm_reduce_segments / k_msm_window_sum)", "group")
            elif kind == st.BITSUM:
                assert g.ngroups == c
                same(got, pts(exp.bit_sums(c)), f"{tag}, bit sums (k_msm_bitsum_partial bit_groups={g.bit_groups} / k_msm_bitsum_final)", "bit")
            else:
                assert g.ngroups == (g.log_l + 1) * g.gc + g.log_h * g.gr and g.log_l + g.log_h == c - 1
                cols, rows = exp.grid_sums(g.log_l, g.log_h)
                got_cols = np.stack([add_all(curve, group, got[k * g.gc:(k + 1) * g.gc]) for k in range(g.log_l + 1)])
                at = (g.log_l + 1) * g.gc
                got_rows = np.stack([add_all(curve, group, got[at + k * g.gr:at + (k + 1) * g.gr]) for k in range(g.log_h)])
                same(got_cols, pts(cols), f"{tag}, column bit sums (k_msm_grid_partial / k_msm_grid_bitsum, gc={g.gc})", "column bit")
                same(got_rows, pts(rows), f"{tag}, row bit sums (k_msm_grid_partial / k_msm_grid_bitsum, gr={g.gr})", "row bit")
        if "folded" in want:
            same(affine(curve, group, res.folded[s:s + 1]), pts([exp.folded()]), f"{tag}, the host's fold ({st.KINDS[kind]})", "result")
    return res, exps


# ------------------------------------------------------------------------------------------------ A. chunk phase and length
@functools.lru_cache(maxsize=None)
def scalar_schedule(curve, c, name, n):
    return wrap_rows(st.from_scalars(curve, c, 0, ms.distribution(name, curve, c, ms.nwin_of(curve, c), n)))


@pytest.mark.parametrize("L", [1, 3, 4, 5, 8, 16, 139, 192])
@pytest.mark.parametrize("name", ["uniform", "hot bucket", "staircase", "all equal", "all zero"])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_chunk_phase_and_length(ctx, curve, group, name, L):
    """classic c = 8, 300 scalars, chunk lengths that put a chunk's first entry at each of the four phases of the index quads (1, 3, 5, 139), multiples
    of four, and lengths beyond a whole bucket set's entries.  All zero: every chunk lies behind the list, everything is infinity."""
    c, n = 8, 300
    sched = scalar_schedule(curve, c, name, n)
    assert (sched.total == 0) == (name == "all zero")
    check(ctx, bases_of(ctx, curve, group, "random"), table_of(curve, group, "random"), [sched], L, sched.nwin * n, st.SEGMENTS, what=name)


# ------------------------------------------------------------------------------------------------ B. placed boundaries
def placed(curve, L, variant):
    """bucket sizes for classic c = 8 with every situation of the list in the module's issue: see the assertions of test_placed_boundaries"""
    nbk = ms.nbuckets_of(8, ms.nwin_of(curve, 8), 0)
    p = st.Placer(nbk, L)
    p.empty(3)                                                          # empty first buckets
    p.bucket(2); p.to_chunk_start()
    p.bucket(1); p.empty(2); p.bucket(1); p.empty(5); p.bucket(2)      # runs of 2 and 5 empty buckets inside one chunk (L >= 5)
    p.to_chunk_start()
    for k, pieces in enumerate((1, 2, 11, 12, 13, 14, 63, 64, 65, 128, 129, 200)):
        p.bucket(1 + k % 3)
        p.run(pieces, tail=(k * 3) % L)
    p.to_chunk(0); p.run(65, tail=L - 1)                                # long runs whose first piece is chunk 0, 1 and 63 mod 64; this one ends at a chunk end
    p.to_chunk(1); p.run(129, tail=0)
    p.to_chunk(63); p.run(13, tail=1 % L)
    p.to_chunk(0); p.run(64, tail=0)
    p.to_chunk(63); p.run(200, tail=2 % L)
    p.bucket(3)
    p.to_chunk(1)
    if variant == 0:
        p.empty(nbk - 1 - p.b)                                          # the last bucket of the last set holds the final long run
    want_mod = variant + 1                                              # total = 1, 2, 3 mod 4
    tail = next(t for t in range(L) if ((p.pos // L + 70) * L + t + 1) % 4 == want_mod) if L >= 4 else 0
    p.run(70, tail=tail)                                                # a long run that ends in the list's last chunk
    assert p.b <= nbk and (variant != 0 or p.b == nbk)
    return p.counts


@pytest.mark.parametrize("kind", ["random", "degenerate"])
@pytest.mark.parametrize("L", [8, 5])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_placed_boundaries(ctx, curve, group, L, kind):
    c = 8
    seen = dict(pieces=set(), starts=set(), mods=set(), empty_last=set())
    for variant in range(3):
        sched = st.from_counts(curve, c, 0, placed(curve, L, variant), ROWS, np.random.default_rng(100 * L + variant))
        entries = sched.total + 3 * L + 1                               # trailing chunks behind the list
        s = st.situations(sched, L, entries)
        assert s["ends_at_chunk_end"] and s["starts_at_chunk_start"] and {2, 5} <= s["empty_runs_inside_a_chunk"] and s["empty_first"] == 3, s
        assert s["trailing_chunks"] >= 3 and s["long_run_ends_at_last_chunk"] and {0, 1, 63} <= s["long_run_starts_mod_64"], s
        assert {1, 2, 11, 12, 13, 14, 63, 64, 65, 128, 129, 200} <= s["pieces"], s
        assert s["empty_last"] == (variant != 0), s
        seen["mods"].add(s["total_mod_4"])
        check(ctx, bases_of(ctx, curve, group, kind), table_of(curve, group, kind), [sched], L, entries, st.SEGMENTS, what=f"{kind} table, variant {variant}")
    assert seen["mods"] == {1, 2, 3}, seen


# ------------------------------------------------------------------------------------------------ C. shared bucket set, window field and sign
def dense(curve, c, shared, rng, pool, low=1, high=3):
    nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), shared)
    return st.from_counts(curve, c, shared, rng.integers(low, high, nbk), ROWS, rng, pool=pool)


@pytest.mark.parametrize("c,items,bit_groups", [(8, 1, 1), (11, 1, 2), (12, 8, 1), (17, 8, 16)])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_shared_set_bit_sums(ctx, curve, group, c, items, bit_groups):
    """one bucket set for all windows: entries carry the window (every one of them) and the sign; bit sums with 1 and 8 buckets per lane, one and more
    workgroups per bit"""
    rng = np.random.default_rng(c)
    sched = dense(curve, c, 1, rng, pool=0 if c <= 12 else 512, low=0 if c <= 12 else 1, high=8 if c == 8 else 3)
    wins = (np.concatenate(sched.per_bucket) >> 24) & 0x7F
    assert set(wins.tolist()) == set(range(sched.nwin)) and len(set((np.concatenate(sched.per_bucket) >> 31).tolist())) == 2
    for kind in ("random", "degenerate") if c <= 12 else ("random",):
        res, _ = check(ctx, bases_of(ctx, curve, group, kind, c), table_of(curve, group, kind), [sched], 8, sched.total + 13, st.BITSUM, what=f"shared, {kind} table")
        assert res.geom.bit_groups == bit_groups and (1 if res.geom.nb <= 1024 else 8) == items, res.geom


@pytest.mark.parametrize("curve,group,c", [g + (18,) for g in GROUPS] + [(BN254, G1, 19)], ids=[i + "-c18" for i in IDS] + ["bn254-g1-c19"])
def test_shared_set_grid(ctx, curve, group, c):
    """the grid reduction from its smallest size: every bucket holds one or two entries"""
    rng = np.random.default_rng(c)
    sched = dense(curve, c, 1, rng, pool=512)
    res, _ = check(ctx, bases_of(ctx, curve, group, "random", c), table_of(curve, group, "random"), [sched], 16, sched.total + 5, st.GRID, what="shared")
    assert res.geom.log_l == 10 and res.geom.log_h == c - 11


# ------------------------------------------------------------------------------------------------ D. classic reductions
@pytest.mark.parametrize("c,seg_len", [(2, 1), (3, 1), (12, 1), (13, 2)])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_classic_reductions(ctx, curve, group, c, seg_len):
    rng = np.random.default_rng(40 + c)
    sched = dense(curve, c, 0, rng, pool=0 if c <= 3 else 256)
    for kind in ("random", "degenerate") if c <= 3 else ("random",):
        res, _ = check(ctx, bases_of(ctx, curve, group, kind), table_of(curve, group, kind), [sched], 8, sched.total, st.SEGMENTS, what=f"classic, {kind} table")
        assert res.geom.seg_len == seg_len and res.geom.ngroups == sched.nwin


@pytest.mark.parametrize("curve,group", G1S[0], ids=G1S[1])
def test_classic_reduction_with_long_segments(ctx, curve, group):
    """c = 16: segments of 16 buckets (lo * run in k_msm_reduce_segments); the partial sums and the fold only (half a million buckets)"""
    rng = np.random.default_rng(56)
    sched = dense(curve, 16, 0, rng, pool=64)
    res, _ = check(ctx, bases_of(ctx, curve, group, "random"), table_of(curve, group, "random"), [sched], 16, sched.total, st.SEGMENTS, want=("partials", "folded"), what="classic")
    assert res.geom.seg_len == 16


# ------------------------------------------------------------------------------------------------ E. padded layout
@pytest.mark.parametrize("shared,c", [(0, 8), (1, 13)], ids=["classic8", "shared13"])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_padded_layout(ctx, curve, group, shared, c):
    """cap = 4 with counts below, at and above it: only a bucket's first min(count, cap) slots exist (k_msm_accumulate)"""
    rng = np.random.default_rng(60 + c)
    nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), shared)
    counts = np.array([0, 1, 3, 4, 5, 40])[rng.integers(0, 6, nbk)]
    counts[-1] = 40
    sched = st.from_counts(curve, c, shared, counts, ROWS, rng).padded(4)
    assert sched.total == int(np.minimum(counts, 4).sum()) < int(counts.sum())
    for kind in ("random", "degenerate"):
        check(ctx, bases_of(ctx, curve, group, kind, c if shared else 0), table_of(curve, group, kind), [sched], 8, sched.total + 9, st.BITSUM if shared else st.SEGMENTS, cap=4,
              what=f"padded, {kind} table")


# ------------------------------------------------------------------------------------------------ F. sets
@pytest.mark.parametrize("cap", [0, 4], ids=["compact", "padded"])
@pytest.mark.parametrize("nsets", [2, 8])
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_sets(ctx, curve, group, nsets, cap):
    """blockIdx.y: different schedules of one geometry side by side, every set compared"""
    c = 8
    nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), 0)
    scheds = []
    for s in range(nsets):
        rng = np.random.default_rng(700 + s)
        counts = rng.integers(0, 7, nbk) * (rng.integers(0, 4, nbk) == 0)         # three buckets in four empty: few distinct points to expect per set
        counts[rng.integers(0, nbk)] = 200 + 31 * s                     # a long run somewhere else in every set
        sched = st.from_counts(curve, c, 0, counts, ROWS, rng)
        scheds.append(sched.padded(cap) if cap else sched)
    assert len({s.counts.tobytes() for s in scheds}) == nsets and len({s.sorted[:64].tobytes() for s in scheds}) == nsets   # no two sets alike
    check(ctx, bases_of(ctx, curve, group, "random"), table_of(curve, group, "random"), scheds, 8, max(s.total for s in scheds) + 1, st.SEGMENTS, cap=cap, what=f"{nsets} sets")


# ------------------------------------------------------------------------------------------------ G. slices
@pytest.mark.parametrize("curve,group", G2S[0], ids=G2S[1])
def test_g2_slices(curve, group):
    """CG_OPT_MSM_G2_SLICES: one entry per lane over one slice of workgroups and 1000 chunks more, so that the accumulation is two launches and the
    second one's first_chunk is not zero"""
    ensure_built()
    c, L = 8, 1
    own = cg.Context(0)
    try:
        own.set_option(cg.OPT_MSM_G2_SLICES, 1)
        table = table_of(curve, group, "random")
        bases = own.register_bases(curve, group, table.points())
        nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), 0)
        rng = np.random.default_rng(80)
        tiny = st.from_counts(curve, c, 0, (np.arange(nbk) < 3).astype(np.int64), ROWS, rng)
        slice_groups = own.msm_stages(bases, c, 3, 1, [tiny.arrays()], want=("folded",)).geom.slice_groups
        assert slice_groups >= 256
        entries = slice_groups * 128 + 1000                             # 128 lanes per G2 workgroup
        sched = st.from_counts(curve, c, 0, rng.multinomial(entries - 7, np.full(nbk, 1.0 / nbk)), ROWS, rng)
        check(own, bases, table, [sched], L, entries, st.SEGMENTS, what="sliced")
        bases.release()
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------ H. infinity rows
@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_infinity_rows(ctx, curve, group):
    """a quarter of the rows at infinity (the registration census then keeps the per-point test in the kernel): their entries add nothing, which is
    the same schedule without them over a table that has points there"""
    c, L = 8, 8
    rng = np.random.default_rng(90)
    nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), 0)
    holes, filled = table_of(curve, group, "quarter infinity"), table_of(curve, group, "filled")
    assert sum(k == 0 for k in holes.ks) == ROWS // 4 and not filled.has_infinity()
    sched = st.from_counts(curve, c, 0, rng.integers(0, 6, nbk), ROWS, rng)
    dropped = st.StageSchedule(curve, c, 0, [e[np.array([holes.ks[int(i) & 0xFFFFFF] != 0 for i in e], dtype=bool)] for e in sched.per_bucket])
    assert dropped.total < sched.total
    a, ea = check(ctx, bases_of(ctx, curve, group, "quarter infinity"), holes, [sched], L, sched.total, st.SEGMENTS, what="rows at infinity")
    b, eb = check(ctx, bases_of(ctx, curve, group, "filled"), filled, [dropped], L, sched.total, st.SEGMENTS, what="their entries dropped")
    assert ea[0].merged == eb[0].merged
    same(a.merged_buckets[0], b.merged_buckets[0], "merged buckets, rows at infinity against their entries dropped", "bucket")
    same(affine(curve, group, a.partials[0]), affine(curve, group, b.partials[0]), "window sums, rows at infinity against their entries dropped", "window")
    same(affine(curve, group, a.folded), affine(curve, group, b.folded), "fold, rows at infinity against their entries dropped", "result")


# ------------------------------------------------------------------------------------------------ I. refusals
def test_refusals(ctx):
    """a schedule broken in one way at a time is refused with its message before anything is launched; the output arrays stay as they were and the
    next valid call on the same context is right"""
    curve, group, c, L = BN254, G1, 8, 8
    nwin = ms.nwin_of(curve, c)
    rng = np.random.default_rng(99)
    table = table_of(curve, group, "random")

    def broken(shared, how):
        sched = st.from_counts(curve, c, shared, rng.integers(0, 4, ms.nbuckets_of(c, nwin, shared)), ROWS, rng)
        counts, offsets, sorted_ = [a.copy() for a in sched.arrays()]
        entries = sched.total
        if how == "count":
            counts[5] += 1
        elif how == "index":
            sorted_[7] = (sorted_[7] & np.uint32(0xFF000000)) | np.uint32(ROWS)
        elif how == "window":
            sorted_[7] = (sorted_[7] & np.uint32(0x80FFFFFF)) | np.uint32(nwin << 24)
        elif how == "total":
            entries -= 1
        return sched, (counts, offsets, sorted_), entries

    cases = [(0, "count", "exclusive scan"), (0, "index", "point index outside the table"), (1, "index", "point index outside the table"),
             (1, "window", "window field outside"), (0, "total", "more than `entries`")]
    for shared, how, message in cases:
        sched, arrays, entries = broken(shared, how)
        bases = bases_of(ctx, curve, group, "random", c if shared else 0)
        nbk, nchunks, aw, jw = sched.nbuckets, -(-entries // L), orc.point_words(curve, group), orc.point_words(curve, group) // 2 * 3
        out = dict(acc_buckets=np.empty((1, nbk, aw), dtype=np.uint64), acc_cont=np.empty((1, nchunks, aw), dtype=np.uint64), cont_state=np.empty((1, nchunks), dtype=np.uint32),
                   cont_bucket=np.empty((1, nchunks), dtype=np.uint32), merged_buckets=np.empty((1, nbk, aw), dtype=np.uint64),
                   partials=np.empty(cg.MSM_MAX_PARTIALS * jw, dtype=np.uint64), folded=np.empty((1, jw), dtype=np.uint64))
        for a in out.values():
            a.view(np.uint8)[...] = 0xA5
        with pytest.raises(cg.BackendError, match=message):
            ctx.msm_stages(bases, c, entries, L, [arrays], out=out)
        assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), f"{how}: refused, but the outputs were written"
        check(ctx, bases, table, [sched], L, sched.total, st.BITSUM if shared else st.SEGMENTS, what=f"after the refusal of a bad {how}")
    sched, arrays, entries = broken(0, "none")
    bases = bases_of(ctx, curve, group, "random")
    for kw, message in ((dict(c=21), "window size out of range"), (dict(L=0), "chunk length"), (dict(nsets=9), "1 .. 8 sets")):
        with pytest.raises(cg.BackendError, match=message):
            ctx.msm_stages(bases, kw.get("c", c), entries, kw.get("L", L), [arrays] * kw.get("nsets", 1), want=("folded",))
    with pytest.raises(cg.BackendError, match="window size out of range"):
        ctx.msm_stages(bases_of(ctx, curve, group, "random", 8), 9, entries, L, [arrays], want=("folded",))
