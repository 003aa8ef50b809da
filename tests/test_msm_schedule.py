"""The MSM's scalar side on the GPU, path by path, against the Python restatement (tests/msm_schedule.py; pinned by test_msm_schedule_host.py).
cg_msm_schedule_dev builds the schedule of one scalar vector with the launchers an MSM call uses and downloads it: counts and offsets must be equal,
every bucket's segment must hold that bucket's entries, and no position behind the last entry may have been written.  Every case asserts the path
that ran, so none can silently take another one.

Distributions (msm_schedule.distribution): uniform | all equal | all zero | boundary (digit_scalars of test_msm_edges.py and 2^c - 1 digits under a
carry, tiled) | hot bucket (digit 2^(c-1) in every window) | staircase (equally full buckets, every region populated) | far regions (digits 1, 2^(c-1)
and -(2^(c-1) - 1): item tiles span far more than their LDS window, with both signs) | near regions (digits <= 2048: with one bucket set every tile stays inside its window)."""
import ctypes as C

import numpy as np
import pytest

import msm_schedule as ms
from oracle_lib import BN254, BLS12_381
from product import cg, ensure_built
from test_msm_edges import digit_scalars

pytestmark = pytest.mark.gpu
CURVE_IDS = {BN254: "bn254", BLS12_381: "bls12_381"}
ALL = ["uniform", "all equal", "all zero", "boundary", "hot bucket", "staircase", "far regions", "near regions"]
GENERAL, SMALL, PARTITION, DIRECT, UNSTAGED = cg.MSM_PATH_GENERAL, cg.MSM_PATH_SMALL, cg.MSM_PATH_PARTITION, cg.MSM_PATH_DIRECT, cg.MSM_PATH_PARTITION_UNSTAGED
PATH_NAMES = {GENERAL: "general", SMALL: "small", PARTITION: "partition, staged", DIRECT: "direct", UNSTAGED: "partition, unstaged"}
THRESHOLD = 1 << 21                      # entries from which an MSM call takes the partition sort (msm_sort_use_partition)


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def scalars(name, curve, c, n):
    nwin = ms.nwin_of(curve, c)
    return ms.distribution(name, curve, c, nwin, n, boundary=digit_scalars(curve, c) + ms.carry_scalars(curve, c, nwin))


def build(ctx, curve, sc, c, shared, path=0, cap=0):
    d = ctx.to_device(sc.mont)
    try:
        return ctx.msm_schedule(curve, d, sc.n, c, shared=shared, path=path, cap=cap)
    finally:
        d.free()


def check(ctx, curve, sc, exp, want_path, path=0, what=""):
    counts, offsets, sorted_, taken, overflow = build(ctx, curve, sc, exp.c, exp.shared, path)
    assert taken == want_path, f"{what}: the {PATH_NAMES.get(taken, taken)} path ran, not the {PATH_NAMES[want_path]} one"
    assert overflow == 0
    ms.check_dense(exp, counts, offsets, sorted_, what)


# ------------------------------------------------------------------------------------------------ one workgroup (k_msm_sort_small)
@pytest.mark.parametrize("n", [1, 1023, 1025, "most"])
@pytest.mark.parametrize("c", [8, 14])
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=CURVE_IDS.values())
def test_small_path(ctx, curve, c, n, lib_option):
    """one shared bucket set of at most 2^13 buckets and 2^15 entries: n around the 1024 lanes, and the most that fits; what does not fit (c = 8,
    n = 1025) must take the general path and refuse the forced small one.  With CG_GOPT_SORT_SMALL = 0 the same inputs take the general path and
    give the same schedule."""
    nwin = ms.nwin_of(curve, c)
    n = (1 << 15) // nwin if n == "most" else n
    fits = n * nwin <= 1 << 15
    for name in ALL:
        sc = scalars(name, curve, c, n)
        exp = ms.Schedule(sc.limbs, c, nwin, 1)
        what = f"{name}, c={c}, n={n}"
        lib_option(cg.GOPT_SORT_SMALL, 1)
        check(ctx, curve, sc, exp, SMALL if fits else GENERAL, what=what)
        if fits:
            check(ctx, curve, sc, exp, SMALL, path=SMALL, what=what + ", forced")
        else:
            with pytest.raises(cg.BackendError):
                build(ctx, curve, sc, c, 1, path=SMALL)
        check(ctx, curve, sc, exp, GENERAL, path=GENERAL, what=what + ", forced general")
        lib_option(cg.GOPT_SORT_SMALL, 0)
        check(ctx, curve, sc, exp, GENERAL, what=what + ", CG_GOPT_SORT_SMALL = 0")


@pytest.mark.parametrize("c", [8, 14])
def test_small_path_ends_at_its_entry_limit(ctx, c):
    curve = BN254
    nwin = ms.nwin_of(curve, c)
    n = (1 << 15) // nwin + 1
    sc = scalars("uniform", curve, c, n)
    check(ctx, curve, sc, ms.Schedule(sc.limbs, c, nwin, 1), GENERAL, what=f"c={c}, n={n}")


# ------------------------------------------------------------------------------------------------ six launches (k_msm_digits, k_scan_*, k_msm_scatter)
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("shared,c", [(0, 2), (0, 3), (0, 13), (0, 16), (0, 19), (0, 20), (1, 15), (1, 22)], ids=lambda v: str(v))
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=CURVE_IDS.values())
def test_general_path(ctx, curve, shared, c, n):
    """classic c = 19 and 20 have 1792 and 3328 scan tiles: k_scan_exclusive with two and four tile sums per lane"""
    nwin = ms.nwin_of(curve, c)
    if not shared and c in (19, 20):
        assert -(-ms.nbuckets_of(c, nwin, 0) // 2048) == {19: 1792, 20: 3328}[c]
    for name in ALL:
        sc = scalars(name, curve, c, n)
        check(ctx, curve, sc, ms.Schedule(sc.limbs, c, nwin, shared), GENERAL, what=f"{name}, c={c}, shared={shared}, n={n}")


# ------------------------------------------------------------------------------------------------ partition sort (k_part_*, k_items_*)
#            shared, c, regions of 512 buckets
WINDOWS = [(1, 13, 8),        # the lower bound
           (0, 13, 160),
           (0, 16, 1024),
           (1, 20, 1024),
           (0, 17, 1920),     # staged with two regions per lane
           (1, 21, 2048),     # exactly STAGE_MAX_REGIONS
           (0, 18, 3840),     # unstaged even with staging on
           (1, 22, 4096)]     # the upper bound
BLS_WINDOWS = [w for w in WINDOWS if w[:2] in ((0, 16), (1, 21), (1, 22))]
PART_CASES = [(BN254,) + w for w in WINDOWS] + [(BLS12_381,) + w for w in BLS_WINDOWS]
PART_IDS = [f"{CURVE_IDS[cv]}-{'shared' if sh else 'classic'}{c}-{r}" for cv, sh, c, r in PART_CASES]


def partition_paths(regions):
    """[(CG_GOPT_SORT_STAGING, the path that must be reported)]"""
    return [(1, PARTITION if regions <= 2048 else UNSTAGED), (0, UNSTAGED)]


@pytest.mark.parametrize("name", ["uniform", "all equal", "all zero", "far regions", "near regions"])
@pytest.mark.parametrize("curve,shared,c,regions", PART_CASES, ids=PART_IDS)
def test_partition_path_at_its_threshold(ctx, curve, shared, c, regions, name, lib_option):
    """what an MSM call selects at the smallest n of 2^21 entries, staged and unstaged"""
    nwin = ms.nwin_of(curve, c)
    assert -(-ms.nbuckets_of(c, nwin, shared) // ms.REGION) == regions
    n = -(-THRESHOLD // nwin)
    sc = scalars(name, curve, c, n)
    exp = ms.Schedule(sc.limbs, c, nwin, shared)
    outside = exp.direct_items()
    print(f"{name}: {exp.total} entries, {outside} outside their item tile's window")
    if name == "far regions":
        assert outside > 0
    if name == "near regions" and shared:
        assert outside == 0
    for staging, want in partition_paths(regions):
        lib_option(cg.GOPT_SORT_STAGING, staging)
        check(ctx, curve, sc, exp, want, what=f"{name}, c={c}, shared={shared}, n={n}, staging={staging}")


def n_just_over_an_item_tile(curve, c, nwin):
    """the first n at which the uniform scalars have ITEM_TILE + 64 non-zero digits (the narrow top window of some c is often zero)"""
    digs, _ = ms.signed_digits(ms.uniform_pool(curve).limbs[:4096], c, nwin)
    return int(np.searchsorted(np.cumsum((digs != 0).sum(axis=0)), ms.ITEM_TILE + 64)) + 1


@pytest.mark.parametrize("shape", ["one", "tile", "tile+1", "item tile"])
@pytest.mark.parametrize("curve,shared,c,regions", PART_CASES, ids=PART_IDS)
def test_partition_path_forced_at_small_shapes(ctx, curve, shared, c, regions, shape, lib_option):
    """the partition kernels below their threshold: one scalar; at most one PART_TILE of entries (exactly one where the window count divides it:
    16 windows, n = 1024) and the first n above it; just over one ITEM_TILE of non-zero items"""
    nwin = ms.nwin_of(curve, c)
    n = {"one": 1, "tile": ms.PART_TILE // nwin, "tile+1": ms.PART_TILE // nwin + 1, "item tile": n_just_over_an_item_tile(curve, c, nwin)}[shape]
    if nwin == 16 and shape == "tile":
        assert n * nwin == ms.PART_TILE
    for name in ALL:
        sc = scalars(name, curve, c, n)
        exp = ms.Schedule(sc.limbs, c, nwin, shared)
        if shape == "item tile" and name == "uniform":
            assert ms.ITEM_TILE + 64 <= exp.total < ms.ITEM_TILE + 64 + nwin
        for staging, want in partition_paths(regions):
            lib_option(cg.GOPT_SORT_STAGING, staging)
            check(ctx, curve, sc, exp, want, path=PARTITION, what=f"{name}, c={c}, shared={shared}, n={n}, staging={staging}")


def test_partition_needs_eight_regions(ctx):
    """shared c = 12 has four regions: an MSM call of 2^21 entries takes the general path (a forced partition is refused: test_refusals)"""
    curve, c = BN254, 12
    nwin = ms.nwin_of(curve, c)
    sc = scalars("uniform", curve, c, -(-THRESHOLD // nwin))
    check(ctx, curve, sc, ms.Schedule(sc.limbs, c, nwin, 1), GENERAL, what="shared c=12")


# ------------------------------------------------------------------------------------------------ one-pass scatter (k_msm_scatter_direct)
def check_direct(ctx, curve, sc, c, shared, cap, want_overflow, what):
    nwin = ms.nwin_of(curve, c)
    exp = ms.Schedule(sc.limbs, c, nwin, shared)
    counts, offsets, sorted_, taken, overflow = build(ctx, curve, sc, c, shared, path=DIRECT, cap=cap)
    assert taken == DIRECT
    assert bool((exp.counts > cap).any()) == want_overflow, f"{what}: the inputs do not {'overflow' if want_overflow else 'fit'} cap = {cap}"
    ms.check_direct(exp, cap, counts, offsets, sorted_, overflow, what)
    return exp


@pytest.mark.parametrize("shared,c", [(0, 8), (1, 13)], ids=["classic8", "shared13"])
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=CURVE_IDS.values())
def test_direct_path(ctx, curve, shared, c):
    n = 5000
    nwin = ms.nwin_of(curve, c)
    uni = scalars("uniform", curve, c, n)
    fullest = int(ms.Schedule(uni.limbs, c, nwin, shared).counts.max())
    check_direct(ctx, curve, uni, c, shared, fullest, False, "uniform, cap = the fullest bucket")          # some bucket holds exactly cap entries
    check_direct(ctx, curve, uni, c, shared, fullest - 1, True, "uniform, cap = the fullest bucket - 1")
    check_direct(ctx, curve, scalars("all equal", curve, c, n), c, shared, 16, True, "all equal, cap = 16")
    # exactly cap entries in bucket (window 3, digit 5) and cap - 1 / cap + 1 in bucket (window 0, digit 9); every other scalar zero
    cap = 40
    for extra, over in ((cap - 1, False), (cap + 1, True)):
        index = np.array([0] * cap + [1] * extra + [2] * (n - cap - extra))
        sc = ms.Scalars(curve, [5 << (3 * c), 9, 0], np.random.default_rng(extra).permutation(index))
        exp = check_direct(ctx, curve, sc, c, shared, cap, over, f"{cap} and {extra} entries under cap = {cap}")
        assert sorted(int(v) for v in exp.counts[exp.counts > 0]) == sorted([cap, extra])
    check_direct(ctx, curve, uni, c, shared, 1, True, "uniform, cap = 1")
    once = ms.Scalars(curve, [j + 1 for j in range(100)] + [0], np.minimum(np.arange(n), 100))
    check_direct(ctx, curve, once, c, shared, 1, False, "a hundred buckets of one entry, cap = 1")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    """null pointers, c = 1 and 23, n = 0, and forced paths outside their structural limits: an error, and the host buffers as they were"""
    curve, n = BN254, 4
    lib = cg.load()
    sc = scalars("uniform", curve, 8, n)
    d = ctx.to_device(sc.mont)
    size = 1 << 16
    bufs = [np.full(size, 0xA5A5A5A5, dtype=np.uint32) for _ in range(3)]
    taken, overflow = C.c_int32(-7), C.c_uint32(77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(h=ctx.h, scal=d.ptr, n=n, c=8, shared=0, path=0, cap=0, out=(0, 1, 2), t=True, o=True):
        args = [ptr(bufs[k]) if k in out else None for k in range(3)]
        return lib.cg_msm_schedule_dev(h, curve, C.c_void_p(scal), C.c_size_t(n), c, shared, path, C.c_uint32(cap), *args, C.byref(taken) if t else None, C.byref(overflow) if o else None)

    refused = [("no context", dict(h=None)), ("no scalars", dict(scal=None)), ("no counts", dict(out=(1, 2))), ("no offsets", dict(out=(0, 2))), ("no sorted", dict(out=(0, 1))),
               ("no path_taken", dict(t=False)), ("no overflow", dict(o=False)), ("c = 1", dict(c=1)), ("c = 23", dict(c=23)), ("n = 0", dict(n=0)),
               ("path 5", dict(path=5)), ("path -1", dict(path=-1)), ("shared 2", dict(shared=2)),
               ("small with 2^14 buckets", dict(c=15, shared=1, path=SMALL)), ("small without a shared set", dict(c=8, shared=0, path=SMALL)),
               ("partition with 4 regions", dict(c=12, shared=1, path=PARTITION)), ("partition with 7168 regions", dict(c=19, shared=0, path=PARTITION)),
               ("partition with 13312 regions", dict(c=20, shared=0, path=PARTITION)), ("direct without a capacity", dict(path=DIRECT, cap=0))]
    try:
        for what, kw in refused:
            assert call(**kw) != 0, f"{what}: accepted"
            assert lib.cg_last_error(), what
            assert all((b == 0xA5A5A5A5).all() for b in bufs) and taken.value == -7 and overflow.value == 77, f"{what}: refused, but the outputs were written"
        # (no power-of-two window count gives exactly 8192 regions; 7168 = classic c = 19 is the first count above 4096)
        assert call(c=8, shared=1, path=SMALL) == 0 and taken.value == SMALL and overflow.value == 0           # the same buffers, accepted
        assert not (bufs[0][:128] == 0xA5A5A5A5).any() and (bufs[0][128:] == 0xA5A5A5A5).all()
    finally:
        d.free()
