"""Structured MSM inputs on the GPU, exact against the CPU oracle through the C ABI: what random points and random scalars reach with
probability zero.
  A  edge coordinates: tables of curve points whose x limbs sit on the boundary values of unpack_small (tests/msm_edges.py), each alone in a
     bucket, doubled, cancelled, and next to another point — bucket contents that do not depend on the order the sort leaves them in
  B  one point many times: every merge and reduction tree then adds multiples of one point, so equal and opposite operands meet constantly
  C  the digit boundaries of the signed-window decomposition, which is written out in four kernels
The host model of the same arithmetic (tests/test_lazy_bucket_host.py) covers the functions one by one; these cover the kernels around them."""
import os
import re

import numpy as np
import pytest

import bench_check as bc
import msm_edges
import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, G1, G2
from product import cg, ensure_built

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]
GROUPS = msm_edges.GROUPS
GROUP_IDS = ["bn254-g1", "bn254-g2", "bls12_381-g1", "bls12_381-g2"]


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.set_msm_window(0); c.set_scatter_capacity(-1)
    c.close()


def random_points(curve, group, n, rng):
    return np.stack([orc.generator_mul(curve, group, k) for k in orc.random_field(curve, FR, n, rng)])


def affine(curve, group, jac):
    return cg.point_to_affine(curve, group, jac)


# ------------------------------------------------------------------------------------------------ A: edge coordinates
WINDOW = 8
PER_COMPONENT = 18              # edge points per MSM: 7 buckets each out of the 2^(c-1) = 128 of window 0


def edge_rows(edges, others, curve):
    """table rows and, per row, (component, digit, negative digit?) for the seven bucket patterns of every edge point E:
    {E} {E,E} {E,E,E} {E,-E} {E,-E,E} {E,R} {E,-R}.  -X is reached both ways: even edge points through a negative digit (scalar 2^c - d on the
    row X, which also drops X into bucket 1 of window 1), odd ones through a negated table row with the positive digit."""
    neg_e, neg_o = msm_edges.neg_points(curve, edges), msm_edges.neg_points(curve, others)
    rows, plan = [], []
    for i, e in enumerate(edges):
        comp, slot = divmod(i, PER_COMPONENT)
        r, nr = others[i % len(others)], neg_o[i % len(others)]
        by_digit = i % 2 == 0
        minus = lambda pos, neg: (pos, True) if by_digit else (neg, False)
        patterns = [[(e, False)], [(e, False)] * 2, [(e, False)] * 3, [(e, False), minus(e, neg_e[i])], [(e, False), minus(e, neg_e[i]), (e, False)],
                    [(e, False), (r, False)], [(e, False), minus(r, nr)]]
        for k, pat in enumerate(patterns):
            for pt, negd in pat:
                rows.append(pt); plan.append((comp, 1 + 7 * slot + k, negd))
    return np.stack(rows), plan


@pytest.mark.parametrize("curve,group", GROUPS, ids=GROUP_IDS)
def test_msm_edge_coordinates(ctx, curve, group):
    """every edge point alone, doubled, tripled, cancelled and beside another point in a bucket of window 0 (fixed window 8, scalars below 2^9),
    plain and with per-window precomputed tables; expected value: the oracle's MSM over the rows with a non-zero scalar"""
    rng = np.random.default_rng(900 + 2 * curve + group)
    edges, _ = msm_edges.edge_points(curve, group)
    for pt in edges:
        assert orc.on_curve(curve, group, pt)
    others = random_points(curve, group, 8, rng)
    table, plan = edge_rows(edges, others, curve)
    ncomp = plan[-1][0] + 1
    values = np.zeros((ncomp, len(plan)), dtype=np.int64)
    for row, (comp, d, negd) in enumerate(plan):
        values[comp, row] = (1 << WINDOW) - d if negd else d
    scalars = [msm_edges.small_scalars(curve, v) for v in values]
    want = []
    for v, sc in zip(values, scalars):
        nz = np.nonzero(v)[0]
        want.append(orc.msm(curve, group, table[nz], sc[nz], threads=8))
    bases = ctx.register_bases(curve, group, table)
    ctx.set_msm_window(WINDOW)
    try:
        for precomputed in (False, True):
            if precomputed:
                ctx.precompute_bases(bases, WINDOW)
            for j in range(0, ncomp, 2):
                got = ctx.msm(bases, scalars[j:j + 2])
                for t in range(got.shape[0]):
                    np.testing.assert_array_equal(affine(curve, group, got[t]), want[j + t], err_msg=f"edge points {PER_COMPONENT * (j + t)}.., precomputed={precomputed}")
    finally:
        ctx.set_msm_window(0)
        bases.release()


# ------------------------------------------------------------------------------------------------ B: one point, many times
def signed_sum(curve, scalars, signs):
    """sum_i sign_i s_i in Fr (sign 0 = the row is infinity), with the oracle's field operations"""
    neg = orc.field_op(curve, FR, "sub", np.zeros_like(scalars), scalars)
    s = np.where(signs[:, None] > 0, scalars, np.where(signs[:, None] < 0, neg, np.zeros_like(scalars)))
    return bc.field_sum(s, curve)


def one_point_table(curve, group, signs, rng):
    p = random_points(curve, group, 1, rng)
    both = np.concatenate([np.zeros_like(p), p, msm_edges.neg_points(curve, p)])       # index 0: infinity, 1: P, 2 (= -1): -P
    return p[0], both[signs]


def check_one_point(ctx, curve, group, p, table, signs, scalars_list, path):
    bases = ctx.register_bases(curve, group, table)
    try:
        if path.startswith("pre"):
            ctx.precompute_bases(bases, int(path[3:]))
        if path.startswith("cap"):
            ctx.set_scatter_capacity(int(path[3:]))
        got = ctx.msm(bases, scalars_list)
        for j, sc in enumerate(scalars_list):
            want = orc.points_mul(curve, group, p[None], signed_sum(curve, sc, signs)[None])[0]
            np.testing.assert_array_equal(affine(curve, group, got[j]), want, err_msg=f"component {j}, {path}")
    finally:
        ctx.set_scatter_capacity(-1)
        bases.release()


@pytest.mark.parametrize("path", ["classic", "pre8", "pre13", "pre18", "cap0", "cap4"])
@pytest.mark.parametrize("curve,group", GROUPS, ids=GROUP_IDS)
def test_msm_one_point_many_times(ctx, curve, group, path):
    """3000 rows, each P, -P or (5 %) infinity; uniform scalars, and all scalars identical (one bucket per window spread over hundreds of
    chunks: equal pieces fold on both merge levels).  classic: per-window bucket sets (k_msm_reduce_segments / k_msm_window_sum); pre8 / pre13:
    k_msm_bitsum_* at 1 and 8 buckets per lane; pre18: k_msm_grid_*.  cap0: the one-pass scatter and the padded k_msm_accumulate, on the uniform
    component alone under the automatic capacity (128 slots per bucket at the automatic window 8, about 23 entries in a bucket and about 47 in
    those of the narrow top window), so that nothing overflows and the padded kernel's own sums are what is compared.  cap4: a capacity both
    components overflow, i.e. the FALLBACK: the optimistic result is discarded and the exact schedule runs.  Expected: P times the signed scalar sum."""
    n = 3000
    rng = np.random.default_rng(1300 + 2 * curve + group)
    signs = rng.choice(np.array([1, -1, 0]), size=n, p=[0.475, 0.475, 0.05])
    p, table = one_point_table(curve, group, signs, rng)
    uniform = orc.random_field(curve, FR, n, rng)
    same = np.tile(orc.random_field(curve, FR, 1, rng), (n, 1))
    check_one_point(ctx, curve, group, p, table, signs, [uniform] if path == "cap0" else [uniform, same], path)


@pytest.mark.parametrize("path", ["classic", "pre13"])
@pytest.mark.parametrize("curve,group", GROUPS, ids=GROUP_IDS)
def test_msm_one_point_pairs_and_equal_signs(ctx, curve, group, path):
    """exact pairs (P, -P) with pairwise equal scalars sum to infinity; a table of 3000 copies of P (all signs equal) only ever doubles"""
    n = 3000
    rng = np.random.default_rng(1400 + 2 * curve + group)
    signs = np.tile(np.array([1, -1]), n // 2)
    p, table = one_point_table(curve, group, signs, rng)
    half = orc.random_field(curve, FR, n // 2, rng)
    paired = np.repeat(half, 2, axis=0)
    same = np.tile(half[:1], (n, 1))
    bases = ctx.register_bases(curve, group, table)
    try:
        if path != "classic": ctx.precompute_bases(bases, 13)
        got = ctx.msm(bases, [paired, same])
        assert not affine(curve, group, got[0]).any() and not affine(curve, group, got[1]).any()
    finally:
        bases.release()
    ones = np.ones(n, dtype=np.int64)
    check_one_point(ctx, curve, group, p, np.tile(p, (n, 1)), ones, [paired, same], path)


# ------------------------------------------------------------------------------------------------ C: digit boundaries
def digit_scalars(curve, c):
    """scalars below r whose every window digit (as far as that stays below r) is 2^(c-1) (the largest digit that stays positive), 2^(c-1) + 1
    (the first that turns negative and carries), 2^(c-1) - 1, 2^c - 1 (a carry rippling through every window into the top one); a single 1 in
    the top window; and r - 1, r - 2, (r - 1) / 2, (r + 1) / 2, 2^floor(log2 r)"""
    r = orc.MODULI[(curve, FR)]
    top = r.bit_length() - 1                               # floor(log2 r)
    nwin = r.bit_length() // c + 1                         # the product's window count (capi_msm.hip)
    out = []
    for v in ((1 << (c - 1)), (1 << (c - 1)) + 1, (1 << (c - 1)) - 1, (1 << c) - 1):
        out.append(sum(v << (c * w) for w in range(nwin)) % (1 << top))
    out.append(1 << min(c * (nwin - 1), top))
    out += [r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, 1 << top]
    assert all(0 < s < r for s in out)
    return out


def tiled(curve, c, n, shift=0):
    vals = digit_scalars(curve, c)
    vals = [vals[(i + shift) % len(vals)] for i in range(n)]
    return msm_edges.scalars_from_ints(curve, vals)


@pytest.mark.parametrize("c", [2, 3, 5, 8, 13, 15, 16])
@pytest.mark.parametrize("curve", CURVES, ids=["bn254", "bls12_381"])
def test_msm_digit_boundaries_classic(ctx, curve, c):
    n = 64
    rng = np.random.default_rng(1500 + 32 * curve + c)
    pts = random_points(curve, G1, n, rng)
    sa, sb = tiled(curve, c, n), tiled(curve, c, n, shift=3)
    bases = ctx.register_bases(curve, G1, pts)
    ctx.set_msm_window(c)
    try:
        got = ctx.msm(bases, [sa, sb])
    finally:
        ctx.set_msm_window(0)
        bases.release()
    for j, sc in enumerate((sa, sb)):
        np.testing.assert_array_equal(affine(curve, G1, got[j]), orc.msm(curve, G1, pts, sc, threads=8), err_msg=f"component {j}")


@pytest.mark.parametrize("c", [8, 13, 17, 18, 20])
@pytest.mark.parametrize("curve", CURVES, ids=["bn254", "bls12_381"])
def test_msm_digit_boundaries_precomputed(ctx, curve, c):
    """per-window precomputed tables: k_msm_digits with one shared bucket set; c = 8 goes through the single-launch sort (k_msm_sort_small)"""
    n = 64
    rng = np.random.default_rng(1600 + 32 * curve + c)
    pts = random_points(curve, G1, n, rng)
    sa, sb = tiled(curve, c, n), tiled(curve, c, n, shift=5)
    bases = ctx.register_bases(curve, G1, pts)
    try:
        ctx.precompute_bases(bases, c)
        got = ctx.msm(bases, [sa, sb])
    finally:
        bases.release()
    for j, sc in enumerate((sa, sb)):
        np.testing.assert_array_equal(affine(curve, G1, got[j]), orc.msm(curve, G1, pts, sc, threads=8), err_msg=f"component {j}")


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("curve", CURVES, ids=["bn254", "bls12_381"])
def test_msm_digit_boundaries_direct_scatter(ctx, curve, cap):
    """k_msm_scatter_direct decomposes the scalars itself: automatic capacity (0), and a capacity of 3 that the tiled scalars overflow, so the
    exact schedule runs after it; classic window 8 and per-window tables with c = 13"""
    n = 64
    rng = np.random.default_rng(1700 + 8 * curve + cap)
    pts = random_points(curve, G1, n, rng)
    ctx.set_scatter_capacity(cap)
    try:
        for c, precomputed in ((8, False), (13, True)):
            sa, sb = tiled(curve, c, n), tiled(curve, c, n, shift=7)
            bases = ctx.register_bases(curve, G1, pts)
            try:
                if precomputed: ctx.precompute_bases(bases, c)
                else: ctx.set_msm_window(c)
                got = ctx.msm(bases, [sa, sb])
            finally:
                ctx.set_msm_window(0)
                bases.release()
            for j, sc in enumerate((sa, sb)):
                np.testing.assert_array_equal(affine(curve, G1, got[j]), orc.msm(curve, G1, pts, sc, threads=8), err_msg=f"component {j}, c={c}")
    finally:
        ctx.set_scatter_capacity(-1)


def partition_threshold_entries():
    """the number of (window, point) entries from which msm_sort_use_partition (csrc/fr_impl.hpp) takes the partition sort"""
    src = open(os.path.join(orc.ROOT, "collaborative-circom_amd", "csrc", "fr_impl.hpp")).read()
    body = src[src.index("inline bool msm_sort_use_partition"):]
    m = re.search(r"nwin \* n >= \(\(size_t\)1 << (\d+)\)", body[:body.index("\n}")])
    assert m, "msm_sort_use_partition no longer has the form this test reads its threshold from"
    return 1 << int(m.group(1))


@pytest.mark.parametrize("staging", [1, 0])
@pytest.mark.parametrize("curve", CURVES, ids=["bn254", "bls12_381"])
def test_msm_digit_boundaries_partition_sort(ctx, curve, staging, lib_option):
    """the partition sort (k_msm_digits_only + k_part_*) at the smallest n it accepts for c = 16, on the synthetic table [(1 + i) G]: exact value
    from one generator multiplication; with and without LDS staging of the scatter"""
    c = 16
    nwin = (orc.MODULI[(curve, FR)].bit_length()) // c + 1
    n = -(-partition_threshold_entries() // nwin)
    lib_option(cg.GOPT_SORT_STAGING, staging)
    rng = np.random.default_rng(1800 + curve)
    sa, sb = tiled(curve, c, n), tiled(curve, c, n, shift=4)
    bases = ctx.synth_bases(curve, G1, 1, n)
    ctx.set_msm_window(c)
    try:
        got = ctx.msm_dev(bases, [ctx.to_device(sa), ctx.to_device(sb)], n)
    finally:
        ctx.set_msm_window(0)
        bases.release()
    for j, sc in enumerate((sa, sb)):
        np.testing.assert_array_equal(affine(curve, G1, got[j]), bc.synth_table_msm(curve, G1, sc, 1), err_msg=f"component {j}")
