"""The two batch kernels of the pairing layer that the verifiers only reach on their happy path, at their edges and against the integer
tower of tests/pairing_tower.py (pinned to the oracle by tests/test_pairing_pieces_host.py):
  k_final_exp_check (Context.final_exp_check_batch): group sizes 1, 2, 3, 5 over lane counts 1 .. 130, equal products reached in different
      orders, near misses of one bit in every coordinate of the target, the zero element, refusals;
  k_fp12_product (Context.miller_product) beyond its grid cap, where a lane strides over more than one value.
Every expected flag and value is computed in the tower.  All points are subgroup points: nothing outside the kernels' contract goes to the GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, G1
from pairing_tower import tower
from product import cg, ensure_built
from test_pairing import DISTINCT, batch_inputs, limbs, seeded_pairs

CURVES = [BN254, BLS12_381]
# csrc/pairing.hpp: PAIRING_PRODUCT_GROUPS_MAX = 256 workgroups of PAIRING_BLOCK = 64 lanes; a lane of k_fp12_product strides only beyond
GRID_CAP = 256 * 64
assert GRID_CAP == 16384


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


_pools = {}


def pool(ctx, curve):
    """13 values with a known final exponentiation, once per module: 7 Miller values of seeded pairs (exponentiation: the oracle's pairing)
    and 6 arbitrary elements (exponentiation: the tower's plain power).  -> (values in the ABI layout, exponentiations as tower elements)"""
    if curve not in _pools:
        T = tower(curve)
        g1, g2, want = seeded_pairs(curve)
        vals = [v for v in ctx.miller_batch(curve, g1[:7], g2[:7])]
        refs = [T.from_abi(w) for w in want[:7]]
        sp = T.special_elements()
        for name in ("one", "minus_one", "fp6", "all_pm1", "line", "dense"):
            vals.append(T.to_abi(sp[name])); refs.append(T.final_exp(sp[name]))
        assert refs[7] == T.one and refs[9] == T.one and len(vals) == 13
        _pools[curve] = (np.stack(vals), refs)
    return _pools[curve]


MULTISET = [0, 12, 1, 9, 10]            # the pool values a good group holds (its first k): Miller values and arbitrary elements mixed


def groups_of(curve, refs, k, n):
    """n groups of k pool indices: rotations of one multiset, every third group with one factor swapped for another pool value; and the
    tower's product of each group's exponentiations"""
    T = tower(curve)
    base = MULTISET[:k]
    idx, prods = [], []
    for g in range(n):
        grp = [base[(g + t) % k] for t in range(k)]
        if g % 3 == 2:
            grp[g % k] = (5 * g + 3) % 13
        e = T.one
        for i in grp:
            e = T.mul(e, refs[i])
        idx.append(grp); prods.append(e)
    return np.array(idx), prods


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_final_exp_check_flags_match_the_tower(ctx, curve, k, n):
    """lane, wave and workgroup edges times group sizes; the target is the good multiset's exponentiation (not one)"""
    T = tower(curve)
    vals, refs = pool(ctx, curve)
    idx, prods = groups_of(curve, refs, k, n)
    target = prods[0]
    assert target != T.one and target != T.zero
    want = np.array([e == target for e in prods])
    got = ctx.final_exp_check_batch(curve, vals[idx.reshape(-1)], k, T.to_abi(target))
    assert got.shape == (n,)
    np.testing.assert_array_equal(got, want)
    assert want[0] and (n < 3 or not want.all())


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_final_exp_check_against_one(ctx, curve):
    """groups that multiply to one: Miller(P, Q) Miller(-P, Q), in both orders; every third group has one factor swapped"""
    T = tower(curve)
    g1, g2, want = seeded_pairs(curve)
    neg = np.stack([cg.point_to_affine(curve, G1, cg.point_neg(curve, G1, cg.point_from_affine(curve, G1, p))) for p in g1[:4]])
    vals = ctx.miller_batch(curve, np.concatenate([g1[:4], neg]), np.concatenate([g2[:4], g2[:4]]))       # 0..3: e_i, 4..7: 1 / e_i
    refs = [T.from_abi(w) for w in want[:4]]
    refs += [T.conj(r) for r in refs]                            # the inverse of a pairing value is its conjugate
    for i in range(4):
        assert T.mul(refs[i], refs[4 + i]) == T.one
    n = 65
    idx = np.array([[g % 4, 4 + g % 4][:: 1 if g % 2 == 0 else -1] for g in range(n)])
    for g in range(2, n, 3):
        idx[g, g % 2] = (g + 1) % 8
    flags = np.array([T.mul(refs[i], refs[j]) == T.one for i, j in idx])
    assert flags.any() and not flags.all()
    np.testing.assert_array_equal(ctx.final_exp_check_batch(curve, vals[idx.reshape(-1)], 2, T.to_abi(T.one)), flags)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coefficient", range(6))
def test_final_exp_check_refuses_near_misses(ctx, curve, coefficient):
    """a target with one bit flipped in the lowest or in the highest word of any one of the twelve coordinates gives 0; the true one gives 1.
    One case per Fp2 coefficient of the ABI's layout (its two coordinates, four targets): a call is one lane's whole final exponentiation."""
    T = tower(curve)
    vals, refs = pool(ctx, curve)
    grp = vals[[0, 12]]
    target = T.to_abi(T.mul(refs[0], refs[12]))
    assert ctx.final_exp_check_batch(curve, grp, 2, target).tolist() == [True]
    nq = limbs(curve)
    for coord in (2 * coefficient, 2 * coefficient + 1):
        for word, bit in ((0, coord % 32), (nq - 1, 32 + (3 * coord) % 29)):
            t = target.copy().reshape(12, nq)
            t[coord, word] ^= np.uint64(1 << bit)
            assert ctx.final_exp_check_batch(curve, grp, 2, t.reshape(target.shape)).tolist() == [False], f"coordinate {coord}, word {word}, bit {bit}"


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_final_exp_check_with_a_zero_factor(ctx, curve):
    """0^e = 0 in the tower: a group that holds the zero element never meets a nonzero target, and meets the all-zero one"""
    T = tower(curve)
    vals, refs = pool(ctx, curve)
    assert T.final_exp(T.zero) == T.zero
    zero = np.zeros_like(vals[0])
    groups = np.stack([vals[0], vals[12], zero, vals[12], vals[0], zero, vals[0], vals[12]])        # k = 2: good, zero first, zero last, good
    target = T.mul(refs[0], refs[12])
    assert ctx.final_exp_check_batch(curve, groups, 2, T.to_abi(target)).tolist() == [True, False, False, True]
    assert ctx.final_exp_check_batch(curve, groups, 2, T.to_abi(T.one)).tolist() == [False] * 4
    assert ctx.final_exp_check_batch(curve, groups, 2, zero).tolist() == [False, True, True, False]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_final_exp_check_refusals(ctx, curve):
    """k = 0 is an error that leaves `ok` alone; n = 0 is no work"""
    vals, _ = pool(ctx, curve)
    lib = cg.load()
    ok = np.full(4, 77, dtype=np.int32)
    v = np.ascontiguousarray(vals[:4])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for k in (0, -1):
        assert lib.cg_final_exp_check_batch(ctx.h, curve, p(v), k, C.c_size_t(4), p(v[0]), p(ok)) != 0
        assert (ok == 77).all()
    assert lib.cg_final_exp_check_batch(ctx.h, curve, p(v), 2, C.c_size_t(0), p(v[0]), p(ok)) == 0
    assert lib.cg_final_exp_check_batch(ctx.h, curve, None, 2, C.c_size_t(0), p(v[0]), None) == 0
    assert (ok == 77).all()
    assert ctx.final_exp_check_batch(curve, vals[:0], 2, vals[0]).shape == (0,)


def strided_product_inputs(curve, n):
    """batch_inputs' pairs (cycling through the 13 seeded ones, infinities at slots 0 and n - 1) and how often each distinct pair counts"""
    a, b, _ = batch_inputs(curve, n)
    counts = np.bincount(np.arange(n) % DISTINCT, minlength=DISTINCT)
    counts[0] -= 1; counts[(n - 1) % DISTINCT] -= 1              # the two infinities give one
    return a, b, counts


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [GRID_CAP + 1, 2 * GRID_CAP + 3])
def test_miller_product_beyond_the_grid_cap(ctx, curve, n):
    """the smallest sizes at which k_fp12_product's lanes stride: one lane once (n = cap + 1); every lane once and three twice (2 cap + 3).
    Expected: prod_j v_j^(count_j) in the tower, from the 13 Miller values of one miller_batch call (pinned to the oracle by test_pairing.py)"""
    T = tower(curve)
    g1, g2, _ = seeded_pairs(curve)
    a, b, counts = strided_product_inputs(curve, n)
    want = T.one
    for v, c in zip(ctx.miller_batch(curve, g1, g2), counts):
        want = T.mul(want, T.pow(T.from_abi(v), int(c)))
    np.testing.assert_array_equal(ctx.miller_product(curve, a, b), T.to_abi(want))


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_miller_product_beyond_the_grid_cap_with_scalars(ctx, curve):
    """128-bit scalars on the first 65 lanes, (1, 0) on the others; the reference pairs of those lanes are multiplied on the host first"""
    T = tower(curve)
    n, scaled = GRID_CAP + 1, 65
    g1, g2, _ = seeded_pairs(curve)
    a, b, _ = strided_product_inputs(curve, n)
    rng = np.random.default_rng(53 + curve)
    ks = np.zeros((n, 2), dtype=np.uint64); ks[:, 0] = 1
    ks[:scaled] = rng.integers(0, 2**64, size=(scaled, 2), dtype=np.uint64)
    ks[1] = (0, 0); ks[2] = (2**64 - 1, 2**64 - 1); ks[3] = (1, 0)
    ref_a = a[:scaled].copy()
    for i in range(scaled):
        k = orc.from_dec(curve, FR, int(ks[i, 0]) + (int(ks[i, 1]) << 64))
        ref_a[i] = cg.point_to_affine(curve, G1, cg.point_scalar_mul(curve, G1, cg.point_from_affine(curve, G1, a[i]), k))
    want = T.one
    for v in ctx.miller_batch(curve, ref_a, b[:scaled]):
        want = T.mul(want, T.from_abi(v))
    counts = np.bincount(np.arange(scaled, n) % DISTINCT, minlength=DISTINCT)
    counts[(n - 1) % DISTINCT] -= 1                              # slot n - 1 holds G2's infinity
    for v, c in zip(ctx.miller_batch(curve, g1, g2), counts):
        want = T.mul(want, T.pow(T.from_abi(v), int(c)))
    np.testing.assert_array_equal(ctx.miller_product(curve, a, b, ks), T.to_abi(want))
