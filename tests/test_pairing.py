"""The product's pairing layer (csrc/pairing.hpp behind cg_pairing, cg_miller_loop, cg_final_exp, cg_pairing_check on the host and
cg_miller_batch, cg_miller_product on the GPU) against the oracle's optimal-ate pairing, which pins the value convention of arkworks 0.4 and
snarkjs (tests/test_oracle_pinning.py: `vk_alphabeta_12`).  Every comparison is bit for bit."""
import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, G1, G2
from product import cg, ensure_built

CURVES = [BN254, BLS12_381]
DISTINCT = 13          # distinct (P, Q) pairs behind every batch: lane i holds pair i % 13 (13 is coprime to the wave and workgroup sizes)


def limbs(curve):
    return 6 if curve == BLS12_381 else 4


_pairs = {}


def seeded_pairs(curve):
    """13 seeded pairs (a_i G1, b_i G2) and the oracle's pairing of each, computed once per curve"""
    if curve not in _pairs:
        rng = np.random.default_rng(900 + curve)
        ks = orc.random_field(curve, FR, 2 * DISTINCT, rng)
        g1 = np.stack([orc.generator_mul(curve, G1, k) for k in ks[:DISTINCT]])
        g2 = np.stack([orc.generator_mul(curve, G2, k) for k in ks[DISTINCT:]])
        want = np.stack([orc.pairing(curve, p, q) for p, q in zip(g1, g2)])
        _pairs[curve] = (g1, g2, want)
    return _pairs[curve]


def batch_inputs(curve, n, infinities=True):
    """n pairs cycling through the seeded ones, slot 0 with G1 at infinity and slot n - 1 with G2 at infinity, and the expected pairings"""
    g1, g2, want = seeded_pairs(curve)
    idx = np.arange(n) % DISTINCT
    a, b, w = g1[idx].copy(), g2[idx].copy(), want[idx].copy()
    if not infinities:
        return a, b, w
    one = cg.fp12_one(curve)
    a[0] = 0; w[0] = one
    b[n - 1] = 0; w[n - 1] = one
    return a, b, w


@pytest.mark.parametrize("curve", CURVES)
def test_host_pairing_matches_the_oracle(curve):
    """generators, three seeded random multiples, P or Q at infinity (both give one)"""
    ensure_built()
    one_fr = orc.from_dec(curve, FR, 1)
    P, Q = orc.generator_mul(curve, G1, one_fr), orc.generator_mul(curve, G2, one_fr)
    np.testing.assert_array_equal(cg.pairing(curve, P, Q), orc.pairing(curve, P, Q))
    g1, g2, want = seeded_pairs(curve)
    for i in range(3):
        np.testing.assert_array_equal(cg.pairing(curve, g1[i], g2[i]), want[i])
    one = cg.fp12_one(curve)
    assert one[0, 0, 0].any() and not one[0, 0, 1].any() and not one[0, 1:].any() and not one[1].any()
    for p, q in ((np.zeros_like(P), Q), (P, np.zeros_like(Q))):
        np.testing.assert_array_equal(orc.pairing(curve, p, q), one)
        np.testing.assert_array_equal(cg.pairing(curve, p, q), one)
    # the pieces compose: Miller loop then final exponentiation is the pairing, and a Miller product exponentiates to the product
    np.testing.assert_array_equal(cg.final_exp(curve, cg.miller_loop(curve, g1[:1], g2[:1])), want[0])
    np.testing.assert_array_equal(cg.final_exp(curve, cg.miller_loop(curve, g1[:2], g2[:2])), cg.fp12_mul(curve, want[0], want[1]))


@pytest.mark.parametrize("curve", CURVES)
def test_host_pairing_is_bilinear(curve):
    ensure_built()
    rng = np.random.default_rng(77 + curve)
    a = orc.random_field(curve, FR, 1, rng)[0]
    g1, g2, want = seeded_pairs(curve)
    P, Q = g1[3], g2[3]
    aP = orc.points_mul(curve, G1, P[None, :], a[None, :])[0]; aQ = orc.points_mul(curve, G2, Q[None, :], a[None, :])[0]
    left, right = cg.pairing(curve, aP, Q), cg.pairing(curve, P, aQ)
    np.testing.assert_array_equal(left, right)
    assert not np.array_equal(left, cg.fp12_one(curve))
    # e(P, Q) e(-P, Q) == 1, and a product that is not one is refused
    negP = cg.point_to_affine(curve, G1, cg.point_neg(curve, G1, cg.point_from_affine(curve, G1, P)))
    assert cg.pairing_check(curve, np.stack([P, negP]), np.stack([Q, Q]))
    assert not cg.pairing_check(curve, np.stack([P, P]), np.stack([Q, Q]))
    assert cg.pairing_check(curve, np.zeros((0, 2 * limbs(curve)), dtype=np.uint64), np.zeros((0, 4 * limbs(curve)), dtype=np.uint64))


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_miller_batch_then_final_exp_is_the_pairing(ctx, curve, n):
    """lane, wave and workgroup edges; an infinity in G1 at slot 0 and in G2 at slot n - 1"""
    a, b, want = batch_inputs(curve, n)
    vals = ctx.miller_batch(curve, a, b)
    assert vals.shape == (n, 2, 3, 2, limbs(curve))
    done = {}
    for i in range(n):
        key = vals[i].tobytes()
        if key not in done:
            done[key] = cg.final_exp(curve, vals[i])
        np.testing.assert_array_equal(done[key], want[i], err_msg=f"pair {i} of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 65, 257])
@pytest.mark.parametrize("scaled", [False, True])
def test_miller_product_is_the_product_of_the_values(ctx, curve, n, scaled):
    """odd tree sizes and more than one workgroup; with 128-bit scalars the reference pairs are multiplied on the host first"""
    a, b, _ = batch_inputs(curve, n, infinities=not (scaled and n <= 2))     # (at n <= 2 the infinities would leave no lane for the scalars)
    ks = None
    if scaled:
        rng = np.random.default_rng(31 * n + curve)
        ks = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
        ks[n // 2] = (1, 0)
        if n > 2:
            ks[1] = (0, 0); ks[2] = (2**64 - 1, 2**64 - 1)
        ref_a = a.copy()
        for i in range(n):
            k = orc.from_dec(curve, FR, int(ks[i, 0]) + (int(ks[i, 1]) << 64))
            ref_a[i] = cg.point_to_affine(curve, G1, cg.point_scalar_mul(curve, G1, cg.point_from_affine(curve, G1, a[i]), k))
    else:
        ref_a = a
    got = ctx.miller_product(curve, a, b, ks)
    vals = ctx.miller_batch(curve, ref_a, b)
    want = cg.fp12_one(curve)
    for v in vals:
        want = cg.fp12_mul(curve, want, v)
    np.testing.assert_array_equal(got, want)
    if n <= 2:                                   # and against the host loop, which shares no kernel with either
        np.testing.assert_array_equal(got, cg.miller_loop(curve, ref_a, b))
        if scaled:
            assert not np.array_equal(got, cg.fp12_one(curve))
