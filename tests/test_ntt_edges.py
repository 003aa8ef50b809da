"""The NTT on the inputs its lazy reduction is tightest on, against the oracle's NTT and distribute_powers, exact and over the full vector.

The lazy kernels keep elements unreduced between stages; how far they grow depends on the limbs the kernels see, so the patterns below are set in
those limbs (Montgomery representatives), where p - 1 is the largest value an input can hold.  The transform is linear over them, so the oracle,
given the same limbs, is the reference as it stands.  Sizes: lg 3, 4, 6, 7, 8 (one pass: odd and even stage counts, the radix-2 step behind the
radix-4 ones), lg 11, 14, 16, 17 (two passes, the first of 1, 4, 6 and 7 stages under the default tile of 2^10; 7 + 10 at lg 17 is three radix-4
steps and a radix-2 tail on a strided tile) and lg 18, the smallest three-pass plan, 4 + 4 + 10 stages: the only size here at which the middle
passes run (k_ntt_ct_pass<F, false> with t > 0 and another pass behind it, k_ntt_dit_pass<F, false, false>).  One call transforms 8 vectors (the
most a call takes), each with another pattern, at every size."""
import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR
from product import cg, ensure_built

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 6, 7, 8, 11, 14, 16, 17, 18)
PATTERNS = ("all zero", "all p - 1", "p - 1 at index 0", "p - 1 at index n - 1", "alternating 0 / p - 1", "pure tone", "all >= p - 2^32", "uniform random")


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def limbs(values):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in values), dtype=np.uint64).reshape(-1, 4).copy()


_vectors = {}


def vectors(curve, lg):
    """the eight input vectors of one size, made once and never changed: (list of (n, 4) arrays, omega, its 2n-th root g)"""
    if (curve, lg) not in _vectors:
        n, p = 1 << lg, orc.MODULI[(curve, FR)]
        rng = np.random.default_rng([17, curve, lg])
        _, roots, _ = orc.roots_of_unity(curve)
        pm1 = limbs([p - 1])[0]
        zero = np.zeros((n, 4), dtype=np.uint64)
        full = np.tile(pm1, (n, 1))
        first, last, alt = zero.copy(), zero.copy(), zero.copy()
        first[0] = pm1; last[n - 1] = pm1; alt[1::2] = pm1
        # x_j = (p - 1) w^(-j (n/2 + 1)): the transform puts n (p - 1) into bin n/2 + 1 and zero elsewhere
        w = int(orc.to_dec(curve, FR, roots[lg]))
        step, x, tone = pow(w, n - (n // 2 + 1), p), p - 1, []
        for _ in range(n): tone.append(x); x = x * step % p
        high = limbs([p - 1 - int(r) for r in rng.integers(0, 1 << 32, size=n)])
        vs = [zero, full, first, last, alt, limbs(tone), high, orc.random_field(curve, FR, n, rng)]
        for v in vs: v.setflags(write=False)
        _vectors[(curve, lg)] = (vs, roots[lg], roots[lg + 1])
    return _vectors[(curve, lg)]


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
@pytest.mark.parametrize("lg", SIZES)
def test_ntt_edge_inputs_match_oracle(ctx, curve, lg):
    n = 1 << lg
    vs, w, g = vectors(curve, lg)
    one = orc.from_dec(curve, FR, 1)
    inv = [orc.ntt(curve, v, w, inverse=True) for v in vs]
    shifted = [orc.distribute_powers(curve, x, g, one) for x in inv]
    want = {"forward": [orc.ntt(curve, v, w) for v in vs], "inverse": inv, "inverse with coset_gen": shifted,
            "coset pair": [orc.ntt(curve, x, w) for x in shifted]}
    run = {"forward": lambda d: ctx.ntt_dev(curve, d, n, w), "inverse": lambda d: ctx.ntt_dev(curve, d, n, w, inverse=True),
           "inverse with coset_gen": lambda d: ctx.ntt_dev(curve, d, n, w, inverse=True, coset_gen=g), "coset pair": lambda d: ctx.ntt_coset_pair_dev(curve, d, n, w, g)}
    if lg == 3:                                                                          # the tone is what its comment says
        bins = want["forward"][5]
        assert not bins[np.arange(n) != n // 2 + 1].any() and bins[n // 2 + 1].any()
    for name, fn in run.items():
        d = [ctx.to_device(v) for v in vs]
        try:
            fn(d)
            for i, b in enumerate(d):
                np.testing.assert_array_equal(b.download((n, 4)), want[name][i], err_msg=f"{name}, lg {lg}, vector {i}: {PATTERNS[i]}")
        finally:
            ctx.free_many(d)


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_nine_vectors_are_refused_and_left_unchanged(ctx, curve):
    lg = 6
    n = 1 << lg
    vs, w, g = vectors(curve, lg)
    vs = vs + [vs[7][::-1].copy()]
    d = [ctx.to_device(v) for v in vs]
    try:
        for fn in (lambda: ctx.ntt_dev(curve, d, n, w), lambda: ctx.ntt_dev(curve, d, n, w, inverse=True, coset_gen=g), lambda: ctx.ntt_coset_pair_dev(curve, d, n, w, g)):
            with pytest.raises(cg.BackendError, match="k out of range"):
                fn()
        for i, b in enumerate(d):
            np.testing.assert_array_equal(b.download((n, 4)), vs[i], err_msg=f"vector {i}")
    finally:
        ctx.free_many(d)


def refused_and_unchanged(ctx, curve, calls, message):
    """every call of `calls(d, n, w, g)` on eight lg-6 vectors raises `message`, and the buffers hold afterwards what they held before"""
    lg = 6
    n = 1 << lg
    vs, w, g = vectors(curve, lg)
    d = [ctx.to_device(v) for v in vs]
    try:
        for fn in calls(d, n, w, g):
            with pytest.raises(cg.BackendError, match=message):
                fn()
        for i, b in enumerate(d):
            np.testing.assert_array_equal(b.download((n, 4)), vs[i], err_msg=f"vector {i}")
    finally:
        ctx.free_many(d)


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_forward_transform_with_coset_gen_is_refused_and_leaves_the_vectors_unchanged(ctx, curve):
    refused_and_unchanged(ctx, curve, lambda d, n, w, g: [lambda: ctx.ntt_dev(curve, d, n, w, coset_gen=g)], "coset_gen is only supported with inverse != 0")


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_length_48_is_refused_and_leaves_the_vectors_unchanged(ctx, curve):
    refused_and_unchanged(ctx, curve, lambda d, n, w, g: [lambda: ctx.ntt_dev(curve, d, 48, w), lambda: ctx.ntt_dev(curve, d, 48, w, inverse=True, coset_gen=g),
                                                          lambda: ctx.ntt_coset_pair_dev(curve, d, 48, w, g)], "NTT length must be a power of two")
