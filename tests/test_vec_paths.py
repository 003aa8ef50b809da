"""The vector kernels (csrc/vec_kernels.hpp) on the launch paths their launchers (csrc/fr_impl.hpp) choose by size, each against Python integers
(tests/vec_ref.py: Montgomery representatives, R = 2^256).  Every comparison is exact and covers every output element.

  SpMV        one hand-built matrix of 8193 rows: its first 8192 rows take k_spmv_csr_wave (a wave per row, up to 2^13 rows), all 8193 take
              k_spmv_csr (a lane per row), so both kernels see the same row shapes; party -1, 0, 1, 2; the refusals of the C entry.
  prefix      product and sum past the first tile (k_prefix_tiles alone at 2048, the smallest k_prefix_fixup at 2049) and past the first trip
              of k_prefix_totals (256 tile totals per trip: one trip at 524288, a carry at 524289, an accumulated carry at 1048577), on inputs
              without a zero, so a wrong total or fix-up cannot hide behind one.
  inverse     k_vec_inverse's eight elements per lane with zeros in every slot pattern, a partial tail group included.
  canonical   k_vec_count_noncanonical on raw limbs around the modulus.
The Shamir share kernel's long polynomials are in test_plonk_shamir_party.py, the transforms' three-pass plans in test_ntt_edges.py."""
import os

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR
from product import cg, ensure_built
from vec_ref import Mont, from_ints, spmv_ints, to_ints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
FILL = np.uint64(0xA5A5A5A55A5A5A5A)                       # what an output buffer holds before a call: no result here has these limbs


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def filled(ctx, n):
    return ctx.to_device(np.full((max(n, 1), 4), FILL, dtype=np.uint64))


# ---- SpMV ----------------------------------------------------------------------------------------------------------------------------------
N_INPUTS, N_WITNESS, N_ROWS = 3, 61, 8193
LONG = (63, 64, 65, 128, 129)                                # around the wave kernel's stride of 64 and its tail
BLOCKS = (0, 244, N_ROWS - 13)                               # first rows of the three copies of the 13 shapes: rows 0..12, 244..256 (the 128-term
                                                             # row is 255, the 129-term row 256: two workgroups of the lane kernel), 8180..8192
_matrix = {}


def spmv_matrix(curve):
    """(row_ptr, col, coeff limbs, pub limbs, wa limbs, wb limbs), made once per curve and never changed.  Rows have 1..3 random terms, except
    the thirteen shapes of `shapes` below, placed at each of BLOCKS.  Column 1 (public) and column N_INPUTS + 1 (witness, both components)
    hold p - 1."""
    if curve not in _matrix:
        F = Mont(curve)
        rng = np.random.default_rng([23, curve])
        n_cols = N_INPUTS + N_WITNESS
        rnd = lambda k: to_ints(orc.random_field(curve, FR, k, rng))
        any_cols = lambda k: [int(c) for c in rng.integers(0, n_cols, size=k)]
        m1 = F.of(F.r - 1)                                   # the field's p - 1; the limbs p - 1 themselves are the largest an element holds
        shapes = [lambda: ([], []),                                                                  # empty
                  lambda: ([0, 2, 1], rnd(3)),                                                       # public signals only
                  lambda: ([N_INPUTS + 5, N_INPUTS + 60, N_INPUTS + 9], rnd(3)),                     # witness signals only
                  lambda: ([N_INPUTS + 7, 2, N_INPUTS + 7, 2], rnd(4)),                              # the same column twice, on either side
                  lambda: ([N_INPUTS - 1, N_INPUTS], rnd(2)),                                        # the two sides of the public/witness boundary
                  lambda: ([1, N_INPUTS + 4, N_INPUTS + 8], [0] + rnd(1) + [0]),                     # zero coefficients
                  lambda: ([1, N_INPUTS + 1], [m1, m1]),                                             # p - 1 times p - 1, as field values
                  lambda: ([1, N_INPUTS + 1, 0], [F.r - 1, F.r - 1, F.r - 1])]                       # ... and with the limbs p - 1 as coefficient
        shapes += [(lambda k=k: (any_cols(k), rnd(k))) for k in LONG]
        special = {b + i: s for b in BLOCKS for i, s in enumerate(shapes)}
        row_ptr, col, coeff = [0], [], []
        for r in range(N_ROWS):
            if r in special: c, v = special[r]()
            else:
                k = int(rng.integers(1, 4)); c, v = any_cols(k), rnd(k)
            col += c; coeff += v; row_ptr.append(len(col))
        pub, wa, wb = (orc.random_field(curve, FR, k, rng) for k in (N_INPUTS, N_WITNESS, N_WITNESS))
        pub[1] = wa[1] = wb[1] = from_ints([m1])[0]
        out = (np.array(row_ptr, dtype=np.uint32), np.array(col, dtype=np.uint32), from_ints(coeff), pub, wa, wb)
        for a in out: a.setflags(write=False)
        _matrix[curve] = out
    return _matrix[curve]


def test_spmv_matrix_is_valid_and_holds_its_shapes():
    """the hand-built matrix is what the ABI allows (monotone row_ptr, every column in range) and has the rows the module docstring names where
    it names them"""
    row_ptr, col, coeff, pub, wa, wb = spmv_matrix(BN254)
    assert row_ptr.shape == (N_ROWS + 1,) and row_ptr[0] == 0 and row_ptr[-1] == col.shape[0] == coeff.shape[0]
    assert (np.diff(row_ptr.astype(np.int64)) >= 0).all() and col.max() < N_INPUTS + N_WITNESS == pub.shape[0] + wa.shape[0]
    length = np.diff(row_ptr.astype(np.int64))
    for b in BLOCKS:
        assert length[b] == 0 and tuple(length[b + 8:b + 13]) == LONG
        assert (col[row_ptr[b + 1]:row_ptr[b + 2]] < N_INPUTS).all() and (col[row_ptr[b + 2]:row_ptr[b + 3]] >= N_INPUTS).all()
        assert sorted(col[row_ptr[b + 4]:row_ptr[b + 5]]) == [N_INPUTS - 1, N_INPUTS]
        assert not coeff[row_ptr[b + 5]].any() and coeff[row_ptr[b + 5] + 1].any()
    assert length[255] == 128 and length[256] == 129 and length[8191] == 128 and length[8192] == 129
    others = np.delete(length, [b + i for b in BLOCKS for i in range(13)])
    assert others.min() == 1 and others.max() == 3


@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
def test_integer_spmv_reference_equals_oracle_field_ops_on_the_poseidon_matrices(curve_name):
    """pins vec_ref.spmv_ints without a GPU: on the Poseidon fixture's A and B matrices it gives what test_gpu_parity.spmv_expected, built on
    the oracle's field operations, gives, for every party and both components"""
    from test_gpu_parity import rep3_share, spmv_expected
    curve = {"bn254": BN254, "bls12_381": BLS12_381}[curve_name]; F = Mont(curve)
    z = orc.ZKey(curve, os.path.join(GOLDEN, "groth16", curve_name, "poseidon", "circuit.zkey"))
    w = orc.read_wtns(curve, os.path.join(GOLDEN, "groth16", curve_name, "poseidon", "witness.wtns"))
    pub = w[:z.n_public + 1]
    wa, wb = rep3_share(curve, w[z.n_public + 1:], np.random.default_rng(9))
    for m in (0, 1):
        rp, col, co = z.matrix(m)
        for party in (-1, 0, 1, 2):
            a, b = (w[z.n_public + 1:], None) if party < 0 else (wa[party], wb[party])
            ea, eb = spmv_expected(curve, rp, col, co, pub, party, a, b)
            ia, ib = spmv_ints(F, rp, col, to_ints(co), to_ints(pub), party, to_ints(a), None if b is None else to_ints(b))
            np.testing.assert_array_equal(from_ints(ia), ea, err_msg=f"matrix {m} party {party} component a")
            np.testing.assert_array_equal(from_ints(ib), eb, err_msg=f"matrix {m} party {party} component b")


@pytest.mark.gpu
@CURVES
@pytest.mark.parametrize("n_rows", [N_ROWS - 1, N_ROWS], ids=["wave_8192", "lane_8193"])
def test_spmv_hand_built_rows_on_both_kernels(ctx, curve, n_rows):
    """8192 rows take k_spmv_csr_wave, 8193 take k_spmv_csr (launch_spmv_csr switches above 2^13): every output row of both components equals
    the Python-integer evaluation, and a row nobody wrote would still hold FILL"""
    F = Mont(curve)
    row_ptr, col, coeff, pub, wa, wb = spmv_matrix(curve)
    ints = [to_ints(x) for x in (coeff, pub, wa, wb)]
    d_rp, d_col, d_co, d_pub, d_wa, d_wb = (ctx.to_device(x) for x in (row_ptr[:n_rows + 1], col, coeff, pub, wa, wb))
    for party in (-1, 0, 1, 2):
        oa, ob = filled(ctx, n_rows), (None if party < 0 else filled(ctx, n_rows))
        ctx.spmv_csr(curve, d_rp, d_col, d_co, n_rows, d_pub, N_INPUTS, party, d_wa, None if party < 0 else d_wb, oa, ob)
        ea, eb = spmv_ints(F, row_ptr[:n_rows + 1], col, ints[0], ints[1], party, ints[2], None if party < 0 else ints[3])
        np.testing.assert_array_equal(oa.download((n_rows, 4)), from_ints(ea), err_msg=f"party {party} component a")
        if ob is not None:
            np.testing.assert_array_equal(ob.download((n_rows, 4)), from_ints(eb), err_msg=f"party {party} component b")
        ctx.free_many([oa] + ([ob] if ob is not None else []))
    ctx.free_many([d_rp, d_col, d_co, d_pub, d_wa, d_wb])


@pytest.mark.gpu
@CURVES
@pytest.mark.parametrize("n_rows", [N_ROWS - 1, N_ROWS], ids=["wave_8192", "lane_8193"])
def test_spmv_refuses_bad_arguments_and_leaves_the_outputs_unchanged(ctx, curve, n_rows):
    """party 3, and a REP3 party without its second witness component, are refused by the C entry before any launch"""
    row_ptr, col, coeff, pub, wa, wb = spmv_matrix(curve)
    d_rp, d_col, d_co, d_pub, d_wa, d_wb = (ctx.to_device(x) for x in (row_ptr[:n_rows + 1], col, coeff, pub, wa, wb))
    oa, ob = filled(ctx, n_rows), filled(ctx, n_rows)
    with pytest.raises(cg.BackendError, match="party must be"):
        ctx.spmv_csr(curve, d_rp, d_col, d_co, n_rows, d_pub, N_INPUTS, 3, d_wa, d_wb, oa, ob)
    for party in (0, 1, 2):
        with pytest.raises(cg.BackendError, match="REP3 needs both share components"):
            ctx.spmv_csr(curve, d_rp, d_col, d_co, n_rows, d_pub, N_INPUTS, party, d_wa, None, oa, ob)
    for o in (oa, ob):
        assert (o.download((n_rows, 4)) == FILL).all()
    ctx.free_many([d_rp, d_col, d_co, d_pub, d_wa, d_wb, oa, ob])


# ---- prefix product and sum ------------------------------------------------------------------------------------------------------------------
TILE = 2048                                                  # SCAN_ITEMS x 256 elements per tile of k_prefix_tiles; k_prefix_totals scans 256 tile totals per trip
_scan_inputs = {}


def scan_input(curve, n):
    """n random elements, none of them zero, made once and never changed"""
    if (curve, n) not in _scan_inputs:
        x = orc.random_field(curve, FR, n, np.random.default_rng([29, curve, n]))
        x.setflags(write=False)
        _scan_inputs[(curve, n)] = x
    return _scan_inputs[(curve, n)]


def check_scan(curve, op, got, x, last_nonzero=None):
    """`got` is the inclusive scan of x: got[0] == x[0] and got[i] == got[i - 1] (op) x[i] for EVERY i, the right-hand side by one vectorised
    call of the oracle's field operation on the product's own got[i - 1].  That is complete: got[0] is anchored on the input, and by induction
    got[i] is then the scan of x[0..i], each step taken by the oracle and none by the product; an error anywhere, a tile total or a fix-up
    included, breaks the equation at the first element it reaches.  Independently of the oracle, the last element (of the non-zero prefix,
    where x has a zero) is compared with a running product / sum in Python integers."""
    F, n = Mont(curve), x.shape[0]
    np.testing.assert_array_equal(got[0], x[0])
    if n > 1:
        step = orc.field_op(curve, FR, "mul" if op == "prod" else "add", got[:-1], x[1:])
        bad = np.flatnonzero((got[1:] != step).any(axis=1))
        assert bad.size == 0, f"{op}: {bad.size} elements break the recurrence, the first at {bad[0] + 1} (tile {(bad[0] + 1) // TILE}, trip {(bad[0] + 1) // (256 * TILE)})"
    k = n if last_nonzero is None else last_nonzero + 1
    reps = to_ints(x[:k])
    want = F.prod(reps) if op == "prod" else sum(reps) % F.r
    np.testing.assert_array_equal(got[k - 1], from_ints([want])[0], err_msg=f"{op}: element {k - 1} against Python integers")


SCAN_CASES = [(c, n) for n in (TILE, TILE + 1, 256 * TILE, 256 * TILE + 1) for c in (BN254, BLS12_381)] + [(BN254, 512 * TILE + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("curve,n", SCAN_CASES, ids=[f"{'bn254' if c == BN254 else 'bls12_381'}-{n}" for c, n in SCAN_CASES])
def test_prefix_product_and_sum_without_a_zero(ctx, curve, n):
    """2048: one full tile, no fix-up; 2049: the smallest fix-up; 524288: 256 tiles, exactly one trip of k_prefix_totals; 524289: 257 tiles, the
    first carry; 1048577 (BN254): 513 tiles, a carry that is accumulated over two trips.  See check_scan for what is compared and why it is complete."""
    x = scan_input(curve, n)
    assert x.any(axis=1).all(), "the input must hold no zero"
    d_x, d_o = ctx.to_device(x), filled(ctx, n)
    for op, fn in (("prod", ctx.vec_prefix_prod), ("sum", ctx.vec_prefix_sum)):
        fn(curve, d_o, d_x, n)
        got = d_o.download((n, 4))
        if op == "prod": assert got.any(axis=1).all()
        check_scan(curve, op, got, x)
    np.testing.assert_array_equal(d_x.download((n, 4)), x, err_msg="the input changed")
    ctx.free_many([d_x, d_o])


@pytest.mark.gpu
@CURVES
def test_prefix_product_with_one_zero_near_the_end(ctx, curve):
    """257 tiles with a single zero at n - 5: every product before it is non-zero and checked as above, everything from it on is zero"""
    n = 256 * TILE + 1
    x = scan_input(curve, n).copy(); x[n - 5] = 0
    d_x, d_o = ctx.to_device(x), filled(ctx, n)
    ctx.vec_prefix_prod(curve, d_o, d_x, n)
    got = d_o.download((n, 4))
    assert got[:n - 5].any(axis=1).all() and not got[n - 5:].any()
    check_scan(curve, "prod", got, x, last_nonzero=n - 6)
    ctx.free_many([d_x, d_o])


@pytest.mark.gpu
@CURVES
def test_prefix_product_of_minus_ones_alternates(ctx, curve):
    """every input is the representative of p - 1: the product is p - 1 at even indices and 1 at odd ones, every tile total is 1, and so is every
    exclusive prefix of the totals — the scan's identity element, which a fix-up by the sum's identity (zero) would wipe out"""
    F, n = Mont(curve), 256 * TILE + 1
    m1, one = from_ints([F.of(F.r - 1)])[0], from_ints([F.of(1)])[0]
    d_x, d_o = ctx.to_device(np.tile(m1, (n, 1))), filled(ctx, n)
    ctx.vec_prefix_prod(curve, d_o, d_x, n)
    got = d_o.download((n, 4))
    assert (got[0::2] == m1).all() and (got[1::2] == one).all()
    ctx.free_many([d_x, d_o])


@pytest.mark.gpu
@CURVES
def test_prefix_scans_in_place(ctx, curve):
    """out = in at 257 tiles: every lane reads its items before it writes them, and the fix-up touches only out"""
    n = 256 * TILE + 1
    x = scan_input(curve, n)
    for op, fn in (("prod", ctx.vec_prefix_prod), ("sum", ctx.vec_prefix_sum)):
        d = ctx.to_device(x)
        fn(curve, d, d, n)
        check_scan(curve, op, d.download((n, 4)), x)
        d.free()


# ---- inverse -----------------------------------------------------------------------------------------------------------------------------------
MIXED = list(range(16, 24)) + [32, 47, 51, 52]                 # a lane's whole group of 8; slot 0 of a group; slot 7 of a group; two adjacent slots
INVERSE_CASES = [(8, "every element", list(range(8))), (8, "slot 0", [0]), (8, "slot 7", [7]), (8, "slots 3 and 4", [3, 4]), (8, "none", []),
                 (9, "the whole first group", list(range(8))), (9, "the tail group's only element", [8]), (9, "slots 0 and 7", [0, 7]),
                 (1024, "mixed", MIXED), (1024, "mixed and the whole last group", MIXED + list(range(1016, 1024))),
                 (1031, "mixed and the tail's last element", MIXED + [1030]), (1031, "mixed and the tail's first element", MIXED + [1024]),
                 (1031, "the whole tail group", list(range(1024, 1031)))]


def inverse_input(curve, n, zeros):
    F = Mont(curve)
    x = orc.random_field(curve, FR, n, np.random.default_rng([31, curve, n]))
    special = {1: F.of(1), 2: F.of(F.r - 1), 5: 1, 6: F.r - 1, n - 2: F.of(F.r - 1), n - 3: F.of(1)}     # values 1 and p - 1, limbs 1 and p - 1
    if n > 64: special.update({33: F.of(1), 46: F.of(F.r - 1), 53: F.of(F.r - 1)})                       # ... in the groups that hold a zero
    for i, v in special.items(): x[i] = from_ints([v])[0]
    if zeros: x[zeros] = 0
    return x


def check_inverse(curve, got, x, zeros):
    F = Mont(curve)
    reps = to_ints(x)
    assert [i for i, a in enumerate(reps) if a == 0] == sorted(zeros)
    np.testing.assert_array_equal(got, from_ints([F.inv(a) if a else 0 for a in reps]))


@pytest.mark.gpu
@CURVES
@pytest.mark.parametrize("n,name,zeros", INVERSE_CASES, ids=[f"{n}-{name.replace(' ', '_')}" for n, name, _ in INVERSE_CASES])
def test_inverse_with_zeros_in_every_slot_pattern(ctx, curve, n, name, zeros):
    """zeros map to zero, every other element to pow(x, -1, p) in Python integers, Montgomery-converted; the output starts out as FILL, so an
    element that was not written shows"""
    x = inverse_input(curve, n, zeros)
    d_x, d_o = ctx.to_device(x), filled(ctx, n + 8)
    ctx.vec_inverse(curve, d_o, d_x, n)
    got = d_o.download((n + 8, 4))
    check_inverse(curve, got[:n], x, zeros)
    assert (got[n:] == FILL).all(), "written past the end"
    ctx.free_many([d_x, d_o])


@pytest.mark.gpu
@CURVES
def test_inverse_in_place(ctx, curve):
    n, zeros = 1031, MIXED + [1030]
    x = inverse_input(curve, n, zeros)
    d = ctx.to_device(x)
    ctx.vec_inverse(curve, d, d, n)
    check_inverse(curve, d.download((n, 4)), x, zeros)
    d.free()


# ---- canonical check -------------------------------------------------------------------------------------------------------------------------
def words32(v): return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
def from_words32(w): return sum(x << (32 * i) for i, x in enumerate(w))


@pytest.mark.gpu
@CURVES
def test_canonical_check_counts_the_planted_elements(ctx, curve):
    """cg_vec_check_canonical_dev on RAW LIMBS, not field values: the vector is what a peer's message holds, 256-bit integers of which those not
    below the modulus are counted.  4099 canonical random elements with planted ones at index 0, at the last index and on either side of the
    first workgroup boundary (255 | 256).  The kernel ADDS to the counter: a second call doubles it, and n = 0 leaves it alone."""
    n, p = 4099, orc.MODULI[(curve, FR)]
    pw = words32(p)
    assert all(pw), "the planted values below need every 32-bit word of p non-zero"
    bad = {"p": p, "p + 1": p + 1, "2^256 - 1": (1 << 256) - 1,
           "p in words 1..7, larger in word 0": from_words32([0xFFFFFFFF] + pw[1:]),
           "above p in the top word only, below it in every lower word": from_words32([w - 1 for w in pw[:7]] + [pw[7] + 1])}
    good = {"p - 1": p - 1, "0": 0, "p in the top word, smaller below": from_words32([0xFFFFFFFF] * 6 + [pw[6] - 1, pw[7]])}
    assert all(v >= p for v in bad.values()) and all(v < p for v in good.values()) and max(bad.values()) < 1 << 256
    B, G = list(bad.values()), list(good.values())
    planted = {0: B[0], 1: G[0], 2: B[1], 3: G[2], 4: B[4], 253: B[1], 254: B[4], 255: B[2], 256: B[3], 257: G[1], 258: G[2], 259: B[0],
               n - 4: G[0], n - 3: B[3], n - 2: G[2], n - 1: B[0]}
    v = orc.random_field(curve, FR, n, np.random.default_rng([37, curve]))
    for i, val in planted.items(): v[i] = from_ints([val])[0]
    n_bad = sum(a >= p for a in to_ints(v))
    assert n_bad == sum(val >= p for val in planted.values()) == 10 and {val for val in planted.values()} == set(B) | set(G)
    d_v, d_count = ctx.to_device(v), ctx.alloc(16).zero()
    count = lambda: int(d_count.download((1,))[0])
    ctx.vec_check_canonical(curve, d_v, n, d_count)
    assert count() == n_bad
    ctx.vec_check_canonical(curve, d_v, n, d_count)
    assert count() == 2 * n_bad, "the kernel adds to the counter"
    ctx.vec_check_canonical(curve, d_v, 0, d_count)
    assert count() == 2 * n_bad, "n = 0 leaves the counter alone"
    d_count.zero()
    ctx.vec_check_canonical(curve, d_v, 1, d_count)                                 # element 0 alone: p itself
    assert count() == 1
    d_count.zero()
    good_only = ctx.to_device(from_ints(G * 3 + [p - 1]))
    ctx.vec_check_canonical(curve, good_only, 10, d_count)
    assert count() == 0
    ctx.free_many([d_v, d_count, good_only])
