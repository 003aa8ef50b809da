"""Pins the restatement of the MSM's point side (tests/msm_stages.py) against the oracle before the kernels are held to it (tests/test_msm_stages.py):
on one small case per curve and group the pieces of every bucket sum to its merged value, every reduction kind's partial sums fold to the same point,
and that point is the oracle's MSM over the table and the scalars the schedule came from.  No GPU, nothing of the product."""
import random

import numpy as np
import pytest

import msm_schedule as ms
import msm_stages as st
import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, G1, G2

GROUPS = [(BN254, G1), (BN254, G2), (BLS12_381, G1), (BLS12_381, G2)]
IDS = ["bn254-g1", "bn254-g2", "bls12_381-g1", "bls12_381-g2"]
ROWS = 48


def case(curve, group):
    rnd, r = random.Random(31 + curve), ms.modulus(curve)
    table = st.Table(curve, group, [0 if j == 5 else rnd.randrange(1, r) for j in range(ROWS)])
    sc = ms.Scalars(curve, [rnd.randrange(r) for _ in range(ROWS - 4)] + [0, 1, r - 1, (1 << 200) - 1])
    return table, sc


@pytest.mark.parametrize("curve,group", GROUPS, ids=IDS)
def test_restatement_against_the_oracle(curve, group):
    table, sc = case(curve, group)
    want = orc.msm(curve, group, table.points(), sc.mont)
    assert want.any()
    #            shared, c: segments per window | bit sums | grid (the smallest) | one shared set in groups
    for shared, c in ((0, 8), (0, 13), (1, 8), (1, 18), (1, 5)):
        sched = st.from_scalars(curve, c, shared, sc)
        nwin = ms.nwin_of(curve, c)
        for L in (1, 5, 16):
            exp = st.Expected(sched, table, L, nwin * sc.n)
            assert exp.nchunks == -(-nwin * sc.n // L)
            for b in range(sched.nbuckets):
                assert exp.pieces_sum(b) == exp.merged[b], f"shared={shared}, c={c}, L={L}: the pieces of bucket {b} do not sum to it"
            tagged = np.flatnonzero(exp.cont_bucket != st.EMPTY)
            assert sorted(tagged.tolist()) == sorted(exp.cont), "a tag without a piece, or a piece without a tag"
        total = exp.folded()
        if shared:
            assert exp.fold_bits(exp.bit_sums(c)) == total
            log_l = min(10, c - 2); log_h = c - 1 - log_l
            cols, rows = exp.grid_sums(log_l, log_h)
            assert exp.fold_grid(cols, rows, log_l) == total
            assert sum(exp.group_sums(16)) % exp.r == total
        np.testing.assert_array_equal(st.points_of(curve, group, [total])[0], want, err_msg=f"shared={shared}, c={c}")


def test_points_of_is_the_generator_multiple():
    curve, group = BN254, G1
    r = ms.modulus(curve)
    pts = st.points_of(curve, group, [0, 1, 2, r - 1, r, r + 2])
    assert not pts[0].any() and not pts[4].any()
    np.testing.assert_array_equal(pts[2], orc.point_add(curve, group, pts[1], pts[1]))
    np.testing.assert_array_equal(pts[2], pts[5])
    assert not orc.point_add(curve, group, pts[1], pts[3]).any()


def test_from_counts_places_exactly_the_counts():
    curve, c = BN254, 8
    rng = np.random.default_rng(3)
    nbk = ms.nbuckets_of(c, ms.nwin_of(curve, c), 0)
    counts = np.zeros(nbk, dtype=np.int64); counts[[0, 3, 4, nbk - 1]] = [5, 1, 40, 2]
    s = st.from_counts(curve, c, 0, counts, 256, rng)
    assert (s.counts == counts).all() and s.total == 48 and s.sorted.size == 48 and int(s.offsets[4]) == 6
    p = s.padded(4)
    assert p.total == 4 + 1 + 4 + 2 and (p.kept[[0, 3, 4, nbk - 1]] == [4, 1, 4, 2]).all() and p.sorted.size == nbk * 4
    assert (p.sorted[16:20] == s.per_bucket[4][:4]).all() and p.sorted[13] == st.EMPTY and (p.counts == counts).all()
