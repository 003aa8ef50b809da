"""The Python restatement of the MSM's scalar side (tests/msm_schedule.py) pinned on the CPU, before tests/test_msm_schedule.py holds the kernels to
it: the signed digits reconstruct the scalar, stay in range and never carry out of the top window; the numpy form equals the integer form; and the
comparison functions accept every valid arrangement of a schedule and refuse the wrong ones the kernels could produce."""
import random

import numpy as np
import pytest

import msm_schedule as ms
from oracle_lib import BN254, BLS12_381
from test_msm_edges import digit_scalars

CURVES = [BN254, BLS12_381]
WINDOWS = [2, 3, 8, 13, 16, 20, 22]


def edge_values(curve, c):
    nwin = ms.nwin_of(curve, c)
    rnd, r = random.Random(100 * c + curve), ms.modulus(curve)
    return digit_scalars(curve, c) + ms.carry_scalars(curve, c, nwin) + [0, 1, r - 1] + [rnd.randrange(r) for _ in range(200)]


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("curve", CURVES, ids=["bn254", "bls12_381"])
def test_digits_reconstruct_the_scalar_and_stay_in_range(curve, c):
    nwin, half = ms.nwin_of(curve, c), 1 << (c - 1)
    vals = edge_values(curve, c)
    assert len(ms.carry_scalars(curve, c, nwin)) >= (4 if c < 22 else 2)
    digs, carry = ms.signed_digits(ms.limbs_of(vals), c, nwin)
    assert not carry.any()
    seen_zero_with_carry = False
    for k, s in enumerate(vals):
        d, top_carry = ms.digits_of_int(s, c, nwin)
        assert top_carry == 0, f"{s:#x} carries out of the top window"
        assert sum(x << (c * w) for w, x in enumerate(d)) == s
        assert all(-(half - 1) <= x <= half for x in d)
        assert d == [int(x) for x in digs[:, k]], f"numpy digits of {s:#x} differ from the integer ones"
        raw = [(s >> (c * w)) & ((1 << c) - 1) for w in range(nwin)]
        seen_zero_with_carry |= any(raw[w] == (1 << c) - 1 and d[w] == 0 for w in range(nwin))
    assert seen_zero_with_carry, "no 2^c - 1 digit under a carry among the inputs"
    # the boundary digits themselves: 2^(c-1) stays positive, 2^(c-1) + 1 turns into -(2^(c-1) - 1) with a carry
    assert ms.digits_of_int(half, c, nwin)[0][:2] == [half, 0]
    assert ms.digits_of_int(half + 1, c, nwin)[0][:2] == [-(half - 1), 1]


def arrange(exp, rng):
    """one valid arrangement of the expected schedule: every bucket's entries in a random order"""
    order = np.lexsort((rng.random(exp.total), exp.bucket))
    out = np.full(exp.nwin * exp.n, ms.EMPTY, dtype=np.uint32)
    out[:exp.total] = exp.payload[order]
    return out


@pytest.mark.parametrize("shared", [0, 1])
def test_dense_comparison_accepts_valid_and_refuses_wrong_schedules(shared):
    curve, c, n = BN254, 8, 700
    nwin = ms.nwin_of(curve, c)
    sc = ms.distribution("uniform", curve, c, nwin, n)
    exp = ms.Schedule(sc.limbs, c, nwin, shared)
    assert exp.total == int(exp.counts.sum()) and int(exp.offsets[-1]) + int(exp.counts[-1]) == exp.total
    rng = np.random.default_rng(5)
    good = arrange(exp, rng)
    ms.check_dense(exp, exp.counts.copy(), exp.offsets.copy(), good)
    ms.check_dense(exp, exp.counts.copy(), exp.offsets.copy(), arrange(exp, rng))
    full = int(np.flatnonzero(exp.counts)[0]); at = int(exp.offsets[full])
    other = int(np.flatnonzero(exp.counts)[-1]); at2 = int(exp.offsets[other])

    def refused(counts=None, offsets=None, sorted_=None):
        with pytest.raises(AssertionError):
            ms.check_dense(exp, exp.counts if counts is None else counts, exp.offsets if offsets is None else offsets, good if sorted_ is None else sorted_)
    s = good.copy(); s[at] ^= 0x80000000; refused(sorted_=s)                       # a flipped sign
    s = good.copy(); s[at] ^= 1; refused(sorted_=s)                                # another point
    s = good.copy(); s[at], s[at2] = s[at2], s[at]; refused(sorted_=s)             # two entries in each other's bucket
    s = good.copy(); s[at] = s[at + 1] if exp.counts[full] > 1 else ms.EMPTY; refused(sorted_=s)   # an entry twice / a hole
    if exp.total < s.size:
        s = good.copy(); s[exp.total] = 0; refused(sorted_=s)                      # a write behind the end
    if shared:
        s = good.copy(); s[at] ^= 1 << 24; refused(sorted_=s)                      # another window
    k = exp.counts.copy(); k[full] += 1; refused(counts=k)
    o = exp.offsets.copy(); o[other] += 1; refused(offsets=o)


def test_direct_comparison_accepts_valid_and_refuses_wrong_schedules():
    curve, c, n, cap = BN254, 8, 600, 4
    nwin = ms.nwin_of(curve, c)
    exp = ms.Schedule(ms.distribution("uniform", curve, c, nwin, n).limbs, c, nwin, 0)
    over = exp.counts > cap
    assert over.any() and (~over & (exp.counts > 0)).any()
    slots = np.full((exp.nbuckets, cap), ms.EMPTY, dtype=np.uint32)
    for b in np.flatnonzero(exp.counts):
        mine = exp.payload[exp.bucket == b][::-1][:cap]
        slots[b, :mine.size] = mine
    offsets = ms.exclusive_scan(np.minimum(exp.counts, cap))
    ms.check_direct(exp, cap, exp.counts, offsets, slots.ravel(), 1)
    with pytest.raises(AssertionError):
        ms.check_direct(exp, cap, exp.counts, offsets, slots.ravel(), 0)            # the flag must be set
    with pytest.raises(AssertionError):
        ms.check_direct(exp, cap, exp.counts, ms.exclusive_scan(exp.counts), slots.ravel(), 1)   # offsets from the true counts
    b = int(np.flatnonzero(over)[0])
    s = slots.copy(); s[b, 1] = s[b, 0]
    with pytest.raises(AssertionError):
        ms.check_direct(exp, cap, exp.counts, offsets, s.ravel(), 1)                # an overflowing bucket with one entry twice
    b = int(np.flatnonzero(~over & (exp.counts > 0))[0])
    s = slots.copy(); s[b, 0] ^= 0x80000000
    with pytest.raises(AssertionError):
        ms.check_direct(exp, cap, exp.counts, offsets, s.ravel(), 1)
    quiet = ms.Schedule(ms.distribution("all zero", curve, c, nwin, 5).limbs, c, nwin, 0)
    ms.check_direct(quiet, cap, quiet.counts, quiet.offsets, np.full(quiet.nbuckets * cap, ms.EMPTY, dtype=np.uint32), 0)


@pytest.mark.parametrize("c,shared", [(13, 1), (16, 0), (21, 1)])
def test_distributions_have_the_shape_they_are_named_for(c, shared):
    """far regions put entries outside an item tile's window, near regions (one bucket set) none; hot bucket fills the last bucket of every set;
    staircase fills buckets evenly; all zero has no entries"""
    curve = BN254
    nwin, half = ms.nwin_of(curve, c), 1 << (c - 1)
    n = 40000 // nwin * 2 + 11
    sched = lambda name: ms.Schedule(ms.distribution(name, curve, c, nwin, n).limbs, c, nwin, shared)
    far, near = sched("far regions"), sched("near regions")
    assert far.total > ms.ITEM_TILE and far.direct_items() > 0
    assert set(np.flatnonzero(far.counts) % half) == {0, half - 2, half - 1} and (far.payload >> 31).any()     # 1, -(2^(c-1) - 1), 2^(c-1)
    assert (far.bucket % half >= half - 2).sum() * 2 > far.total, "most entries lie in the last region of a bucket set"
    assert near.total > ms.ITEM_TILE and (np.flatnonzero(near.counts) % half).max() < ms.ITEM_WINDOW
    if shared:
        assert near.direct_items() == 0
    hot = sched("hot bucket")
    assert set(np.flatnonzero(hot.counts) % half) == {half - 1} and not (hot.payload >> 31).any()
    assert sched("all zero").total == 0
    stairs = ms.Schedule(ms.distribution("staircase", curve, 8, ms.nwin_of(curve, 8), 1280).limbs, 8, ms.nwin_of(curve, 8), 1)
    assert stairs.counts.min() >= 10 * (ms.nwin_of(curve, 8) - 1) and stairs.counts.max() <= 10 * ms.nwin_of(curve, 8)
