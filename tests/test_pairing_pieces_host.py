"""The pieces of csrc/pairing.hpp one by one against the integer tower of tests/pairing_tower.py, on the host under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sanitize/pairing_pieces_main.cpp (the header compiled as plain C++ into a stand-alone program, run as a child
process) applies every primitive to the cases this file writes, and every result is compared bit for bit here.  The tower is pinned to the
oracle's pairing values first, without the product.  The last test calls the host entries of the library on 8-byte-aligned buffers.
No GPU involved."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, G1, G2, ROOT
from pairing_tower import tower
from product import cg, ensure_built

CURVES = [BN254, BLS12_381]
SAN = os.path.join(ROOT, "tests", "sanitize")
NAMES = {BN254: "bn254", BLS12_381: "bls12_381"}
MUL, SQR, CONJ, MUL_LINE, INV, FP6_MUL, FP6_INV, FROB2, FEXP, MDBL, MADD, MCHAIN, MLOOP, TAIL, UNALIGNED = range(1, 16)
KIND_NAMES = {MUL: "fp12_mul", SQR: "fp12_sqr", CONJ: "fp12_conj", MUL_LINE: "mul_line", INV: "fp12_inverse", FP6_MUL: "fp6_mul", FP6_INV: "fp6_inverse",
              FROB2: "fp12_frob2", FEXP: "final_exp", MDBL: "miller_double", MADD: "miller_add", MCHAIN: "miller_chain", MLOOP: "miller_loop", TAIL: "bn_tail",
              UNALIGNED: "unaligned"}
CHAIN_STEPS, CHAIN_OPS = 8, 0x52          # steps 1, 4, 6 add Q: T = 2, 3, 6, 12, 13, 26, 27, 54 times Q
CHAIN_MULTIPLES = [2, 3, 6, 12, 13, 26, 27, 54]


def seeded_points(curve, n, seed):
    rng = np.random.default_rng(seed + curve)
    ks = orc.random_field(curve, FR, 2 * n, rng)
    return [orc.generator_mul(curve, G1, k) for k in ks[:n]], [orc.generator_mul(curve, G2, k) for k in ks[n:]], ks


# ---- the tower, pinned without the product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_tower_is_pinned_to_the_oracle(curve):
    """v = e(P, Q) of the oracle has order r in the tower (a wrong xi or layout map breaks that), e(2P, Q) = v^2, and the tower's final
    exponentiation of a random element lands in the order-r subgroup"""
    T = tower(curve)
    assert T.p == orc.MODULI[(curve, orc.FQ)] and T.r == orc.MODULI[(curve, FR)]
    g1, g2, _ = seeded_points(curve, 2, 5100)
    two = orc.from_dec(curve, FR, 2)
    for P, Q in zip(g1, g2):
        v = T.from_abi(orc.pairing(curve, P, Q))
        assert v != T.one and T.pow(v, T.r) == T.one
        P2 = orc.points_mul(curve, G1, P[None, :], two[None, :])[0]
        assert T.from_abi(orc.pairing(curve, P2, Q)) == T.mul(v, v)
        np.testing.assert_array_equal(T.to_abi(v), orc.pairing(curve, P, Q))
    a = T.random_element(random.Random(77 + curve))
    e = T.final_exp(a)
    assert e != T.one and T.pow(e, T.r) == T.one
    assert T.final_exp(T.zero) == T.zero and T.final_exp(T.one) == T.one
    g = T.gamma()
    assert pow(g, 6, T.p) == 1 and pow(g, 3, T.p) == T.p - 1                       # a primitive sixth root of unity in Fp


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def edge_fp(T, rng):
    """base-field VALUES whose Montgomery limbs (what the product's arithmetic sees) or whose values sit on an edge"""
    p = T.p
    raw = [0, 1, p - 1, T.R % p, (p - 1) // 2, (p + 1) // 2]
    if T.curve == BN254:        # mul29 repacks eight 32-bit words into nine 29-bit limbs: limbs of all ones
        raw += [(1 << 29) - 1, (1 << 116) - 1, (1 << 232) - 1, (1 << 253) - 1, (((p >> 232) - 1) << 232) | ((1 << 232) - 1)]
    else:                       # the top 32-bit limb zero, and equal to the modulus's
        top = p >> 352
        raw += [(1 << 352) - 1, rng.randrange(1 << 352), top << 352, (top << 352) | rng.randrange(p & ((1 << 352) - 1))]
    assert all(0 <= w < p for w in raw)
    vals = [w * T.Rinv % p for w in raw] + [p - 1, (p - 1) // 2, (p + 1) // 2, 2]
    return list(dict.fromkeys(vals))


def edge_fp2(T, rng):
    """per Fp2 coefficient: one component zero, c0 = c1, c0 = -c1 (c0 + c1 = 0), c0 + c1 = +-1: what Karatsuba's sums and differences meet"""
    p, out = T.p, []
    for e in edge_fp(T, rng):
        out += [(e, 0), (0, e), (e, e), (e, -e % p), (e, (1 - e) % p), (e, (-1 - e) % p)]
    return list(dict.fromkeys(out))


def ring_operands(T, rng, n_random=64):
    """every edge coefficient in one place at a time (the others random) and in all six at once, then random elements"""
    out = []
    for e in edge_fp2(T, rng):
        for k in range(6):
            a = list(T.random_element(rng)); a[k] = e; out.append(tuple(a))
        out.append((e,) * 6)
    return out + [T.random_element(rng) for _ in range(n_random)]


def fp2_sqrt(T, a):
    """a square root in Fp2 (p = 3 mod 4) or None"""
    p = T.p
    if a == (0, 0):
        return a
    s = pow((a[0] * a[0] + a[1] * a[1]) % p, (p + 1) // 4, p)
    if s * s % p != (a[0] * a[0] + a[1] * a[1]) % p:
        return None
    for sign in (1, -1):
        h = (a[0] + sign * s) * pow(2, -1, p) % p
        x0 = pow(h, (p + 1) // 4, p)
        if x0 * x0 % p == h and x0:
            r = (x0, a[1] * pow(2 * x0, -1, p) % p)
            if T.f2_mul(r, r) == a:
                return r
    return None


def random_twist_point(T, rng):
    """a point of E'(Fp2), almost surely outside the order-r subgroup (the cofactor is larger than r)"""
    while True:
        x = T.random_fp2(rng)
        y = fp2_sqrt(T, T.f2_add(T.f2_mul(T.f2_mul(x, x), x), T.b_twist))
        if y is not None:
            assert T.on_twist((x, y))
            return (x, y)


class CaseFile:
    """blocks of (curve, kind, records) in the order written; a record is a flat list of u64 words"""

    def __init__(self):
        self.blocks = []

    def add(self, curve, kind, records, out_words, meta):
        assert records and all(len(r) == len(records[0]) for r in records)
        self.blocks.append({"curve": curve, "kind": kind, "records": records, "out_words": out_words, "meta": meta})

    def write(self, path):
        words = []
        for b in self.blocks:
            words += [b["curve"], b["kind"], len(b["records"])]
            for r in b["records"]:
                words += r
        np.array(words, dtype=np.uint64).tofile(path)

    def read_results(self, path):
        w = np.fromfile(path, dtype=np.uint64)
        at = 0
        for b in self.blocks:
            n = len(b["records"])
            assert [int(v) for v in w[at: at + 3]] == [b["curve"], b["kind"], n]
            at += 3
            b["out"] = [[int(v) for v in w[at + i * b["out_words"]: at + (i + 1) * b["out_words"]]] for i in range(n)]
            at += n * b["out_words"]
        assert at == w.size


def g1_ints(T, P): return (T.fp_from_limbs(P[: T.limbs]), T.fp_from_limbs(P[T.limbs:]))
def g2_ints(T, Q): return (T.f2_from_words(list(Q[: 2 * T.limbs])), T.f2_from_words(list(Q[2 * T.limbs:])))
def fp_words(T, P): return T.fp_to_limbs(P[0]) + T.fp_to_limbs(P[1])
def pt_words(T, Q): return T.f2_to_words(Q[0]) + T.f2_to_words(Q[1])
def jac_words(T, X, Y, Z): return T.f2_to_words(X) + T.f2_to_words(Y) + T.f2_to_words(Z)


def jacobian_of(T, pt, z):
    zz = T.f2_mul(z, z)
    return (T.f2_mul(pt[0], zz), T.f2_mul(pt[1], T.f2_mul(zz, z)), z)


def build_cases(curve, cf):
    T = tower(curve)
    rng = random.Random(9100 + curve)
    L, E = T.limbs, 12 * T.limbs
    ops = ring_operands(T, rng)
    n = len(ops)
    assert n >= 300
    w12 = T.to_words
    e2 = edge_fp2(T, rng)
    # products: an edge element with another edge element (even cases) or a random one (odd)
    bs = [ops[(7 * i + 3) % n] if i % 2 == 0 else T.random_element(rng) for i in range(n)]
    cf.add(curve, MUL, [w12(a) + w12(b) for a, b in zip(ops, bs)], E, (ops, bs))
    cf.add(curve, SQR, [w12(a) for a in ops], E, ops)
    cf.add(curve, CONJ, [w12(a) for a in ops], E, ops)
    lines = [(e2[i % len(e2)], e2[(5 * i + 1) % len(e2)], e2[(11 * i + 2) % len(e2)]) if i % 2 == 0 else (T.random_fp2(rng), T.random_fp2(rng), T.random_fp2(rng))
             for i in range(n)]
    cf.add(curve, MUL_LINE, [w12(a) + T.f2_to_words(l[0]) + T.f2_to_words(l[1]) + T.f2_to_words(l[2]) for a, l in zip(ops, lines)], E, (ops, lines))
    cf.add(curve, INV, [w12(a) for a in ops], E, ops)
    # Fp6 through the same cases: the even and the odd coefficients of every element
    six = [((a[0], a[2], a[4]), (a[1], a[3], a[5])) for a in ops]
    flat6 = lambda x: T.f2_to_words(x[0]) + T.f2_to_words(x[1]) + T.f2_to_words(x[2])
    cf.add(curve, FP6_MUL, [flat6(x) + flat6(y) for x, y in six], 6 * L, six)
    cf.add(curve, FP6_INV, [flat6(x) for x, _ in six] + [flat6(y) for _, y in six], 6 * L, [x for x, _ in six] + [y for _, y in six])
    cf.add(curve, FROB2, [w12(a) for a in ops], E, ops)
    sp = T.special_elements()
    fe = [sp[k] for k in ("zero", "one", "minus_one", "fp6", "all_pm1", "all_minus_one", "line", "pure_odd")] + [T.random_element(rng) for _ in range(4)]
    assert len(fe) <= 12
    cf.add(curve, FEXP, [w12(a) for a in fe], E, fe)
    # Miller steps: T = m Q in Jacobian form with a random Z (and Z = 1 once), P and Q multiples of the generators
    g1, g2, _ = seeded_points(curve, 3, 6100)
    dbl, add = [], []
    for i, (P, Q) in enumerate(zip(g1, g2)):
        Pi, Qi = g1_ints(T, P), g2_ints(T, Q)
        assert T.on_twist(Qi)
        for m in (1, 2, 3, 5, 7):
            t = T.twist_mul(Qi, m)
            z = T.one2 if (m == 1 and i == 0) else T.random_fp2(rng)
            dbl.append((Pi, t, jacobian_of(T, t, z)))
        for m, k in ((2, 1), (3, 1), (5, 1), (6, 1), (5, 2), (2, 7)):
            t, r = T.twist_mul(Qi, m), T.twist_mul(Qi, k)
            z = T.one2 if (m == 2 and i == 0) else T.random_fp2(rng)
            add.append((Pi, t, r, jacobian_of(T, t, z)))
    cf.add(curve, MDBL, [jac_words(T, *j) + fp_words(T, P) for P, _, j in dbl], 12 * L, dbl)
    cf.add(curve, MADD, [jac_words(T, *j) + pt_words(T, r) + fp_words(T, P) for P, _, r, j in add], 12 * L, add)
    chains = [(g1_ints(T, P), g2_ints(T, Q)) for P, Q in zip(g1, g2)]
    cf.add(curve, MCHAIN, [fp_words(T, P) + pt_words(T, Q) + [CHAIN_OPS] for P, Q in chains], CHAIN_STEPS * 12 * L, chains)
    # whole Miller loops on inputs outside the contract (host only): Q on the twist outside the subgroup, Q off the curve, P off the curve
    P0, Q0 = chains[0]
    outside = [(P0, random_twist_point(T, rng)), (chains[1][0], random_twist_point(T, rng)),
               (P0, (T.random_fp2(rng), T.random_fp2(rng))), (P0, (Q0[0], T.f2_add(Q0[1], T.one2))),
               ((rng.randrange(T.p), rng.randrange(T.p)), Q0), ((P0[0], (P0[1] + 1) % T.p), Q0),
               ((rng.randrange(T.p), rng.randrange(T.p)), random_twist_point(T, rng))]
    cf.add(curve, MLOOP, [fp_words(T, P) + pt_words(T, Q) for P, Q in outside], E, outside)
    if curve == BN254:
        cf.add(curve, TAIL, [[int(v) for v in Q] for Q in g2], 8 * L, g2)
    una = [sp["all_pm1"], sp["dense"], T.random_element(rng)]
    cf.add(curve, UNALIGNED, [w12(a) for a in una], E, una)


# ---- the comparisons -------------------------------------------------------------------------------------------------------------------
def check_line(T, what, line_words, lam, t_before, P):
    """(a0', a1, a3) = s yP (1, -lambda xP / yP, (lambda x_T - y_T) / yP) as cross products, s unknown: a1 yP = -lambda xP a0', a3 yP = (lambda x_T - y_T) a0'"""
    n = 2 * T.limbs
    a0, a1, a3 = (T.f2_from_words(line_words[i * n: (i + 1) * n]) for i in range(3))
    a0p = a0 if T.twist_d else T.f2_mul(a0, T.f2_inv(T.xi))
    xP, yP = P
    assert a0p != T.zero2, what
    assert T.f2_scale(a1, yP) == T.f2_scale(T.f2_mul(T.f2_neg(lam), a0p), xP), f"{what}: the line's x coefficient"
    assert T.f2_scale(a3, yP) == T.f2_mul(T.f2_sub(T.f2_mul(lam, t_before[0]), t_before[1]), a0p), f"{what}: the line's constant"


def jac_from_words(T, w):
    n = 2 * T.limbs
    return tuple(T.f2_from_words(w[i * n: (i + 1) * n]) for i in range(3))


def check_block(b):
    curve, kind, meta, out = b["curve"], b["kind"], b["meta"], b["out"]
    T = tower(curve)
    L = T.limbs
    name = f"{NAMES[curve]} {KIND_NAMES[kind]}"
    f12 = T.from_words
    f6 = lambda w: tuple(T.f2_from_words(w[i * 2 * L: (i + 1) * 2 * L]) for i in range(3))
    up6 = lambda x: (x[0], T.zero2, x[1], T.zero2, x[2], T.zero2)                 # Fp6 inside Fp12: v = w^2
    if kind == MUL:
        for i, (a, c, o) in enumerate(zip(meta[0], meta[1], out)):
            assert f12(o) == T.mul(a, c), f"{name} case {i}"
    elif kind == SQR:
        for i, (a, o) in enumerate(zip(meta, out)):
            assert f12(o) == T.mul(a, a), f"{name} case {i}"
    elif kind == CONJ:
        for i, (a, o) in enumerate(zip(meta, out)):
            assert f12(o) == T.conj(a), f"{name} case {i}"
    elif kind == MUL_LINE:
        for i, (a, l, o) in enumerate(zip(meta[0], meta[1], out)):
            assert f12(o) == T.mul(a, T.line_dense(*l)), f"{name} case {i}"
    elif kind == INV:
        zeros = 0
        for i, (a, o) in enumerate(zip(meta, out)):
            if a == T.zero:
                zeros += 1
                assert f12(o) == T.zero, f"{name} case {i}: inverse(0)"
            else:
                assert T.mul(a, f12(o)) == T.one, f"{name} case {i}"
        assert zeros >= 1
    elif kind == FP6_MUL:
        for i, ((x, y), o) in enumerate(zip(meta, out)):
            assert up6(f6(o)) == T.mul(up6(x), up6(y)), f"{name} case {i}"
    elif kind == FP6_INV:
        zeros = 0
        for i, (x, o) in enumerate(zip(meta, out)):
            if x == (T.zero2,) * 3:
                zeros += 1
                assert f6(o) == x, f"{name} case {i}: inverse(0)"
            else:
                assert T.mul(up6(x), up6(f6(o))) == T.one, f"{name} case {i}"
        assert zeros >= 1
    elif kind == FROB2:
        g = T.gamma()
        for i, (a, o) in enumerate(zip(meta, out)):
            assert f12(o) == tuple(T.f2_scale(c, pow(g, k, T.p)) for k, c in enumerate(a)), f"{name} case {i}"
        for i in (len(meta) - 1, len(meta) - 2):                                    # and the plain power, on two random dense elements
            assert f12(out[i]) == T.pow(meta[i], T.p * T.p), f"{name} case {i}: a^(p^2)"
    elif kind == FEXP:
        for i, (a, o) in enumerate(zip(meta, out)):
            assert f12(o) == T.final_exp(a), f"{name} case {i}"
        assert f12(out[0]) == T.zero and f12(out[1]) == T.one and f12(out[3]) == T.one
    elif kind == MDBL:
        for i, ((P, t, _), o) in enumerate(zip(meta, out)):
            want, lam = T.twist_double(t)
            assert T.jacobian_to_affine(*jac_from_words(T, o[: 6 * L])) == want, f"{name} case {i}: 2T"
            check_line(T, f"{name} case {i}", o[6 * L:], lam, t, P)
    elif kind == MADD:
        for i, ((P, t, r, _), o) in enumerate(zip(meta, out)):
            want, lam = T.twist_add(t, r)
            assert T.jacobian_to_affine(*jac_from_words(T, o[: 6 * L])) == want, f"{name} case {i}: T + R"
            check_line(T, f"{name} case {i}", o[6 * L:], lam, t, P)
    elif kind == MCHAIN:
        for i, ((P, Q), o) in enumerate(zip(meta, out)):
            t = Q
            for s in range(CHAIN_STEPS):
                want, lam = T.twist_add(t, Q) if (CHAIN_OPS >> s) & 1 else T.twist_double(t)
                rec = o[s * 12 * L: (s + 1) * 12 * L]
                assert T.jacobian_to_affine(*jac_from_words(T, rec[: 6 * L])) == want, f"{name} case {i} step {s}"
                assert want == T.twist_mul(Q, CHAIN_MULTIPLES[s])
                check_line(T, f"{name} case {i} step {s}", rec[6 * L:], lam, t, P)
                t = want
    elif kind == MLOOP:
        assert len(out) == len(meta)                                                # the value is not compared: the run is the check
    elif kind == TAIL:
        p_r = orc.from_dec(curve, FR, T.p % T.r); p2_r = orc.from_dec(curve, FR, T.p * T.p % T.r)
        gx, gy = T.f2_pow(T.xi, (T.p - 1) // 3), T.f2_pow(T.xi, (T.p - 1) // 2)
        for i, (Q, o) in enumerate(zip(meta, out)):
            q1 = np.array(o[: 4 * L], dtype=np.uint64); q2 = np.array(o[4 * L:], dtype=np.uint64)
            Qi = g2_ints(T, Q)
            pi = lambda pt: (T.f2_mul(T.f2_conj(pt[0]), gx), T.f2_mul(T.f2_conj(pt[1]), gy))
            piQ = pi(Qi); pi2Q = pi(piQ)
            assert g2_ints(T, q1) == piQ and g2_ints(T, q2) == (pi2Q[0], T.f2_neg(pi2Q[1])), f"{name} case {i}: the tower's Frobenius"
            assert T.on_twist(g2_ints(T, q1)) and T.on_twist(g2_ints(T, q2))
            # on the order-r subgroup pi acts as multiplication by p
            np.testing.assert_array_equal(q1, orc.points_mul(curve, G2, Q[None, :], p_r[None, :])[0], err_msg=f"{name} case {i}: pi(Q) = [p] Q")
            neg2 = np.array(pt_words(T, (pi2Q[0], pi2Q[1])), dtype=np.uint64)
            np.testing.assert_array_equal(neg2, orc.points_mul(curve, G2, Q[None, :], p2_r[None, :])[0], err_msg=f"{name} case {i}: pi^2(Q) = [p^2] Q")
    elif kind == UNALIGNED:
        for i, (a, o) in enumerate(zip(meta, out)):
            assert f12(o) == a, f"{name} case {i}"
    else:
        raise AssertionError(kind)


def test_pairing_pieces_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-j2", "-C", SAN, "-f", "pairing_pieces.mk"], stdout=subprocess.DEVNULL, timeout=1200)
    cf = CaseFile()
    for curve in CURVES:
        build_cases(curve, cf)
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    cf.write(cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(SAN, "_build", "pairing_pieces_main"), cases, results], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-6000:]
    assert p.stdout.endswith("done\n")
    for b in cf.blocks:                                         # the program read every block at its full length
        assert f"{NAMES[b['curve']]} {KIND_NAMES[b['kind']]}: {len(b['records'])} cases\n" in p.stdout
    assert {(b["curve"], b["kind"]) for b in cf.blocks} == {(c, k) for c in CURVES for k in KIND_NAMES if (k != TAIL or c == BN254)}
    cf.read_results(results)
    for b in cf.blocks:
        check_block(b)


# ---- the library's host entries on buffers that are 8- but not 16-byte aligned ------------------------------------------------------------
def misaligned(words):
    """a zeroed uint64 view of `words` elements at an address = 8 mod 16 (kept alive by its base)"""
    base = np.zeros(words + 2, dtype=np.uint64)
    v = base[1: 1 + words] if base.ctypes.data % 16 == 0 else base[: words]
    assert v.ctypes.data % 16 == 8 and v.size == words
    return v


@pytest.mark.parametrize("curve", CURVES)
def test_plonk_host_entry_accepts_8_byte_aligned_buffers(curve):
    """cg_plonk_verify_scalars_host with every input and output at an address = 8 mod 16: the values of the aligned call.  (The inputs are
    seeded reduced field elements: the function only hashes the points and computes with the scalars.)"""
    ensure_built()
    lib = cg.load()
    nq = tower(curve).limbs
    rng = np.random.default_rng(61 + curve)
    n, n_pub, power = 3, 2, 5
    fq = lambda *shape: orc.random_field(curve, orc.FQ, int(np.prod(shape)), rng).reshape(*shape, nq)
    fr = lambda *shape: orc.random_field(curve, FR, int(np.prod(shape)), rng).reshape(*shape, 4)
    key = dict(points=fq(8, 2).reshape(8, 2 * nq), k1=fr(1)[0], k2=fr(1)[0], omega=fr(1)[0], power=power)
    commits, evals, pubs = fq(n, 9, 2).reshape(n, 9, 2 * nq), fr(n, 6), fr(n, n_pub)
    coeff = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
    want = cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs, coeff)

    def off(arr):
        v = misaligned(arr.size); v[:] = np.asarray(arr, dtype=np.uint64).reshape(-1); return v

    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    ins = [off(a) for a in (key["points"], key["k1"], key["k2"], key["omega"], commits, evals, pubs, coeff)]
    ch, sp, sk, sums = misaligned(n * 6 * 4), misaligned(n * 11 * 4), misaligned(n * 9 * 4), misaligned(9 * 4)
    valid = np.zeros(n, dtype=np.int32)
    rc = lib.cg_plonk_verify_scalars_host(curve, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), power, ptr(ins[4]), ptr(ins[5]), ptr(ins[6]),
                                          C.c_size_t(n_pub), C.c_size_t(n), ptr(ins[7]), ptr(ch), ptr(sp), ptr(sk), ptr(valid), ptr(sums))
    assert rc == 0, lib.cg_last_error().decode()
    for got, name in ((ch, "challenges"), (sp, "proof_scalars"), (sk, "key_scalars"), (sums, "key_sums")):
        assert got.any()
        np.testing.assert_array_equal(got, want[name].reshape(-1), err_msg=name)
    np.testing.assert_array_equal(valid, want["valid"])


@pytest.mark.parametrize("curve", CURVES)
def test_host_entries_accept_8_byte_aligned_buffers(curve):
    """cg_final_exp, cg_fp12_mul, cg_fp12_pow (and cg_pairing, cg_miller_loop's output) through views at addresses = 8 mod 16, inputs and
    outputs: the same values as the aligned calls.  A Rust caller's [u64; N] is aligned like this."""
    ensure_built()
    lib = cg.load()
    T = tower(curve)
    E = 12 * T.limbs
    rng = random.Random(31 + curve)
    a, b = T.to_abi(T.random_element(rng)), T.to_abi(T.random_element(rng))

    def chk(rc):
        assert rc == 0, lib.cg_last_error().decode()

    def off(arr):
        v = misaligned(arr.size); v[:] = np.asarray(arr, dtype=np.uint64).reshape(-1); return v

    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    ua, ub = off(a), off(b)
    out = misaligned(E); chk(lib.cg_fp12_mul(curve, ptr(ua), ptr(ub), ptr(out)))
    np.testing.assert_array_equal(out.reshape(a.shape), cg.fp12_mul(curve, a, b))
    np.testing.assert_array_equal(out.reshape(a.shape), T.to_abi(T.mul(T.from_abi(a), T.from_abi(b))))
    out = misaligned(E); chk(lib.cg_final_exp(curve, ptr(ua), ptr(out)))
    np.testing.assert_array_equal(out.reshape(a.shape), cg.final_exp(curve, a))
    e = off(np.array([0x123456789abcdef1, 0x5], dtype=np.uint64))
    out = misaligned(E); chk(lib.cg_fp12_pow(curve, ptr(ua), ptr(e), 2, ptr(out)))
    np.testing.assert_array_equal(out.reshape(a.shape), cg.fp12_pow(curve, a, 0x123456789abcdef1 + (5 << 64)))
    np.testing.assert_array_equal(out.reshape(a.shape), T.to_abi(T.pow(T.from_abi(a), 0x123456789abcdef1 + (5 << 64))))
    g1, g2, _ = seeded_points(curve, 1, 5100)
    uP, uQ = off(g1[0]), off(g2[0])
    out = misaligned(E); chk(lib.cg_pairing(curve, ptr(uP), ptr(uQ), ptr(out)))
    np.testing.assert_array_equal(out.reshape(a.shape), orc.pairing(curve, g1[0], g2[0]))
    out = misaligned(E); chk(lib.cg_miller_loop(curve, ptr(uP), ptr(uQ), C.c_size_t(1), ptr(out)))
    np.testing.assert_array_equal(out.reshape(a.shape), cg.miller_loop(curve, g1[0], g2[0]))
