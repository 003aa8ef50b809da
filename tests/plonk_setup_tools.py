"""Python-integer side of the Plonk setup tests: snarkjs' R1CS -> Plonk gate compiler restated with Python integers, the sections of
the key it determines, and the circuit that takes every branch of the compiler.

The compiler (confirmed byte for byte against the four shipped (.r1cs, Plonk .zkey) pairs by test_plonk_setup.py):
  * a combination is a map wire -> coefficient walked by ascending wire; a wire named twice has its coefficients summed, zeros are dropped,
    wire 0 is the constant;
  * reduce(terms, maxC) shortens a combination of t > maxC terms by a = t - maxC additions, each of which joins the two oldest entries of a
    queue into a new wire pushed at its end: in closed form addition j reads elem(2j), elem(2j + 1) with elem(e) = term e for e < t and
    (base + e - t, 1) otherwise, and elem(2a) .. elem(t + a - 1) are left;
  * rows: public-input gates, then per R1CS row the additions of its combinations and one sum or multiplication gate."""
import random
import struct

import r1cs_tools as rt
from r1cs_tools import modulus

R = 1 << 256
# every (.r1cs under golden/groth16, Plonk .zkey under golden/plonk) pair of one circuit
PAIRS = [("bn254", "multiplier2_example"), ("bn254", "sum_arrays"), ("bn254", "kyc"), ("bls12_381", "kyc")]
POSEIDON = [("bn254", "poseidon"), ("bls12_381", "poseidon"), ("bn254", "poseidon_hash2")]


def canonical(lc, r):
    """[(wire, value)] in any order -> (constant, [(wire, coefficient)] ascending, nonzero)"""
    d = {}
    for w, v in lc:
        d[w] = (d.get(w, 0) + v) % r
    k = d.pop(0, 0)
    return k, [(w, d[w]) for w in sorted(d) if d[w]]


def lc_type(k, terms):
    return "n" if terms else ("k" if k else "0")


def reduce_lc(terms, max_c, base, r, out):
    """appends the additions of one combination to out["adds"] and their gates to out["gates"]; -> (what is left, padded to max_c; additions made)"""
    t = len(terms)
    a = t - max_c if t > max_c else 0
    elem = lambda e: terms[e] if e < t else (base + e - t, 1)
    for j in range(a):
        (sl, cl), (sr, cr) = elem(2 * j), elem(2 * j + 1)
        out["adds"].append((sl, sr, cl, cr))
        out["gates"].append(((sl, sr, base + j), (0, (r - cl) % r, (r - cr) % r, 1, 0)))
    left = [elem(e) for e in range(2 * a, t + a)]
    return left + [(0, 0)] * (max_c - len(left)), a


def compile_gates(n_wires, n_public, constraints, r):
    """-> dict(adds=[(id1, id2, f1, f2)], gates=[((a, b, c), (qm, ql, qr, qo, qc))], row_adds=[additions per R1CS row], n_vars, n_constraints, n)"""
    out = dict(adds=[], gates=[], row_adds=[])
    for s in range(1, n_public + 1):
        out["gates"].append(((s, 0, 0), (0, 1, 0, 0, 0)))
    nxt = n_wires

    def sum_gate(k, terms):
        nonlocal nxt
        left, a = reduce_lc(terms, 3, nxt, r, out)
        nxt += a
        out["gates"].append((tuple(w for w, _ in left), (0, left[0][1], left[1][1], left[2][1], k)))

    def joined(k, lc_b, lc_c):            # k * B - C
        kb, tb = lc_b
        kc, tc = lc_c
        d = {}
        for w, v in tb:
            d[w] = k * v % r
        for w, v in tc:
            d[w] = (d.get(w, 0) - v) % r
        return (k * kb - kc) % r, [(w, d[w]) for w in sorted(d) if d[w]]

    for A, B, Cc in constraints:
        a, b, c = canonical(A, r), canonical(B, r), canonical(Cc, r)
        ta, tb = lc_type(*a), lc_type(*b)
        before = nxt
        if ta == "0" or tb == "0":
            sum_gate(*c)
        elif ta == "k":
            sum_gate(*joined(a[0], b, c))
        elif tb == "k":
            sum_gate(*joined(b[0], a, c))
        else:
            left = []
            for k, terms in (a, b, c):
                l, n_add = reduce_lc(terms, 1, nxt, r, out)
                nxt += n_add
                left.append(l[0])
            (sa, ca), (sb, cb), (sc, cc) = left
            out["gates"].append(((sa, sb, sc), (ca * cb % r, ca * b[0] % r, a[0] * cb % r, (r - cc) % r, (a[0] * b[0] - c[0]) % r)))
        out["row_adds"].append(nxt - before)
    out["n_vars"] = nxt
    out["n_constraints"] = len(out["gates"])
    n = 8
    while n < out["n_constraints"]:
        n *= 2
    out["n"] = n
    return out


def snarkjs_roots(r):
    """roots[i] = a primitive 2^i-th root of unity as snarkjs derives them (smallest quadratic non-residue from 2)"""
    s, t = 0, r - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    nqr = 2
    while pow(nqr, (r - 1) // 2, r) == 1:
        nqr += 1
    roots = [0] * (s + 1)
    roots[s] = pow(nqr, t, r)
    for i in range(s - 1, -1, -1):
        roots[i] = roots[i + 1] * roots[i + 1] % r
    return roots


def coset_shifts(n, r):
    k1 = 2
    while pow(k1, n, r) == 1:
        k1 += 1
    k2 = 3
    while pow(k2, n, r) == 1 or pow(k2 * pow(k1, -1, r) % r, n, r) == 1:
        k2 += 1
    return k1, k2


def sigma_rows(g, r):
    """three lists of n labels: sigma[p] = the label of the previous position of the same wire, walking rows then columns; rows past the
    gates carry wire 0 in all three columns"""
    n, nc = g["n"], g["n_constraints"]
    k1, k2 = coset_shifts(n, r)
    omega = snarkjs_roots(r)[n.bit_length() - 1]
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * omega % r
    label = lambda p: (1, k1, k2)[p // n] * wp[p % n] % r
    prev = sigma_prev(g)
    return [[label(prev[w * n + i]) for i in range(n)] for w in range(3)]


def sigma_prev(g):
    n, nc = g["n"], g["n_constraints"]
    last, first, prev = {}, {}, [0] * (3 * n)
    for i in range(n):
        for w in range(3):
            s = g["gates"][i][0][w] if i < nc else 0
            p = w * n + i
            if s in last:
                prev[p] = last[s]
            else:
                first[s] = p
            last[s] = p
    for s, p in first.items():
        prev[p] = last[s]
    return prev


def dft_naive(values, root, r):
    n = len(values)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * root % r
    return [sum(v * pw[i * j % n] for j, v in enumerate(values) if v) % r for i in range(n)]


def mont_bytes(values, r):
    return b"".join((v % r * R % r).to_bytes(32, "little") for v in values)


def poly_block(rows, r):
    """iNTT_n(rows) | NTT_4n(zero-padded coefficients), Montgomery bytes; also the coefficients as integers"""
    n = len(rows)
    roots = snarkjs_roots(r)
    omega, omega4 = roots[n.bit_length() - 1], roots[n.bit_length() + 1]
    n_inv = pow(n, -1, r)
    coef = [v * n_inv % r for v in dft_naive(rows, pow(omega, -1, r), r)]
    ev = dft_naive(coef + [0] * (3 * n), omega4, r)
    return mont_bytes(coef, r) + mont_bytes(ev, r), coef


def key_sections(n_wires, n_public, constraints, r, polys=True):
    """-> (header numbers dict, {section id: bytes} for 3 .. 13 (3 .. 6 only with polys=False), the compiled gates)"""
    g = compile_gates(n_wires, n_public, constraints, r)
    n, nc = g["n"], g["n_constraints"]
    k1, k2 = coset_shifts(n, r)
    hdr = dict(n_vars=g["n_vars"], n_public=n_public, domain_size=n, n_additions=len(g["adds"]), n_constraints=nc, k1=k1, k2=k2)
    sec = {3: b"".join(struct.pack("<II", a, b) + mont_bytes([f1, f2], r) for a, b, f1, f2 in g["adds"])}
    for w in range(3):
        sec[4 + w] = b"".join(struct.pack("<I", gate[0][w]) for gate in g["gates"])
    if polys:
        for i in range(5):
            sec[7 + i] = poly_block([gate[1][i] for gate in g["gates"]] + [0] * (n - nc), r)[0]
        sec[12] = b"".join(poly_block(rows, r)[0] for rows in sigma_rows(g, r))
        sec[13] = b"".join(poly_block([int(i == j) for i in range(n)], r)[0] for j in range(n_public))
    return hdr, sec, g


def plonk_header(curve, sec2):
    """section 2 of a Plonk zkey -> (numbers dict with k1, k2 as integers, the bytes of the eight commitments, the bytes of X_2)"""
    fq = 48 if curve == rt.BLS12_381 else 32
    r = modulus(curve)
    off = 4 + fq + 4 + 32
    n_vars, n_public, n, n_add, nc = struct.unpack_from("<IIIII", sec2, off)
    off += 20
    rinv = pow(R, -1, r)
    k1, k2 = (int.from_bytes(sec2[off + 32 * i:off + 32 * i + 32], "little") * rinv % r for i in range(2))
    off += 64
    assert len(sec2) == off + 8 * 2 * fq + 4 * fq
    return (dict(n_vars=n_vars, n_public=n_public, domain_size=n, n_additions=n_add, n_constraints=nc, k1=k1, k2=k2),
            sec2[off:off + 16 * fq], sec2[off + 16 * fq:])


# ---- the circuit that takes every branch -------------------------------------------------------------------------------------------------
BRANCH_ROWS, BRANCH_BASE, BRANCH_PUBLIC = 4100, 200, 3
MUL_LENGTHS = (1, 2, 3, 64, 65, 130)


def branch_circuit(curve, seed=11):
    """-> (n_wires, n_public, constraints, witness as integers).  Wires: 0 = one, 1 .. BRANCH_BASE random values (the first BRANCH_PUBLIC
    public), then one output wire per row, which is the last (highest) wire of the row's C and is solved for.  Row i takes kind i % 16:
      0 .. 5   multiplication rows: A, B, C of MUL_LENGTHS[(k + 0, 2, 4) % 6] terms, constants on A (bit 0 of i // 16), B (bit 1), C (bit 2)
      6        A of type "0" (empty), C one term: the output wire must be 0
      7        B of type "0" (one term with coefficient 0), C two terms
      8        A of type "k", B and C share a wire whose terms cancel in k * B - C
      9        B of type "k": the joined row is left with (i // 16) % 6 = 0 .. 5 terms (0: C is k_B * k_A, constants only)
      10       A of type "k" and B of type "k", C one term plus a constant
      11       multiplication row whose C is a constant only (A, B one term each on values chosen to satisfy it: A = wire, B = its inverse)
      12       multiplication row with A written in descending wire order, B naming one wire twice
      13       A of type "k" with a 4-term B, 14: B of type "k" with a wire named twice in A whose coefficients cancel
      15       multiplication row
    To keep the domain at 2^15 the long combinations come in every 16th repetition of kinds 0 .. 5 and 13 (64-term B) and in every 8th of
    kind 15 (65-term A and B), the others are cut to at most 3, 4 and 2 terms: rows 2 047 and 4 095 (kind 15) make 128 additions, rows
    2 048 and 4 096 (kind 0) 64, so the counts on either side of both 2 048-row scan tile edges are large and uneven."""
    r = modulus(curve)
    rnd = random.Random(seed * 2 + curve)
    n_wires = 1 + BRANCH_BASE + BRANCH_ROWS
    w = [1] + [rnd.randrange(1, r) for _ in range(BRANCH_BASE)] + [0] * BRANCH_ROWS
    inv_of = {}                                                                  # kind 11: pairs (wire, wire holding its inverse)
    for j in range(1, BRANCH_BASE, 2):
        if j > BRANCH_PUBLIC and j + 1 <= BRANCH_BASE:
            w[j + 1] = pow(w[j], -1, r)
            inv_of[j] = j + 1
    inv_wires = sorted(inv_of)
    tick = [0]

    def coef():
        tick[0] += 1
        return (1, r - 1, rnd.randrange(1, r))[tick[0] % 3]

    def lc(n):
        return [(wire, coef()) for wire in sorted(rnd.sample(range(1, BRANCH_BASE + 1), n))]
    dot = lambda terms: sum(v * w[i] for i, v in terms) % r
    cons = []
    for i in range(BRANCH_ROWS):
        kind, rep = i % 16, i // 16
        out = 1 + BRANCH_BASE + i
        solve = True
        if kind < 6 or kind == 15:
            la, lb, lcn = (65, 65, 2) if kind == 15 else (MUL_LENGTHS[kind], MUL_LENGTHS[(kind + 2) % 6], MUL_LENGTHS[(kind + 4) % 6])
            if (kind == 15 and rep % 8 != 7) or (kind < 6 and rep % 16):
                la, lb, lcn = min(la, 3), min(lb, 4), min(lcn, 2)
            a, b, c = lc(la), lc(lb), lc(lcn - 1)
            if rep & 1: a = [(0, coef())] + a
            if rep & 2: b = b + [(0, coef())]
            if rep & 4: c = [(0, coef())] + c
        elif kind == 6:
            a, b, c = [], lc(2), []
        elif kind == 7:
            a, b, c = lc(3), [(5, 0)], lc(1)
        elif kind == 8:
            b = lc(4); k = coef()
            a = [(0, k)]
            c = [(b[1][0], k * b[1][1] % r)]
        elif kind == 9:
            left = rep % 6
            kb, ka = coef(), coef()
            b = [(0, kb)]
            if left == 0:
                a, c, solve = [(0, ka)], [(0, ka * kb % r)], False
            else:
                a, c = lc(left - 1) + [(0, ka)], []
        elif kind == 10:
            a, b, c = [(0, coef())], [(0, coef())], [(0, coef())]
        elif kind == 11:
            j = inv_wires[rep % len(inv_wires)]; ca, cb = coef(), coef()
            a, b, c, solve = [(j, ca)], [(inv_of[j], cb)], [(0, ca * cb % r)], False
        elif kind == 12:
            a = lc(3)[::-1]
            b = lc(3); b = b + [(b[0][0], coef())]
            c = lc(2)
        elif kind == 13:
            a, b, c = [(0, coef())], lc(4 if rep % 16 else 64), lc(1)
        else:
            t = lc(3)
            a = t + [(t[1][0], (r - t[1][1]) % r)]
            b, c = [(0, coef())], []
        if solve:
            k = coef()
            w[out] = (dot(a) * dot(b) - dot(c)) * pow(k, -1, r) % r
            c = c + [(out, k)]
        cons.append((a, b, c))
    return n_wires, BRANCH_PUBLIC, cons, w


def chain_circuit(curve, n_public, rows, seed=3):
    """`rows` multiplication rows w[i] * w[i + 1] = w[i + 2] over rows + 2 wires (no additions): nConstraints = n_public + rows"""
    r = modulus(curve)
    rnd = random.Random(seed)
    w = [1, rnd.randrange(2, r), rnd.randrange(2, r)]
    cons = []
    for i in range(rows):
        w.append(w[i + 1] * w[i + 2] % r)
        cons.append(([(i + 1, 1)], [(i + 2, 1)], [(i + 3, 1)]))
    return len(w), n_public, cons, w
