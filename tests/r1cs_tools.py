"""Python-integer side of the R1CS tests: an .r1cs writer and parser, the sections of a zkey, Montgomery conversion, and the
4 099-row circuit whose rows cycle through the lengths at which the check and column-sum kernels take another path."""
import os
import random
import struct

import numpy as np

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = {"bn254": BN254, "bls12_381": BLS12_381}
# (curve, directory under tests/golden/groth16): every (.r1cs, .zkey) pair the reference ships for Groth16
PAIRS = [("bn254", "multiplier2"), ("bn254", "poseidon"), ("bls12_381", "multiplier2"), ("bls12_381", "poseidon"),
         ("bn254", "multiplier2_example"), ("bn254", "sum_arrays"), ("bn254", "poseidon_hash2"), ("bn254", "kyc"), ("bls12_381", "kyc")]
NO_ROW = (1 << 64) - 1
R = 1 << 256


def fx(curve_name, circuit, f):
    return os.path.join(GOLDEN, "groth16", curve_name, circuit, f)


def modulus(curve):
    return orc.MODULI[(curve, FR)]


def to_mont(curve, values):
    """Python integers -> (n, 4) uint64 Montgomery limbs"""
    r = modulus(curve)
    return np.array([[((v % r) * R % r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def from_mont(curve, limbs):
    r = modulus(curve); rinv = pow(R, -1, r)
    return [orc.limbs_to_int(row) * rinv % r for row in np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)]


def lc_bytes(terms):
    return struct.pack("<I", len(terms)) + b"".join(struct.pack("<I", w) + int(v).to_bytes(32, "little") for w, v in terms)


def header_bytes(prime, n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, n_constraints, field_size=32):
    return struct.pack("<I", field_size) + int(prime).to_bytes(field_size, "little") + struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, n_constraints)


def file_bytes(sections, magic=b"r1cs", version=1):
    """sections: list of (id, payload) in file order"""
    return magic + struct.pack("<II", version, len(sections)) + b"".join(struct.pack("<IQ", i, len(p)) + p for i, p in sections)


def write_r1cs(path, prime, n_wires, n_pub_out, n_pub_in, n_prv_in, constraints, before=(), map_section=None):
    """constraints: list of (A, B, C), each a list of (wire, value).  `before`: sections put in front of the header; map_section: the payload of
    section 3 (default: the identity map)."""
    body = b"".join(lc_bytes(a) + lc_bytes(b) + lc_bytes(c) for a, b, c in constraints)
    if map_section is None:
        map_section = b"".join(struct.pack("<Q", i) for i in range(n_wires))
    secs = list(before) + [(1, header_bytes(prime, n_wires, n_pub_out, n_pub_in, n_prv_in, n_wires, len(constraints))), (2, body), (3, map_section)]
    with open(path, "wb") as f:
        f.write(file_bytes(secs))


def parse_r1cs(path):
    """-> dict(n_wires, n_public, n_constraints, prime, constraints=[(A, B, C)]) with Python integers"""
    data = open(path, "rb").read()
    assert data[:4] == b"r1cs"
    _, ns = struct.unpack_from("<II", data, 4)
    off, secs = 12, {}
    for _ in range(ns):
        i, n = struct.unpack_from("<IQ", data, off); off += 12
        secs.setdefault(i, data[off:off + n]); off += n
    h = secs[1]
    fs, = struct.unpack_from("<I", h, 0)
    prime = int.from_bytes(h[4:4 + fs], "little")
    n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, n_con = struct.unpack_from("<IIIIQI", h, 4 + fs)
    body, off, cons = secs[2], 0, []
    for _ in range(n_con):
        lcs = []
        for _ in range(3):
            n, = struct.unpack_from("<I", body, off); off += 4
            lcs.append([(struct.unpack_from("<I", body, off + 36 * t)[0], int.from_bytes(body[off + 36 * t + 4:off + 36 * t + 36], "little")) for t in range(n)])
            off += 36 * n
        cons.append(tuple(lcs))
    return dict(n_wires=n_wires, n_public=n_pub_out + n_pub_in, n_constraints=n_con, prime=prime, constraints=cons)


def evaluate(constraints, w, r):
    """(n_bad, first_bad) of the witness w (Python integers) by Python integers"""
    dot = lambda lc: sum(v * w[i] for i, v in lc) % r
    bad = [i for i, (a, b, c) in enumerate(constraints) if dot(a) * dot(b) % r != dot(c)]
    return len(bad), (bad[0] if bad else NO_ROW)


def zkey_sections(path):
    data = open(path, "rb").read()
    assert data[:4] == b"zkey"
    _, ns = struct.unpack_from("<II", data, 4)
    off, secs = 12, {}
    for _ in range(ns):
        i, n = struct.unpack_from("<IQ", data, off); off += 12
        secs[i] = data[off:off + n]; off += n
    return secs


def zkey_header_numbers(curve, secs):
    """n_vars, n_public, domain_size from section 2"""
    fq = 48 if curve == BLS12_381 else 32
    return struct.unpack_from("<III", secs[2], 4 + fq + 4 + 32)


# ---- the 4 099-row circuit ---------------------------------------------------------------------------------------------------------------
ROWS, BASE = 4099, 200
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 130)


def skewed_circuit(curve, seed=5):
    """-> (n_wires, constraints, witness).  Wires: 0 = one, 1 .. BASE random values, then one output wire per row.  Row i: A_i and C_i have
    LENGTHS[(i + 1) % 8] terms, B_i LENGTHS[(i + 5) % 8] plus a leading term on wire 0 in every third row (so every length occurs in each
    matrix, the empty combination and combinations longer than one and two waves included, and wire 0's column of B has 1 367 entries).  The
    last term of a non-empty C_i is the row's output wire, whose value is solved for; an empty C_i goes with an empty A_i.  The output wires of
    the 512 rows with an empty C_i occur nowhere.  Coefficients cycle through 1, r - 1 and random values."""
    r = modulus(curve)
    rnd = random.Random(seed * 2 + curve)
    n_wires = 1 + BASE + ROWS
    w = [1] + [rnd.randrange(1, r) for _ in range(BASE)] + [0] * ROWS
    tick = [0]

    def coef():
        tick[0] += 1
        return (1, r - 1, rnd.randrange(1, r))[tick[0] % 3]

    def lc(n):
        return [(wire, coef()) for wire in rnd.sample(range(1, BASE + 1), n)]
    dot = lambda terms: sum(v * w[i] for i, v in terms) % r
    cons = []
    for i in range(ROWS):
        la = LENGTHS[(i + 1) % 8]
        a = lc(la)
        b = ([(0, coef())] if i % 3 == 0 else []) + lc(LENGTHS[(i + 5) % 8])
        c = []
        if la:
            c = lc(la - 1)
            k, out = coef(), 1 + BASE + i
            w[out] = (dot(a) * dot(b) - dot(c)) * pow(k, -1, r) % r
            c.append((out, k))
        cons.append((a, b, c))
    return n_wires, cons, w


def columns(constraints, m, n_wires):
    """column-major form of matrix m (0, 1, 2): col_ptr, rows, values (rows ascending inside a column)"""
    cols = [[] for _ in range(n_wires)]
    for j, con in enumerate(constraints):
        for wire, v in con[m]:
            cols[wire].append((j, v))
    col_ptr = np.zeros(n_wires + 1, dtype=np.uint32)
    col_ptr[1:] = np.cumsum([len(c) for c in cols])
    rows = np.array([j for c in cols for j, _ in c], dtype=np.uint32)
    vals = [v for c in cols for _, v in c]
    return cols, col_ptr, rows, vals
