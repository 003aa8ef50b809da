"""Python-integer side of the Plonk witness-check and key-audit tests: the gate residual restated with Python integers over a parsed key,
the rows a changed wire can reach, and a zkey patcher that keeps a mutated polynomial block self-consistent (plonk_setup_tools.poly_block:
the naive DFT is fine at domains 8 and 64).  No tests here."""
import os
import struct

import numpy as np

import oracle_lib as orc
import plonk_setup_tools as pt
import r1cs_tools as rt
from r1cs_tools import CURVES, NO_ROW, R, modulus

# the six shipped Plonk keys with their witnesses
FIXTURES = [("bn254", "kyc"), ("bn254", "multiplier2"), ("bn254", "multiplier2_example"), ("bn254", "sum_arrays"), ("bls12_381", "kyc"), ("bls12_381", "multiplier2")]
SELECTOR_SECTIONS = (7, 8, 9, 10, 11)                     # qm, ql, qr, qo, qc


def plonk_fx(curve_name, circuit, f):
    return os.path.join(rt.GOLDEN, "plonk", curve_name, circuit, f)


def fq_bytes(curve):
    return 48 if curve == orc.BLS12_381 else 32


def ints(curve, data):
    """Montgomery bytes -> Python integers"""
    r = modulus(curve); rinv = pow(R, -1, r)
    return [int.from_bytes(data[o:o + 32], "little") * rinv % r for o in range(0, len(data), 32)]


def rows_of_block(curve, block, n):
    """the values on the n rows of one polynomial block (n coefficients | 4n evaluations): omega4^4 = omega, so row i is evaluation 4 i"""
    ev = block[n * 32:]
    return ints(curve, b"".join(ev[4 * i * 32:4 * i * 32 + 32] for i in range(n)))


class Key:
    """what the witness check and the audit read from a Plonk zkey, as Python integers"""

    def __init__(self, curve, path):
        self.curve, self.path, self.r = curve, path, modulus(curve)
        self.sec = rt.zkey_sections(path)
        self.hdr, self.vk, self.x2 = pt.plonk_header(curve, self.sec[2])
        h = self.hdr
        self.n, self.nc, self.n_public, self.n_vars, self.n_add = h["domain_size"], h["n_constraints"], h["n_public"], h["n_vars"], h["n_additions"]
        s3 = self.sec[3]
        self.adds = [struct.unpack_from("<II", s3, 72 * a) + tuple(ints(curve, s3[72 * a + 8:72 * a + 72])) for a in range(self.n_add)]
        self.maps = [list(struct.unpack_from(f"<{self.nc}I", self.sec[4 + w])) for w in range(3)]
        self.q = [rows_of_block(curve, self.sec[s], self.n) for s in SELECTOR_SECTIONS]

    def wires(self, witness):
        """witness = the n_vars - n_additions integers of the full witness -> the value of every wire: wire 0 is ZERO (the prover forces it,
        types.rs:107-109), the additions extend the witness in their order"""
        assert len(witness) == self.n_vars - self.n_add
        w = [0] + [int(v) % self.r for v in witness[1:]]
        for id1, id2, f1, f2 in self.adds:
            w.append((f1 * w[id1] + f2 * w[id2]) % self.r)
        return w

    def bad_rows(self, witness):
        return residual_rows(self.n, self.nc, self.n_public, self.maps, self.q, self.wires(witness), self.r)

    def holds_by_construction(self, i):
        """rows that hold for EVERY witness on a consistent key: the public-input gate of wire i + 1 (ql w - PI reads the wire on both sides)
        and the gate of an addition (the wire it defines is computed from the very record the gate restates: qo = 1, ql = -f1, qr = -f2)"""
        a, b, c = (self.maps[w][i] for w in range(3))
        sel = tuple(q[i] for q in self.q)
        if i < self.n_public and (a, b, c) == (i + 1, 0, 0) and sel == (0, 1, 0, 0, 0):
            return True
        k = c - (self.n_vars - self.n_add)
        return 0 <= k < self.n_add and self.adds[k][:2] == (a, b) and sel == (0, (-self.adds[k][2]) % self.r, (-self.adds[k][3]) % self.r, 1, 0)

    def reached(self, wire):
        """the rows whose maps name `wire` or an addition fed by it, but for those that hold by construction"""
        hit = {wire}
        base = self.n_vars - self.n_add
        for a, (id1, id2, _, _) in enumerate(self.adds):
            if id1 in hit or id2 in hit:
                hit.add(base + a)
        return [i for i in range(self.nc) if any(self.maps[w][i] in hit for w in range(3)) and not self.holds_by_construction(i)]


def residual_rows(n, nc, n_public, maps, q, w, r):
    """the rows i < n with qm a b + ql a + qr b + qo c + qc - (i < n_public ? w[i + 1] : 0) != 0; a, b, c = w[maps[.][i]] for i < nc, else 0"""
    bad = []
    for i in range(n):
        a, b, c = (w[maps[0][i]], w[maps[1][i]], w[maps[2][i]]) if i < nc else (0, 0, 0)
        res = q[0][i] * a * b + q[1][i] * a + q[2][i] * b + q[3][i] * c + q[4][i] - (w[i + 1] if i < n_public else 0)
        if res % r:
            bad.append(i)
    return bad


def verdict(bad):
    return len(bad), (bad[0] if bad else NO_ROW)


def read_witness(curve, path):
    """(Montgomery limbs for the product, Python integers for the restatement)"""
    w = orc.read_wtns(curve, path)
    return w, rt.from_mont(curve, w)


# ---- the patcher ---------------------------------------------------------------------------------------------------------------------------
def patch_zkey(src, dst, replace):
    """copy a zkey with the sections in `replace` (id -> bytes) swapped in, lengths rewritten, order kept"""
    data = open(src, "rb").read()
    _, ns = struct.unpack_from("<II", data, 4)
    out, off = [data[:12]], 12
    for _ in range(ns):
        i, ln = struct.unpack_from("<IQ", data, off); off += 12
        body = replace.get(i, data[off:off + ln]); off += ln
        out.append(struct.pack("<IQ", i, len(body)) + body)
    with open(dst, "wb") as f:
        f.write(b"".join(out))
    return dst


def block_from_rows(curve, rows):
    """a self-consistent polynomial block (coefficients | 4n evaluations) for the given values on the rows"""
    return pt.poly_block([v % modulus(curve) for v in rows], modulus(curve))[0]


def header_offsets(curve):
    """byte offsets inside section 2: the five numbers, k1, k2, the eight commitments, X_2"""
    fq = fq_bytes(curve)
    numbers = 4 + fq + 4 + 32
    return dict(numbers=numbers, k1=numbers + 20, k2=numbers + 52, vk=numbers + 84, x2=numbers + 84 + 16 * fq)


def splice(data, off, new):
    return data[:off] + new + data[off + len(new):]


def double_point(cg, curve, group, affine_bytes):
    """2 P for a packed affine point, as packed affine bytes: a valid point that differs from P (session open validates the points)"""
    words = len(affine_bytes) // 8
    aff = np.frombuffer(affine_bytes, dtype=np.uint64, count=words).copy()
    two = rt.to_mont(curve, [2])[0]
    out = cg.point_to_affine(curve, group, cg.point_scalar_mul(curve, group, cg.point_from_affine(curve, group, aff), two)).tobytes()
    assert out != affine_bytes and any(out), "the point has order two or is the point at infinity"
    return out
