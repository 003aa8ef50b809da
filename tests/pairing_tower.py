"""The pairing's target field and twist in plain Python integers: the reference tests/test_pairing_pieces_host.py and
tests/test_pairing_batches.py compare csrc/pairing.hpp with.  Written from the definitions in that header's comment and the curves' public
parameters; no numpy arithmetic, nothing of the product, and no structure shared with it: products are schoolbook, the final exponentiation
is ONE power by c (p^12 - 1) / r (no easy / hard split, no Frobenius, no inverse).
  Fp2  = Fp[u] / (u^2 + 1)                       a pair (c0, c1) of ints in [0, p)
  Fp12 = Fp2[w] / (w^6 - xi)                     a tuple of six Fp2, the coefficients of w^0 .. w^5
  xi   = 9 + u (BN254), 1 + u (BLS12-381)
  ABI  : (2, 3, 2, limbs) u64, [i][j][k] = c[2 j + i].c_k, little-endian Montgomery limbs (R = 2^(64 limbs))
tests/test_pairing_pieces_host.py pins this module to the oracle's pairing values before anything is compared with it."""
import random

import numpy as np

BN254, BLS12_381 = 0, 1


class Tower:
    def __init__(self, curve):
        self.curve = curve
        if curve == BN254:
            x = 4965661367192848881
            self.p = 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1
            self.r = 36 * x**4 + 36 * x**3 + 18 * x**2 + 6 * x + 1
            self.xi = (9, 1)
            self.limbs = 4
            self.conv = 2 * x * (6 * x * x + 3 * x + 1)          # the convention's factor on the final exponent (pairing.hpp)
            self.twist_d = True
        else:
            x = -0xd201000000010000
            self.r = x**4 - x**2 + 1
            assert (x - 1) ** 2 * self.r % 3 == 0
            self.p = (x - 1) ** 2 * self.r // 3 + x
            self.xi = (1, 1)
            self.limbs = 6
            self.conv = 3
            self.twist_d = False
        self.x = x
        p = self.p
        assert p % 4 == 3 and (p**12 - 1) % self.r == 0 and (p * p - 1) % 6 == 0
        self.R = 1 << (64 * self.limbs)
        self.Rinv = pow(self.R, -1, p)
        self.final_exponent = self.conv * ((p**12 - 1) // self.r)
        # the twist y^2 = x^3 + b': b / xi (D-type, b = 3) or b xi (M-type, b = 4)
        self.b_twist = self.f2_mul((3, 0), self.f2_inv(self.xi)) if self.twist_d else self.f2_mul((4, 0), self.xi)
        self.zero2, self.one2 = (0, 0), (1, 0)
        self.zero = (self.zero2,) * 6
        self.one = (self.one2,) + (self.zero2,) * 5

    # ---- Fp2 ----
    def f2_add(self, a, b): return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)
    def f2_sub(self, a, b): return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)
    def f2_neg(self, a): return (-a[0] % self.p, -a[1] % self.p)
    def f2_mul(self, a, b): return ((a[0] * b[0] - a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)
    def f2_scale(self, a, s): return (a[0] * s % self.p, a[1] * s % self.p)
    def f2_conj(self, a): return (a[0], -a[1] % self.p)

    def f2_inv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.p)
        return (a[0] * n % self.p, -a[1] * n % self.p)

    def f2_pow(self, a, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = self.f2_mul(r, r)
            if bit == "1":
                r = self.f2_mul(r, a)
        return r

    # ---- Fp12: schoolbook over w, w^6 = xi ----
    def mul(self, a, b):
        p = self.p
        lo0 = [0] * 11; lo1 = [0] * 11                      # unreduced coefficients of w^0 .. w^10
        for i in range(6):
            a0, a1 = a[i]
            if a0 == 0 and a1 == 0:
                continue
            for j in range(6):
                b0, b1 = b[j]
                lo0[i + j] += a0 * b0 - a1 * b1
                lo1[i + j] += a0 * b1 + a1 * b0
        x0, x1 = self.xi
        out = []
        for k in range(6):
            c0, c1 = lo0[k], lo1[k]
            if k < 5:
                h0, h1 = lo0[k + 6], lo1[k + 6]
                c0 += x0 * h0 - x1 * h1
                c1 += x0 * h1 + x1 * h0
            out.append((c0 % p, c1 % p))
        return tuple(out)

    def pow(self, a, e):
        assert e >= 0
        r = self.one
        for bit in bin(e)[2:]:
            r = self.mul(r, r)
            if bit == "1":
                r = self.mul(r, a)
        return r

    def conj(self, a):
        """conjugation over Fp6: w -> -w"""
        return tuple(c if k % 2 == 0 else self.f2_neg(c) for k, c in enumerate(a))

    def neg(self, a): return tuple(self.f2_neg(c) for c in a)

    def final_exp(self, a):
        """a^(c (p^12 - 1) / r) as one plain power; 0 stays 0"""
        return self.pow(a, self.final_exponent)

    def gamma(self):
        """xi^((p^2 - 1) / 6): w^(p^2) = gamma w; it lies in Fp"""
        g = self.f2_pow(self.xi, (self.p * self.p - 1) // 6)
        assert g[1] == 0
        return g[0]

    def line_dense(self, a0, a1, a3):
        """the sparse line of pairing.hpp as a full element: a0 + a1 w + a3 w^3 (D-type), a0 + a3 w^3 + a1 w^5 (M-type)"""
        z = self.zero2
        return (a0, a1, z, a3, z, z) if self.twist_d else (a0, z, z, a3, z, a1)

    # ---- Montgomery limbs and the ABI layout ----
    def fp_to_limbs(self, v):
        m = v * self.R % self.p
        return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(self.limbs)]

    def fp_from_limbs(self, l):
        raw = sum(int(v) << (64 * i) for i, v in enumerate(l))
        assert raw < self.p, "limbs are not a reduced residue"
        return raw * self.Rinv % self.p

    def f2_to_words(self, a): return self.fp_to_limbs(a[0]) + self.fp_to_limbs(a[1])
    def f2_from_words(self, w): return (self.fp_from_limbs(w[: self.limbs]), self.fp_from_limbs(w[self.limbs: 2 * self.limbs]))

    def to_words(self, a):
        """the 12 x limbs words of an element in the ABI's order"""
        out = []
        for i in range(2):
            for j in range(3):
                out += self.f2_to_words(a[2 * j + i])
        return out

    def from_words(self, w):
        n = 2 * self.limbs
        assert len(w) == 6 * n
        c = [None] * 6
        for i in range(2):
            for j in range(3):
                at = (3 * i + j) * n
                c[2 * j + i] = self.f2_from_words(w[at: at + n])
        return tuple(c)

    def to_abi(self, a): return np.array(self.to_words(a), dtype=np.uint64).reshape(2, 3, 2, self.limbs)
    def from_abi(self, arr): return self.from_words([int(v) for v in np.asarray(arr, dtype=np.uint64).reshape(-1)])

    # ---- affine points of the twist E': y^2 = x^3 + b' over Fp2 (None = infinity) ----
    def on_twist(self, pt):
        x, y = pt
        return self.f2_mul(y, y) == self.f2_add(self.f2_mul(self.f2_mul(x, x), x), self.b_twist)

    def twist_double(self, pt):
        """(2 T, lambda) for the tangent's slope lambda"""
        x, y = pt
        lam = self.f2_mul(self.f2_scale(self.f2_mul(x, x), 3), self.f2_inv(self.f2_scale(y, 2)))
        x3 = self.f2_sub(self.f2_mul(lam, lam), self.f2_scale(x, 2))
        return (x3, self.f2_sub(self.f2_mul(lam, self.f2_sub(x, x3)), y)), lam

    def twist_add(self, t, r):
        """(T + R, lambda) for the chord's slope; T != +-R"""
        assert t[0] != r[0]
        lam = self.f2_mul(self.f2_sub(r[1], t[1]), self.f2_inv(self.f2_sub(r[0], t[0])))
        x3 = self.f2_sub(self.f2_sub(self.f2_mul(lam, lam), t[0]), r[0])
        return (x3, self.f2_sub(self.f2_mul(lam, self.f2_sub(t[0], x3)), t[1])), lam

    def twist_mul(self, pt, m):
        """m T for a small positive m, by doubling and adding"""
        assert m >= 1
        acc = None
        for bit in bin(m)[2:]:
            if acc is not None:
                acc = self.twist_double(acc)[0]
            if bit == "1":
                acc = pt if acc is None else self.twist_add(acc, pt)[0]
        return acc

    def jacobian_to_affine(self, X, Y, Z):
        zi = self.f2_inv(Z); zi2 = self.f2_mul(zi, zi)
        return (self.f2_mul(X, zi2), self.f2_mul(Y, self.f2_mul(zi2, zi)))


    # ---- the arbitrary (non-Miller) elements the final exponentiation is tested on ----
    def random_fp2(self, rng): return (rng.randrange(self.p), rng.randrange(self.p))
    def random_element(self, rng): return tuple(self.random_fp2(rng) for _ in range(6))

    def special_elements(self):
        """name -> element: what a Miller loop never produces.  `all_pm1` has every coordinate's Montgomery limbs equal to p - 1."""
        rng = random.Random(4100 + self.curve)
        z, p = self.zero2, self.p
        pm1 = (p - 1) * self.Rinv % p                                       # the value whose limbs are p - 1
        a, b, c = self.random_fp2(rng), self.random_fp2(rng), self.random_fp2(rng)
        return {
            "zero": self.zero,
            "one": self.one,
            "minus_one": self.neg(self.one),
            "fp6": (self.random_fp2(rng), z, self.random_fp2(rng), z, self.random_fp2(rng), z),      # the Fp6 subfield: (p^6 - 1) kills it
            "all_pm1": ((pm1, pm1),) * 6,
            "all_minus_one": ((p - 1, p - 1),) * 6,
            "line": self.line_dense(a, b, c),
            "pure_odd": (z, self.random_fp2(rng), z, self.random_fp2(rng), z, self.random_fp2(rng)),
            "dense": self.random_element(rng),
        }


_towers = {}


def tower(curve):
    if curve not in _towers:
        _towers[curve] = Tower(curve)
    return _towers[curve]
