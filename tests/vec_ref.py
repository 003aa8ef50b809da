"""Python-integer references for the vector kernels (csrc/vec_kernels.hpp): Montgomery representatives (x R mod r, R = 2^256) as Python
integers, the limb conversions both ways, and the constraint evaluation of rep3.rs:690-708 / plain.rs:243-258 on them.  No GPU, no oracle
arithmetic: what a test compares a kernel with here is integer arithmetic modulo r and nothing else."""
import numpy as np

import oracle_lib as orc
from oracle_lib import FR


def to_ints(a):
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


def from_ints(v):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in v), dtype=np.uint64).reshape(-1, 4).copy()


class Mont:
    """Montgomery representatives (x R mod r, R = 2^256) as Python integers"""

    def __init__(self, curve):
        self.r = orc.MODULI[(curve, FR)]; self.R = (1 << 256) % self.r; self.Rinv = pow(self.R, -1, self.r)

    def mul(self, a, b): return a * b * self.Rinv % self.r
    def of(self, x): return x * self.R % self.r

    def inv(self, a):
        """the representative of x^-1 from the representative a = x R of x: x^-1 R = a^-1 R^2"""
        return pow(a, -1, self.r) * self.R * self.R % self.r

    def prod(self, reps):
        """the representative of the product of the values whose representatives are `reps` (a running product, one R^-1 per factor after the first)"""
        acc, k = self.R, 0
        for a in reps: acc = acc * a % self.r; k += 1
        return acc * pow(self.Rinv, k, self.r) % self.r


def spmv_ints(F, row_ptr, col, coeff, pub, party, wa, wb):
    """evaluate_constraint over every row of a CSR matrix (rep3.rs:690-708 / plain.rs:243-258) on representatives: a signal below len(pub) is
    public (rep3.rs:600-608: its term goes to component a for party 0 and the single-component driver -1, to component b for party 1, nowhere
    for party 2), any other is the shared witness at index - len(pub), added to both components.  wb = None: component b stays zero."""
    n_rows, ninp = len(row_ptr) - 1, len(pub)
    out_a, out_b = [0] * n_rows, [0] * n_rows
    for r in range(n_rows):
        a = b = 0
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            idx, c = int(col[k]), coeff[k]
            if idx < ninp:
                t = F.mul(c, pub[idx])
                if party <= 0: a += t
                elif party == 1: b += t
            else:
                a += F.mul(c, wa[idx - ninp])
                if wb is not None: b += F.mul(c, wb[idx - ninp])
        out_a[r], out_b[r] = a % F.r, b % F.r
    return out_a, out_b
