"""Structured inputs for the MSM's lazy limb arithmetic (test infrastructure; tests/test_lazy_bucket_host.py and tests/test_msm_edges.py).

The bucket accumulation reads a coordinate's Montgomery limbs a < p straight into 9 x 29 / 14 x 28-bit lazy limbs shifted left by SH = 5 / 8
bits (csrc/lazy29.hpp, unpack_small): a quotient estimated from the top limb of 2^SH a brings it into [-p, p).  The values this is tightest
on are the quotient boundaries floor(j p / 2^SH), the values at which that top limb steps, and the powers of two; `edge_points` finds curve
points whose x coordinate sits on them.  Python integers only; the oracle confirms every point is on its curve."""
import numpy as np

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FQ, FR, G1, G2

GROUPS = [(BN254, G1), (BN254, G2), (BLS12_381, G1), (BLS12_381, G2)]      # the order of the four tables in an edge point file


def lazy_shape(p):
    """(limbs, bits per limb, SH) of csrc/lazy29.hpp for a modulus of this size"""
    return (9, 29, 5) if p.bit_length() <= 256 else (14, 28, 8)


def boundary_values(p, js=None):
    """Raw Montgomery-limb values a < p at the edges of unpack_small: 0, 1, 2, p - 1, p - 2; floor(j p / 2^SH) + {-2 .. 2} for j in `js`
    (default: every j in 1 .. 2^SH - 1) and, beside each, the values at which the top limb of 2^SH a steps; 2^k - 1, 2^k, 2^k + 1 for every k."""
    nl, w, sh = lazy_shape(p)
    step = 1 << (w * (nl - 1) - sh)                    # the top limb of 2^SH a is floor(a / step)
    out = [0, 1, 2, p - 1, p - 2]
    for j in (js if js is not None else range(1, 1 << sh)):
        q = j * p >> sh
        out += [q + d for d in range(-2, 3)]
        out += [(q // step + up) * step + d for up in (0, 1) for d in (-1, 0, 1)]
    for k in range(p.bit_length() + 1):
        out += [(1 << k) + d for d in (-1, 0, 1)]
    seen, res = set(), []
    for v in out:
        if 0 <= v < p and v not in seen:
            seen.add(v); res.append(v)
    return res


# a spread of BLS12-381 Fq's 255 quotient boundaries: every fourth one, and the first, middle and last three
BLS_FQ_JS = sorted(set(range(1, 256, 4)) | {1, 2, 3, 127, 128, 129, 253, 254, 255})


def _fp_sqrt(a, p):                                    # both base fields are = 3 mod 4
    s = pow(a, (p + 1) // 4, p)
    return s if s * s % p == a % p else None


def _fp2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def _fp2_sqrt(a, p):
    a0, a1 = a[0] % p, a[1] % p
    if a1 == 0:
        s = _fp_sqrt(a0, p)
        if s is not None: return (s, 0)
        s = _fp_sqrt(-a0 % p, p)
        return (0, s) if s is not None else None
    n = _fp_sqrt((a0 * a0 + a1 * a1) % p, p)
    if n is None: return None
    inv2 = pow(2, -1, p)
    for t in ((a0 + n) * inv2 % p, (a0 - n) * inv2 % p):
        x0 = _fp_sqrt(t, p)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, p) % p)
            if _fp2_mul(x, x, p) == (a0, a1): return x
    return None


def _curve_b(curve, group, p):
    if group == G1:
        return 3 if curve == BN254 else 4
    if curve == BN254:
        inv = pow(82, -1, p)                           # 3 / (9 + u) = 3 (9 - u) / 82
        return (27 * inv % p, -3 * inv % p)
    return (4, 4)


def edge_points(curve, group):
    """(table of packed affine points, the Montgomery-limb values m their x coordinates sit on): for every boundary value m (for G2: m for x.c0
    and another boundary value for x.c1) the nearest m', stepping m by +1, -1, +2, ..., at which x = m' / R gives a square x^3 + b.  The points
    lie on the curve, not necessarily in the prime-order subgroup: the group law the MSM and the oracle share does not care."""
    p = orc.MODULI[(curve, FQ)]
    nq = orc.nlimbs(curve, FQ)
    R = 1 << (64 * nq)
    rinv = pow(R, -1, p)
    b = _curve_b(curve, group, p)
    vals = boundary_values(p, BLS_FQ_JS if curve == BLS12_381 else None)
    limbs = lambda v: orc.int_to_limbs(v % p, nq)
    pts, ms = [], []
    for i, m in enumerate(vals):
        m1 = vals[(7 * i + 3) % len(vals)]                                     # G2: the second component of x
        for k in range(400):
            mm = m + (k + 1) // 2 * (1 if k % 2 else -1)                       # m, m + 1, m - 1, m + 2, ...
            if not 0 <= mm < p: continue
            if group == G1:
                x = mm * rinv % p
                y = _fp_sqrt((x * x * x + b) % p, p)
                if y is None or y == 0: continue
                pts.append(np.concatenate([limbs(mm), limbs(y * R)]))
            else:
                x = (mm * rinv % p, m1 * rinv % p)
                x3 = _fp2_mul(_fp2_mul(x, x, p), x, p)
                y = _fp2_sqrt(((x3[0] + b[0]) % p, (x3[1] + b[1]) % p), p)
                if y is None or y == (0, 0): continue
                pts.append(np.concatenate([limbs(mm), limbs(m1), limbs(y[0] * R), limbs(y[1] * R)]))
            ms.append(mm)
            break
        else:
            raise AssertionError(f"no curve point within 200 of the boundary value {m}")
    pts = np.stack(pts)
    for pt in pts:
        assert orc.on_curve(curve, group, pt)
    return pts, ms


def write_edge_file(path):
    """the four edge tables in GROUPS order, each as a uint64 count followed by the packed points: the argument of tests/sanitize/lazy_bucket_main;
    returns the four counts"""
    counts = []
    with open(path, "wb") as f:
        for curve, group in GROUPS:
            pts, _ = edge_points(curve, group)
            f.write(np.uint64(len(pts)).tobytes()); f.write(np.ascontiguousarray(pts, dtype=np.uint64).tobytes())
            counts.append(len(pts))
    return counts


def neg_points(curve, pts):
    """-P for packed affine points (infinity stays infinity)"""
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    nq = orc.nlimbs(curve, FQ)
    out = pts.copy()
    h = pts.shape[1] // 2
    y = pts[:, h:].reshape(-1, nq)
    out[:, h:] = orc.field_op(curve, FQ, "sub", np.zeros_like(y), y).reshape(pts.shape[0], h)
    return out


def scalars_from_ints(curve, values):
    """Montgomery-form Fr limbs of Python integers (reduced mod r)"""
    r = orc.MODULI[(curve, FR)]
    raw = np.stack([orc.int_to_limbs(int(v) % r, 4) for v in values])
    r2 = orc.from_dec(curve, FR, str(pow(2, 256, r)))                        # Montgomery representative of R: x -> x R
    return orc.field_op(curve, FR, "mul", raw, np.broadcast_to(r2, raw.shape).copy())


def small_scalars(curve, values):
    """the same for an array of integers below 2^63"""
    raw = np.zeros((len(values), 4), dtype=np.uint64); raw[:, 0] = np.asarray(values, dtype=np.uint64)
    r2 = orc.from_dec(curve, FR, str(pow(2, 256, orc.MODULI[(curve, FR)])))
    return orc.field_op(curve, FR, "mul", raw, np.broadcast_to(r2, raw.shape).copy())
