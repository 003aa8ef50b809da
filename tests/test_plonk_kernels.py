"""co-plonk's eight fused kernels (csrc/plonk_kernels.hpp), each called alone through its Context wrapper (cg_plonk_additions_dev,
cg_plonk_r2_factors_dev, cg_plonk_r3_blind_dev, cg_plonk_r3_perm_dev, cg_plonk_r3_gate_dev, cg_plonk_mul4_tail_dev, cg_plonk_r3_t_dev,
cg_plonk_r3_divide_dev) and compared bit for bit with the formula of its header comment, evaluated with the oracle's field add / sub / mul
and NumPy indexing only (no round function of oracle/plonk.hpp, no product code).

Every case: both scalar fields; n in {1, 5, 257, 4099} (5 and 4099 leave every residue of i & 3 and a ragged tail); k in {1, 2} share
components with every legal public component; every input vector and constant a distinct random value, with 0, 1 and p - 1 rotated through
the leading lanes of every operand; every output its own buffer filled with a sentinel; for k == 1 the second table entries are NULL and a
spare buffer per output, never passed, keeps its sentinel.  Constants all 0, all 1 and all p - 1 at n = 5.  One case per kernel at
n = 2^19 + 259 on BN254 wraps the grid-stride loop (the grid is capped at 2048 blocks of 256 lanes): its inputs are one 4099-element random
block, rolled by a different amount per input and tiled."""
import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR
from product import cg, ensure_built

pytestmark = pytest.mark.gpu

BLOCK = 4099
WRAP = 524288 + 259                      # GRID_CAP * 256 lanes + a ragged rest
SIZES = (1, 5, 257, BLOCK)
KPC = ((1, -1), (1, 0), (2, -1), (2, 0), (2, 1))
CURVE_ID = {BN254: "bn254", BLS12_381: "bls12_381"}


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def cases(with_pc, const_modes=("zero", "one", "pm1")):
    """(curve, n, k, pc, consts) of one kernel; kernels without a public component take pc = -1"""
    out = []
    for curve in (BN254, BLS12_381):
        for n in SIZES:
            for k, pc in (KPC if with_pc else ((1, -1), (2, -1))):
                out.append((curve, n, k, pc, "random"))
        for mode in const_modes:
            out.append((curve, 5, 2, 1 if with_pc else -1, mode))
    out.append((BN254, WRAP, 2, 1 if with_pc else -1, "random"))
    return [pytest.param(*c, id=f"{CURVE_ID[c[0]]}-n{c[1]}-k{c[2]}-pc{c[3]}-{c[4]}") for c in out]


class Field:
    """the oracle's vector add / sub / mul with NumPy broadcasting of constants"""
    _made = {}

    def __new__(cls, curve):
        if curve not in cls._made:
            f = super().__new__(cls)
            f.curve, f.p = curve, orc.MODULI[(curve, FR)]
            f.zero, f.one, f.pm1 = np.zeros(4, dtype=np.uint64), orc.from_dec(curve, FR, 1), orc.from_dec(curve, FR, orc.MODULI[(curve, FR)] - 1)
            cls._made[curve] = f
        return cls._made[curve]

    def _op(self, op, a, b):
        a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
        shape = np.broadcast_shapes(a.shape, b.shape)
        return orc.field_op(self.curve, FR, op, np.broadcast_to(a, shape), np.broadcast_to(b, shape))

    def add(self, a, b): return self._op("add", a, b)
    def sub(self, a, b): return self._op("sub", a, b)
    def mul(self, a, b): return self._op("mul", a, b)

    def sum(self, *xs):
        acc = xs[0]
        for x in xs[1:]: acc = self.add(acc, x)
        return acc


class Case:
    """inputs, sentinel-filled outputs and device buffers of one call; frees the buffers at the end"""
    MODES = ("random", "zero", "one", "pm1")

    def __init__(self, ctx, kernel, curve, n, k, pc, consts="random"):
        self.ctx, self.curve, self.n, self.k, self.pc, self.mode = ctx, curve, n, k, pc, consts
        self.F = Field(curve)
        self.rng = np.random.default_rng([kernel, curve, n, k, pc + 1, self.MODES.index(consts)])
        self.big = n > BLOCK
        self.block = orc.random_field(curve, FR, BLOCK, self.rng) if self.big else None
        self.nvec, self.nout, self.salt = 0, 0, 2 * k + pc + 1
        self.bufs, self.sentinels, self.spares = [], {}, []

    def __enter__(self): return self

    def __exit__(self, *exc):
        self.ctx.free_many(self.bufs)
        return False

    # ---- host inputs
    def vec(self, length, stride=1, blocks=1, edges=True):
        """one input vector, different from every other one.  Small cases: uniform random, with 0, 1, p - 1 in the first lanes that are read
        (lane i at i * stride, of each of `blocks` equal parts), rotated by the vector's number.  The wrap case: the shared block rolled and tiled."""
        v = self.nvec; self.nvec += 1
        if self.big:
            return np.tile(np.roll(self.block, 1 + 37 * v, axis=0), (-(-length // BLOCK), 1))[:length].copy()
        a = orc.random_field(self.curve, FR, length, self.rng)
        if edges:
            part = length // blocks
            for b in range(blocks):
                for i in range(min(-(-part // stride), 4)):
                    e = (i + v + b + self.salt) % 4
                    if e < 3: a[b * part + i * stride] = (self.F.zero, self.F.one, self.F.pm1)[e]
        return a

    def shares(self, length, **kw):
        return [self.vec(length, **kw) for _ in range(self.k)]

    def consts(self, m):
        if self.mode == "random": return orc.random_field(self.curve, FR, m, self.rng)
        return np.tile({"zero": self.F.zero, "one": self.F.one, "pm1": self.F.pm1}[self.mode], (m, 1))

    # ---- device buffers
    def dev(self, arr):
        b = self.ctx.to_device(arr); self.bufs.append(b)
        return b

    def devs(self, vecs):
        """flat share table [v * k + j] of a list of per-vector component lists"""
        return [self.dev(x) for comps in vecs for x in comps]

    def out(self, length):
        """an output buffer of its own, filled with a pattern no other buffer has"""
        self.nout += 1
        s = np.full((length, 4), 0x5A5A5A5A5A5A0000 + self.nout, dtype=np.uint64)
        b = self.dev(s); self.sentinels[id(b)] = s
        return b

    def outs(self, nv, length):
        """nv outputs x k components; for k == 1 a spare buffer per output that is never passed"""
        o = [[self.out(length) for _ in range(self.k)] for _ in range(nv)]
        if self.k == 1: self.spares += [self.out(length) for _ in range(nv)]
        return o

    @staticmethod
    def flat(vecs):
        return [x for comps in vecs for x in comps]

    def check(self, buf, want, name):
        np.testing.assert_array_equal(buf.download(want.shape), want, err_msg=f"{name} (n = {self.n}, k = {self.k}, pc = {self.pc})")

    def untouched(self, buf, name):
        self.check(buf, self.sentinels[id(buf)], name + " keeps its sentinel")

    def check_spares(self):
        for i, b in enumerate(self.spares): self.untouched(b, f"second-component buffer {i} that was not passed")


# ---- round 2: num_w = w + beta k_w omega^i + gamma, den_w = w + beta sigma_w(omega^i) + gamma, the public addends in pc (round2.rs:162-216) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(True))
def test_r2_factors(ctx, curve, n, k, pc, consts):
    """omega^i and sigma are read with strides (4, 4), (1, 1) and (4, 1); the skipped entries are random, so reading one changes the result.
    The wrap case runs the driver's strides (4, 4) only."""
    for ps, ss in (((4, 4),) if n > BLOCK else ((4, 4), (1, 1), (4, 1))):
        with Case(ctx, 2, curve, n, k, pc, consts) as c:
            F = c.F
            pw = c.vec(n * ps, stride=ps); sigma = [c.vec(n * ss, stride=ss) for _ in range(3)]
            w = [c.shares(n) for _ in range(3)]
            coef = c.consts(4)                                                           # beta, beta k1, beta k2, gamma
            outs = c.outs(6, n)
            ctx.plonk_r2_factors(curve, k, pc, n, c.dev(pw), ps, [c.dev(s) for s in sigma], ss, coef, c.devs(w), c.flat(outs))
            for v in range(3):
                pf = F.add(F.mul(coef[v], pw[::ps]), coef[3]); pg = F.add(F.mul(coef[0], sigma[v][::ss]), coef[3])
                for j in range(k):
                    c.check(outs[v][j], F.add(w[v][j], pf) if j == pc else w[v][j], f"strides ({ps}, {ss}): num_{'abc'[v]} component {j}")
                    c.check(outs[3 + v][j], F.add(w[v][j], pg) if j == pc else w[v][j], f"strides ({ps}, {ss}): den_{'abc'[v]} component {j}")
            c.check_spares()


# ---- round 3: ap = b1 x + b2, bp = b3 x + b4, cp = b5 x + b6, zp = b7 x^2 + b8 x + b9, zwp = zp at omega x (round3.rs:246-256, :307-322) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(False))
def test_r3_blind(ctx, curve, n, k, pc, consts):
    with Case(ctx, 3, curve, n, k, pc, consts) as c:
        F = c.F
        x = c.vec(n)
        omega = c.consts(1)[0]; b = c.consts(9 * k).reshape(k, 9, 4)                     # b[j][t] = component j of b_(t+1)
        outs = c.outs(5, n)
        ctx.plonk_r3_blind(curve, k, n, c.dev(x), omega, b, c.flat(outs))
        x2 = F.mul(x, x); xw = F.mul(omega, x); xw2 = F.mul(xw, xw)
        for j in range(k):
            for v, name in enumerate(("ap", "bp", "cp")):
                c.check(outs[v][j], F.add(F.mul(b[j][2 * v], x), b[j][2 * v + 1]), f"{name} component {j}")
            c.check(outs[3][j], F.sum(F.mul(b[j][6], x2), F.mul(b[j][7], x), b[j][8]), f"zp component {j}")
            c.check(outs[4][j], F.sum(F.mul(b[j][6], xw2), F.mul(b[j][7], xw), b[j][8]), f"zwp component {j}")
        c.check_spares()


# ---- round 3: f_w = w + beta k_w x + gamma, g_w = w + beta sigma_w + gamma, the public parts in pc (round3.rs:363-375) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(True))
def test_r3_perm(ctx, curve, n, k, pc, consts):
    with Case(ctx, 4, curve, n, k, pc, consts) as c:
        F = c.F
        x = c.vec(n); sigma = [c.vec(n) for _ in range(3)]
        w = [c.shares(n) for _ in range(3)]
        coef = c.consts(4)                                                               # beta, beta k1, beta k2, gamma
        outs = c.outs(6, n)
        ctx.plonk_r3_perm(curve, k, pc, n, c.dev(x), [c.dev(s) for s in sigma], coef, c.devs(w), c.flat(outs))
        for v in range(3):
            pf = F.add(F.mul(coef[v], x), coef[3]); pg = F.add(F.mul(coef[0], sigma[v]), coef[3])
            for j in range(k):
                c.check(outs[v][j], F.add(w[v][j], pf) if j == pc else w[v][j], f"f_{'abc'[v]} component {j}")
                c.check(outs[3 + v][j], F.add(w[v][j], pg) if j == pc else w[v][j], f"g_{'abc'[v]} component {j}")
        c.check_spares()


# ---- round 3: e1 = qm ab + ql a + qr b + qo c + qc - sum_l L_l buffer_a[l], e1z = qm (ab' + a'b + Z1 a'b') + ql a' + qr b' + qo c' (round3.rs:328-361) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(True))
def test_r3_gate(ctx, curve, n, k, pc, consts):
    """n_lagrange in {0, 1, 3} on the same inputs (the Lagrange table holds 3 rows of n; NULL for 0 rows).  buffer_a is n + 3 random values without
    the 0 / 1 / p - 1 lanes: its first n_lagrange entries are distinct and non-zero, and the entries behind them are what a kernel that indexed it
    by the lane would read.  The wrap case runs all three as well: the sums without the Lagrange term are made once."""
    with Case(ctx, 5, curve, n, k, pc, consts) as c:
        F = c.F
        q = [c.vec(n) for _ in range(5)]                                                 # qm, ql, qr, qo, qc
        lag = c.vec(3 * n, blocks=3)
        ins = [c.shares(n + 3, edges=False)] + [c.shares(n) for _ in range(10)]          # buffer_a, ab, ab', a'b, a'b', a, b, c, a', b', c'
        z1 = c.consts(4)
        d_q, d_lag, d_in = [c.dev(x) for x in q], c.dev(lag), c.devs(ins)
        zsel = z1[np.arange(n) & 3]
        I = lambda s, j: ins[s][j]
        e1 = [F.sum(F.mul(q[0], I(1, j)), F.mul(q[1], I(5, j)), F.mul(q[2], I(6, j)), F.mul(q[3], I(7, j))) for j in range(k)]
        if pc >= 0: e1[pc] = F.add(e1[pc], q[4])
        e1z = [F.sum(F.mul(q[0], F.sum(I(2, j), I(3, j), F.mul(zsel, I(4, j)))), F.mul(q[1], I(8, j)), F.mul(q[2], I(9, j)), F.mul(q[3], I(10, j))) for j in range(k)]
        rows = 0
        for n_lag in (0, 1, 3):
            outs = c.outs(2, n)
            ctx.plonk_r3_gate(curve, k, pc, n, d_q, d_lag if n_lag else None, n_lag, d_in, z1, c.flat(outs))
            for j in range(k):
                for l in range(rows, n_lag): e1[j] = F.sub(e1[j], F.mul(lag[l * n:(l + 1) * n], I(0, j)[l]))
                c.check(outs[0][j], e1[j], f"e1 component {j}, n_lagrange {n_lag}")
                c.check(outs[1][j], e1z[j], f"e1z component {j}, n_lagrange {n_lag}")
            rows = n_lag
        c.check_spares()


# ---- round 3: rz = p0 + p1 + Z1 (p2 + p3 + p4) + Z2 (p5 + p6) + Z3 p7 with Z_a[i & 3] (round3.rs:54-71 over the sums of :32-49) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(False))
def test_mul4_tail(ctx, curve, n, k, pc, consts):
    with Case(ctx, 6, curve, n, k, pc, consts) as c:
        F = c.F
        p = [c.shares(n) for _ in range(8)]
        z = c.consts(12).reshape(3, 4, 4)                                                # Z1, Z2, Z3: four values each
        outs = c.outs(1, n)
        ctx.plonk_mul4_tail(curve, k, n, c.devs(p), z, c.flat(outs))
        r = np.arange(n) & 3
        for j in range(k):
            want = F.sum(p[0][j], p[1][j], F.mul(z[0][r], F.sum(p[2][j], p[3][j], p[4][j])), F.mul(z[1][r], F.add(p[5][j], p[6][j])), F.mul(z[2][r], p[7][j]))
            c.check(outs[0][j], want, f"rz component {j}")
        c.check_spares()


# ---- round 3: t = e1 + alpha (e2 - e3) + alpha^2 L1 (z - 1), tz = e1z + alpha (e2z - e3z) + alpha^2 L1 z', the 1 in pc (round3.rs:405-437) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(True))
def test_r3_t(ctx, curve, n, k, pc, consts):
    """L1 is the first row of a longer Lagrange table, as the driver passes it"""
    with Case(ctx, 7, curve, n, k, pc, consts) as c:
        F = c.F
        lag = c.vec(2 * n + 3)
        ins = [c.shares(n) for _ in range(8)]                                            # e1, e1z, e2, e3, e2z, e3z, z, z'
        alpha = c.consts(1)[0]
        outs = c.outs(2, n)
        ctx.plonk_r3_t(curve, k, pc, n, c.dev(lag), c.devs(ins), alpha, c.flat(outs))
        l = F.mul(F.mul(alpha, alpha), lag[:n])
        for j in range(k):
            I = lambda s: ins[s][j]
            z = F.sub(I(6), F.one) if j == pc else I(6)
            c.check(outs[0][j], F.sum(I(0), F.mul(alpha, F.sub(I(2), I(3))), F.mul(l, z)), f"t component {j}")
            c.check(outs[1][j], F.sum(I(1), F.mul(alpha, F.sub(I(4), I(5))), F.mul(l, I(7))), f"tz component {j}")
        c.check_spares()


# ---- round 3 after the inverse NTTs: run_b = run_(b-1) - t_b, t_b = run_b + tz_b over the four blocks of n coefficients (round3.rs:438-451) ----
@pytest.mark.parametrize("curve,n,k,pc,consts", cases(False, const_modes=()))
def test_r3_divide(ctx, curve, n, k, pc, consts):
    """in place on t, as the driver calls it; n is the block length, t and tz hold 4n elements.  The kernel has no constants."""
    with Case(ctx, 8, curve, n, k, pc, consts) as c:
        F = c.F
        t = c.shares(4 * n, blocks=4); tz = c.shares(4 * n, blocks=4)
        d_t, d_tz = [c.dev(x) for x in t], [c.dev(x) for x in tz]
        spare = c.out(4 * n) if k == 1 else None
        ctx.plonk_r3_divide(curve, k, n, d_t, d_tz)
        for j in range(k):
            run, got = np.zeros((n, 4), dtype=np.uint64), d_t[j].download((4 * n, 4))
            for b in range(4):
                run = F.sub(run, t[j][b * n:(b + 1) * n])
                np.testing.assert_array_equal(got[b * n:(b + 1) * n], F.add(run, tz[j][b * n:(b + 1) * n]), err_msg=f"t block {b} component {j} (n = {n}, k = {k})")
            c.check(d_tz[j], tz[j], f"tz component {j} is unchanged")
        if spare is not None: c.untouched(spare, "second-component t that was not passed")


# ---- round 1: ext[n_priv + a] = f1 w[id1] + f2 w[id2], w[id] = pub[id] in component pc (0 elsewhere) for id < n_inputs (round1.rs:209-238) ----
N_INPUTS, N_PRIV = 7, 50


def synthetic_additions(c, widths):
    """an addition list whose dependency levels have the given widths: (ids (A, 2) uint32, coeffs (A, 2, 4)).  Every addition of level L > 0 has
    one operand (first or second) from level L - 1; the other is public, private or any earlier result.  Indices are in dependency order (as in a
    zkey) with the levels interleaved."""
    rng, F = c.rng, c.F
    A, base = sum(widths), N_INPUTS + N_PRIV
    start = [0] + np.cumsum(widths).tolist()
    fix, other = np.zeros(A, dtype=np.int64), np.zeros(A, dtype=np.int64)
    for L, w in enumerate(widths):
        s = slice(start[L], start[L + 1])
        pick = lambda hi: np.choose(rng.integers(0, hi, size=w), [rng.integers(0, N_INPUTS, size=w), N_INPUTS + rng.integers(0, N_PRIV, size=w),
                                                                  base + rng.integers(0, max(start[L], 1), size=w)])
        other[s] = pick(3 if L else 2)
        fix[s] = base + rng.integers(start[L - 1], start[L], size=w) if L else pick(2)
    sp = start[max(range(1, len(widths)), key=lambda L: widths[L])]                      # the widest level above 0 takes the operands every list must have
    other[sp:sp + 5] = (0, N_INPUTS - 1, N_INPUTS, base - 1, fix[sp + 4])                 # first / last public, first / last private, id1 == id2
    other[0], fix[0] = 0, N_INPUTS                                                       # level 0 starts from a public and a private operand
    swap = rng.random(A) < 0.5
    ids = np.stack([np.where(swap, other, fix), np.where(swap, fix, other)], axis=1)
    coef = orc.random_field(c.curve, FR, 2 * A, rng).reshape(A, 2, 4)
    for i, (e1, e2) in enumerate(((F.zero, None), (None, F.zero), (F.pm1, None), (None, F.pm1), (F.one, F.one), (F.zero, F.zero), (F.pm1, F.pm1))):
        for a in (sp + 3 + i, sp + 20 + i):                                              # coefficients 0, 1, p - 1 in either position and in both
            if e1 is not None: coef[a, 0] = e1
            if e2 is not None: coef[a, 1] = e2
    # renumber: a random interleaving of the levels that keeps every operand before its use
    key, r0, r1 = [0.0] * A, (len(widths) * rng.random(A)).tolist(), rng.random(A).tolist()
    for a, row in enumerate(ids.tolist()):
        deps = [x - base for x in row if x >= base]
        key[a] = (max(key[d] for d in deps) if deps else r0[a]) + r1[a]
    rank = np.empty(A, dtype=np.int64); rank[np.argsort(key)] = np.arange(A)
    ids = np.where(ids >= base, base + rank[np.maximum(ids - base, 0)], ids)
    new_ids, new_coef = np.empty_like(ids), np.empty_like(coef)
    new_ids[rank], new_coef[rank] = ids, coef
    return new_ids.astype(np.uint32), new_coef


def dependency_levels(ids):
    """level of every addition: 0 with witness operands only, else one above the highest operand"""
    base, A = N_INPUTS + N_PRIV, ids.shape[0]
    lvl = [0] * A
    for a, row in enumerate(ids.tolist()):
        deps = [x - base for x in row if x >= base]
        assert all(d < a for d in deps), "the list is not in dependency order"
        if deps: lvl[a] = 1 + max(lvl[d] for d in deps)
    lvl = np.array(lvl, dtype=np.int64)
    return lvl


def run_additions(ctx, c, ids, coef, lvl, reference):
    F, k, pc = c.F, c.k, c.pc
    A, base = ids.shape[0], N_INPUTS + N_PRIV
    order = np.concatenate([c.rng.permutation(np.flatnonzero(lvl == L)) for L in range(lvl.max() + 1)]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(np.bincount(lvl))])
    assert not np.array_equal(order, np.arange(A)), "the order array must not be the identity"
    pub = c.vec(N_INPUTS); priv = c.shares(N_PRIV)
    ext = [np.concatenate([priv[j], np.full((A, 4), 0x5A5A5A5A5A5A5A00 + j, dtype=np.uint64)]) for j in range(k)]
    d_ext = [c.dev(x) for x in ext] + [None] * (2 - k)                                   # k == 1: d_ext_b = NULL
    spare = c.out(N_PRIV + A) if k == 1 else None
    d_order, d_ids, d_coef, d_pub = c.dev(order), c.dev(ids), c.dev(coef), c.dev(pub)
    for L in range(len(off) - 1):                                                        # one launch per level, as extend_witness (host/plonk.hpp)
        ctx.plonk_additions(c.curve, d_order, int(off[L + 1] - off[L]), d_ids, d_coef, d_pub, N_INPUTS, pc, d_ext[0], d_ext[1], N_PRIV, order_off=int(off[L]))
    for j in range(k):
        w = np.concatenate([pub if j == pc else np.zeros_like(pub), priv[j], np.zeros((A, 4), dtype=np.uint64)])
        reference(F, w, ids, coef, lvl)
        got = d_ext[j].download((N_PRIV + A, 4))
        np.testing.assert_array_equal(got[N_PRIV:], w[base:], err_msg=f"additions, component {j} (k = {k}, pc = {pc})")
        np.testing.assert_array_equal(got[:N_PRIV], priv[j], err_msg=f"private witness, component {j}")
    if spare is not None: c.untouched(spare, "second-component ext that was not passed")


def sequential_reference(F, w, ids, coef, lvl):
    """calculate_additions: one addition after the other, in dependency order"""
    base = N_INPUTS + N_PRIV
    for a in range(ids.shape[0]):
        w[base + a] = orc.field_op(F.curve, FR, "add", orc.field_op(F.curve, FR, "mul", coef[a, 0], w[ids[a, 0]]), orc.field_op(F.curve, FR, "mul", coef[a, 1], w[ids[a, 1]]))


def level_reference(F, w, ids, coef, lvl):
    """the same sums, one level of independent additions at a time (the wrap case: half a million sequential steps would take a minute)"""
    base = N_INPUTS + N_PRIV
    for L in range(lvl.max() + 1):
        a = np.flatnonzero(lvl == L)
        w[base + a] = F.add(F.mul(coef[a, 0], w[ids[a, 0]]), F.mul(coef[a, 1], w[ids[a, 1]]))


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
@pytest.mark.parametrize("k,pc", KPC)
def test_plonk_additions(ctx, curve, k, pc):
    """four levels of widths 1, 300, 5000 and 300, launched level by level; operands: the first and last public and private entries, results of
    earlier levels, id1 == id2; coefficients 0, 1 and p - 1; a shuffled order array"""
    with Case(ctx, 1, curve, 5, k, pc) as c:
        ids, coef = synthetic_additions(c, [1, 300, 5000, 300])
        lvl = dependency_levels(ids)
        assert np.bincount(lvl).tolist() == [1, 300, 5000, 300]
        flat = ids.ravel().tolist()
        assert {0, N_INPUTS - 1, N_INPUTS, N_INPUTS + N_PRIV - 1} <= set(flat) and (ids[:, 0] == ids[:, 1]).any()
        run_additions(ctx, c, ids, coef, lvl, sequential_reference)


def test_plonk_additions_wraps_the_grid(ctx):
    """one level of 2^19 + 259 additions (the grid-stride loop wraps) under a level of 300 that reads its last results; the coefficients are the
    tiled block, the reference goes level by level"""
    with Case(ctx, 1, BN254, WRAP, 2, 1) as c:
        ids, _ = synthetic_additions(c, [WRAP, 300])
        coef = c.vec(2 * ids.shape[0]).reshape(-1, 2, 4)
        lvl = dependency_levels(ids)
        assert np.bincount(lvl).tolist() == [WRAP, 300]
        c.big = False                                                                    # the witness itself stays small and random
        run_additions(ctx, c, ids, coef, lvl, level_reference)


# ---- argument checks: nothing is launched ------------------------------------------------------------------------------------------------
def valid_calls(ctx, c, n):
    """entry -> (call(**kw), kw, takes k, takes pc): one valid k = 2 call per entry on small distinct buffers, every output sentinel-filled"""
    k = 2
    V = lambda nv, length=n: [c.dev(c.vec(length)) for _ in range(nv)]
    O = lambda nv, length=n: [c.out(length) for _ in range(nv)]
    return {
        "cg_plonk_additions_dev": (lambda curve, k, pc, n, order, ids, coeffs, pub, ext_a, ext_b: ctx.plonk_additions(curve, order, n, ids, coeffs, pub, 3, pc, ext_a, ext_b, 4),
                                   dict(order=c.dev(np.arange(n, dtype=np.uint32)), ids=c.dev(np.zeros((n, 2), dtype=np.uint32)), coeffs=V(1, 2 * n)[0], pub=V(1, 3)[0],
                                        ext_a=O(1, 4 + n)[0], ext_b=O(1, 4 + n)[0]), False, True),
        "cg_plonk_r2_factors_dev": (lambda curve, k, pc, n, pw, sigmas, coeffs, wires, outs: ctx.plonk_r2_factors(curve, k, pc, n, pw, 4, sigmas, 4, coeffs, wires, outs),
                                    dict(pw=V(1, 4 * n)[0], sigmas=V(3, 4 * n), coeffs=c.consts(4), wires=V(3 * k), outs=O(6 * k)), True, True),
        "cg_plonk_r3_blind_dev": (lambda curve, k, pc, n, pw, omega, blind, outs: ctx.plonk_r3_blind(curve, k, n, pw, omega, blind, outs),
                                  dict(pw=V(1)[0], omega=c.consts(1), blind=c.consts(9 * k), outs=O(5 * k)), True, False),
        "cg_plonk_r3_perm_dev": (lambda curve, k, pc, n, pw, sigmas, coeffs, wires, outs: ctx.plonk_r3_perm(curve, k, pc, n, pw, sigmas, coeffs, wires, outs),
                                 dict(pw=V(1)[0], sigmas=V(3), coeffs=c.consts(4), wires=V(3 * k), outs=O(6 * k)), True, True),
        "cg_plonk_r3_gate_dev": (lambda curve, k, pc, n, q, lagrange, ins, z1, outs: ctx.plonk_r3_gate(curve, k, pc, n, q, lagrange, 1, ins, z1, outs),
                                 dict(q=V(5), lagrange=V(1)[0], ins=V(11 * k), z1=c.consts(4), outs=O(2 * k)), True, True),
        "cg_plonk_mul4_tail_dev": (lambda curve, k, pc, n, prods, z, rz: ctx.plonk_mul4_tail(curve, k, n, prods, z, rz),
                                   dict(prods=V(8 * k), z=c.consts(12), rz=O(k)), True, False),
        "cg_plonk_r3_t_dev": (lambda curve, k, pc, n, l1, ins, alpha, outs: ctx.plonk_r3_t(curve, k, pc, n, l1, ins, alpha, outs),
                              dict(l1=V(1)[0], ins=V(8 * k), alpha=c.consts(1), outs=O(2 * k)), True, True),
        "cg_plonk_r3_divide_dev": (lambda curve, k, pc, n, t, tz: ctx.plonk_r3_divide(curve, k, n, t, tz),
                                   dict(t=O(k, 4 * n), tz=V(k, 4 * n)), True, False),
    }


ENTRIES = ("cg_plonk_additions_dev", "cg_plonk_r2_factors_dev", "cg_plonk_r3_blind_dev", "cg_plonk_r3_perm_dev", "cg_plonk_r3_gate_dev", "cg_plonk_mul4_tail_dev",
           "cg_plonk_r3_t_dev", "cg_plonk_r3_divide_dev")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_bad_arguments(ctx, entry):
    """a NULL table, vector or constant, a NULL share component below k, k = 0 and 3, pc = k and an unknown curve end with an error; n = 0 is a
    success; after all of it every output still holds its sentinel"""
    n = 5
    with Case(ctx, 9, BN254, n, 2, 1) as c:
        call, kw, takes_k, takes_pc = valid_calls(ctx, c, n)[entry]
        def refused(what, curve=BN254, k=2, pc=-1, n=n, **over):
            with pytest.raises(cg.BackendError):
                call(curve, k, pc, n, **{**kw, **over})
                pytest.fail(f"{entry} accepted {what}")

        for name, val in kw.items():
            if entry == "cg_plonk_additions_dev" and name == "ext_b": continue           # NULL d_ext_b is one share component
            refused(f"NULL {name}", **{name: None})
            if isinstance(val, list):
                for j in ((0, len(val) - 1) if len(val) % 2 or name in ("sigmas", "q") else (0, 1, len(val) - 2, len(val) - 1)):
                    refused(f"NULL entry {j} of {name}", **{name: val[:j] + [None] + val[j + 1:]})
        if takes_k:
            refused("k = 0", k=0); refused("k = 3", k=3)
        if takes_pc:
            refused("pc = k = 2", pc=2); refused("pc = -2", pc=-2)
            if takes_k: refused("pc = k = 1", k=1, pc=1)
            else: refused("pc = k = 1", pc=1, ext_b=None)
        refused("an unknown curve", curve=7)
        call(BN254, 2, 1 if takes_pc else -1, 0, **kw)                                   # n = 0: success, nothing written
        if entry == "cg_plonk_additions_dev":
            call(BN254, 2, 1, 0, **{**kw, "order": None, "ids": None, "coeffs": None, "pub": None})
        for b in c.bufs:
            if id(b) in c.sentinels: c.untouched(b, f"{entry}: an output")
