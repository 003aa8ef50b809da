"""Which gate does a witness break?  cg_plonk_gate_check_dev and cg_vec_mismatch_dev alone at the lane, wave and workgroup edges of a
256-lane workgroup, then cgh_plonk_session_check_witness on shipped, compiled and synthetic keys and cgh_r1cs_plonk_gate_origin.  Every
expectation is the gate residual restated with Python integers (plonk_audit_tools.py, pinned on the CPU by test_plonk_audit_host.py)."""
import random

import numpy as np
import pytest

import oracle_lib as orc
import plonk_audit_tools as at
import plonk_setup_tools as pt
import r1cs_tools as rt
from oracle_lib import BN254, BLS12_381
from product import cg, ensure_built
from r1cs_tools import CURVES, NO_ROW, R

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)                # rows: the lane, wave and workgroup edges of a 256-lane workgroup
N_EXT = 5                                                   # wires beyond the public ones in the random tables


def mont(curve, values):
    r = rt.modulus(curve)
    return np.frombuffer(b"".join((v % r * R % r).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4)


def strided(curve, values, stride, rnd):
    """element i at i * stride; what lies between is random and must not be read"""
    if stride == 1:
        return mont(curve, values)
    r = rt.modulus(curve)
    out = [rnd.randrange(1, r) for _ in range(len(values) * stride)]
    out[::stride] = values
    return mont(curve, out)


def plants(n, nc):
    """name -> rows made to fail (through qc): row 0, the last row, both sides of the wave and workgroup edges, a padding row, every row, none"""
    p = {"none": [], "row_0": [0], "last_row": [n - 1], "every_row": list(range(n))}
    if n > 64: p["rows_63_64"] = [63, 64]
    if n > 256: p["rows_255_256"] = [255, 256]
    if nc < n: p["padding_row"] = [nc + (n - nc) // 2]
    return p


@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def result_of(buf):
    res = buf.download((2,))
    return int(res[0]), int(res[1])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_gate_check_kernel(ctx, curve, n):
    """random gate tables that a random witness satisfies (qc solved for, the padding rows and the public-input term included), then rows
    made to fail through qc: count and first row are exact for every plant, with contiguous selectors and with a stride of 4"""
    r = rt.modulus(curve)
    rnd = random.Random(1000 * curve + n)
    d_res = ctx.alloc(16)
    seen = set()
    for n_public in sorted({0, 1, n}):
        n_wires = n_public + 1 + N_EXT
        w = [0] + [rnd.randrange(1, r) for _ in range(n_wires - 1)]
        d_pub, d_ext = ctx.to_device(mont(curve, w[:n_public + 1])), ctx.to_device(mont(curve, w[n_public + 1:]))
        for nc in sorted({0, n - 1, n}):
            maps = [[rnd.randrange(n_wires) for _ in range(nc)] for _ in range(3)]
            for m in maps[:1]:
                if nc: m[0], m[-1] = n_wires - 1, 0                                   # the last wire and wire 0 are both named
            q = [[rnd.randrange(r) if i < nc else 0 for i in range(n)] for _ in range(4)] + [[0] * n]
            for i in range(n):                                                          # solve qc: every row holds
                a, b, c = (w[maps[0][i]], w[maps[1][i]], w[maps[2][i]]) if i < nc else (0, 0, 0)
                q[4][i] = -(q[0][i] * a * b + q[1][i] * a + q[2][i] * b + q[3][i] * c - (w[i + 1] if i < n_public else 0)) % r
            assert at.residual_rows(n, nc, n_public, maps, q, w, r) == []
            d_maps = [ctx.to_device(np.array(m if m else [0], dtype=np.uint32)) for m in maps]
            for stride in (1, 4):
                d_q = [ctx.to_device(strided(curve, q[s], stride, rnd)) for s in range(4)]
                for name, rows in plants(n, nc).items():
                    qc = list(q[4])
                    for i in rows:
                        qc[i] = (qc[i] + 1 + rnd.randrange(r - 1)) % r
                    want = at.verdict(at.residual_rows(n, nc, n_public, maps, q[:4] + [qc], w, r))
                    assert want == (len(rows), min(rows, default=NO_ROW)), name
                    d_qc = ctx.to_device(strided(curve, qc, stride, rnd))
                    ctx.plonk_gate_check(curve, d_maps, nc, d_q + [d_qc], stride, n, d_pub, n_public, d_ext, n_wires, d_res)
                    assert result_of(d_res) == want, (n_public, nc, stride, name)
                    d_qc.free(); seen.add(name)
                for b in d_q: b.free()
            for b in d_maps: b.free()
        d_pub.free(); d_ext.free()
    d_res.free()
    assert {"none", "row_0", "last_row", "every_row"} <= seen and ("padding_row" in seen) and (n <= 64 or "rows_63_64" in seen) and (n <= 256 or "rows_255_256" in seen)


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_gate_check_kernel_witness_side(ctx, curve):
    """the same residual with the failure planted in the WITNESS: a changed extended-witness entry, a changed public input (which moves the
    public-input term of its row as well), and wire 0 read as whatever pub[0] holds"""
    r = rt.modulus(curve); rnd = random.Random(77 + curve)
    n, nc, n_public = 257, 200, 3
    n_wires = n_public + 1 + N_EXT
    w = [0] + [rnd.randrange(1, r) for _ in range(n_wires - 1)]
    maps = [[rnd.randrange(n_wires) for _ in range(nc)] for _ in range(3)]
    q = [[rnd.randrange(r) if i < nc else 0 for i in range(n)] for _ in range(4)] + [[0] * n]
    for i in range(n):
        a, b, c = (w[maps[0][i]], w[maps[1][i]], w[maps[2][i]]) if i < nc else (0, 0, 0)
        q[4][i] = -(q[0][i] * a * b + q[1][i] * a + q[2][i] * b + q[3][i] * c - (w[i + 1] if i < n_public else 0)) % r
    d_maps = [ctx.to_device(np.array(m, dtype=np.uint32)) for m in maps]
    d_q = [ctx.to_device(mont(curve, v)) for v in q]
    d_res = ctx.alloc(16)
    for wire in (0, 2, n_public + 1, n_wires - 1):
        v = list(w); v[wire] = (v[wire] + 1) % r
        want = at.verdict(at.residual_rows(n, nc, n_public, maps, q, v, r))
        assert want[0] > 0
        d_pub, d_ext = ctx.to_device(mont(curve, v[:n_public + 1])), ctx.to_device(mont(curve, v[n_public + 1:]))
        ctx.plonk_gate_check(curve, d_maps, nc, d_q, 1, n, d_pub, n_public, d_ext, n_wires, d_res)
        assert result_of(d_res) == want, wire
        d_pub.free(); d_ext.free()
    # a map entry that is no wire: its row is counted, nothing is read for it
    maps[1][150] = n_wires
    d_bad = ctx.to_device(np.array(maps[1], dtype=np.uint32))
    d_pub, d_ext = ctx.to_device(mont(curve, w[:n_public + 1])), ctx.to_device(mont(curve, w[n_public + 1:]))
    ctx.plonk_gate_check(curve, [d_maps[0], d_bad, d_maps[2]], nc, d_q, 1, n, d_pub, n_public, d_ext, n_wires, d_res)
    assert result_of(d_res) == (1, 150)
    with pytest.raises(cg.BackendError):
        ctx.plonk_gate_check(curve, d_maps, n + 1, d_q, 1, n, d_pub, n_public, d_ext, n_wires, d_res)      # more gates than rows
    with pytest.raises(cg.BackendError):
        ctx.plonk_gate_check(curve, d_maps, nc, d_q, 0, n, d_pub, n_public, d_ext, n_wires, d_res)         # no stride
    with pytest.raises(cg.BackendError):
        ctx.plonk_gate_check(curve, d_maps, nc, d_q, 1, n, d_pub, n_public, d_ext, n_public, d_res)        # the wires do not hold the public ones
    ctx.sync()
    for b in d_maps + d_q + [d_bad, d_pub, d_ext, d_res]: b.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_vec_mismatch(ctx, curve, n):
    r = rt.modulus(curve); rnd = random.Random(31 * n + curve)
    a = [rnd.randrange(r) for _ in range(n)]
    d_res = ctx.alloc(16)
    where = plants(n, n)
    where["last_two"] = [n - 1] if n == 1 else [n - 2, n - 1]
    for sa in (1, 4):
        d_a = ctx.to_device(strided(curve, a, sa, rnd))
        for sb in (1, 4):
            for name, rows in where.items():
                b = list(a)
                for i in rows:
                    b[i] = (b[i] + 1 + rnd.randrange(r - 1)) % r
                d_b = ctx.to_device(strided(curve, b, sb, rnd))
                ctx.vec_mismatch(curve, d_a, d_b, n, d_res, a_stride=sa, b_stride=sb)
                assert result_of(d_res) == (len(rows), min(rows, default=NO_ROW)), (sa, sb, name)
                for first in sorted({0, 1, n // 2, n - 1, n}):                         # a row range: what lies before it is not counted
                    left = [i for i in rows if i >= first]
                    ctx.vec_mismatch(curve, d_a, d_b, n, d_res, a_stride=sa, b_stride=sb, first=first)
                    assert result_of(d_res) == (len(left), min(left, default=NO_ROW)), (sa, sb, name, first)
                d_b.free()
        d_a.free()
    # against zero over a row range: nonzero entries planted in a vector of zeros
    for stride in (1, 4):
        for name, rows in where.items():
            z = [0] * n
            for i in rows:
                z[i] = 1 + rnd.randrange(r - 1)
            d_z = ctx.to_device(strided(curve, z, stride, rnd))
            for first in sorted({0, n // 2, n - 1, n}):
                left = [i for i in rows if i >= first]
                ctx.vec_mismatch(curve, d_z, None, n, d_res, a_stride=stride, first=first)
                assert result_of(d_res) == (len(left), min(left, default=NO_ROW)), (stride, name, first)
            d_z.free()
    with pytest.raises(cg.BackendError):
        ctx.vec_mismatch(curve, d_res, d_res, 1, d_res, a_stride=0)
    ctx.sync()
    d_res.free()


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
def check_against_restatement(session, key, w_ints, wires):
    """the honest witness gives (0, none); each named entry changed in turn gives the restatement's verdict"""
    curve = key.curve
    assert session.check_witness(mont(curve, w_ints)) == (0, NO_ROW)
    rnd = random.Random(5)
    broke = 0
    for wire in wires:
        v = list(w_ints); v[wire] = (v[wire] + rnd.randrange(1, key.r)) % key.r
        want = at.verdict(key.bad_rows(v))
        assert session.check_witness(mont(curve, v)) == want, wire
        broke += want[0] > 0
    return broke


@pytest.mark.parametrize("curve_name,circuit", at.FIXTURES)
def test_session_check_on_the_shipped_keys(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]
    path = at.plonk_fx(curve_name, circuit, "circuit.zkey")
    key = at.Key(curve, path)
    w, w_ints = at.read_witness(curve, at.plonk_fx(curve_name, circuit, "witness.wtns"))
    s = cg.PlonkSession(curve, path)
    try:
        assert s.check_witness(w) == (0, NO_ROW)
        assert at.verdict(key.bad_rows(w_ints)) == (0, NO_ROW)
        private, public = len(w_ints) - 1, 1                                           # one private entry, then one public entry
        broke = check_against_restatement(s, key, w_ints, [private, public, min(key.n_public + 1, private)])
        assert broke >= 2 if key.nc > key.n_public else broke == 0                    # (the shipped sum_arrays key has public-input gates only)
        with pytest.raises(cg.BackendError):
            s.check_witness(w[:-1])
        # the leading entry is not read: wire 0 is zero whatever the witness says there
        v = list(w_ints); v[0] = 5
        assert s.check_witness(mont(curve, v)) == (0, NO_ROW)
    finally:
        s.close()


def test_session_check_on_a_compiled_poseidon_key(tmp_path):
    """a key made by setup_plonk from the Poseidon .r1cs: domain 4 096, 1 857 additions in chains"""
    ensure_built()
    curve = BN254
    zp = str(tmp_path / "poseidon.zkey")
    r = cg.R1cs(curve, rt.fx("bn254", "poseidon", "circuit.r1cs"))
    try:
        cg.setup_plonk(r, 20240611, zp)
    finally:
        r.close()
    key = at.Key(curve, zp)
    assert (key.n, key.n_add) == (4096, 1857)
    _, w_ints = at.read_witness(curve, rt.fx("bn254", "poseidon", "witness.wtns"))
    s = cg.PlonkSession(curve, zp)
    try:
        assert check_against_restatement(s, key, w_ints, [len(w_ints) - 1, 1, len(w_ints) // 2]) == 3
    finally:
        s.close()


def test_session_check_on_a_synthetic_key_at_2_16(tmp_path):
    ensure_built()
    curve = BN254
    zp, wp = str(tmp_path / "p16.zkey"), str(tmp_path / "p16.wtns")
    cg.host_synth_plonk_circuit(curve, 16, 29, zp, wp, n_public=3, n_additions=1000)
    key = at.Key(curve, zp)
    assert (key.n, key.n_add) == (1 << 16, 1000)
    _, w_ints = at.read_witness(curve, wp)
    s = cg.PlonkSession(curve, zp)
    try:
        fed = key.adds[500][0] if key.adds[500][0] > key.n_public else key.adds[500][1]   # an entry an addition reads
        assert check_against_restatement(s, key, w_ints, [fed if fed < len(w_ints) else len(w_ints) - 1, len(w_ints) - 1]) >= 1
    finally:
        s.close()


def test_gate_origin_on_the_branch_circuit(tmp_path):
    """every checked gate row maps back to the R1CS row the Python compiler made it from: the first and the last row, every public-input row,
    the additions and the gate of the rows at both scan tile edges and of a row with a 130-term combination, a padding row"""
    ensure_built()
    curve = BN254; mod = rt.modulus(curve)
    n_wires, n_pub, cons, _ = pt.branch_circuit(curve)
    path = str(tmp_path / "branch.r1cs")
    rt.write_r1cs(path, mod, n_wires, 0, n_pub, n_wires - 1 - n_pub, cons)
    g = pt.compile_gates(n_wires, n_pub, cons, mod)
    origin = [(cg.PLONK_GATE_PUBLIC, None, None)] * n_pub                                # gate row -> (kind, R1CS row, addition index)
    for row, n_add in enumerate(g["row_adds"]):
        origin += [(cg.PLONK_GATE_ADDITION, row, j) for j in range(n_add)] + [(cg.PLONK_GATE_CONSTRAINT, row, None)]
    assert len(origin) == g["n_constraints"]
    origin += [(cg.PLONK_GATE_PADDING, None, None)] * (g["n"] - len(origin))
    long_row = next(i for i, (a, b, c) in enumerate(cons) if max(len(a), len(b), len(c)) >= 130)
    start = lambda row: n_pub + row + sum(g["row_adds"][:row])
    rows = {0, g["n"] - 1, g["n_constraints"] - 1, g["n_constraints"]} | set(range(n_pub + 2))
    for row in (long_row, long_row + 1, 2047, 2048, 4095, 4096, len(cons) - 1):
        rows |= {start(row) - 1, start(row), start(row) + g["row_adds"][row] // 2, start(row) + g["row_adds"][row]}
    rows |= set(random.Random(3).sample(range(g["n"]), 100))
    assert {origin[i][0] for i in rows} == {cg.PLONK_GATE_PUBLIC, cg.PLONK_GATE_ADDITION, cg.PLONK_GATE_CONSTRAINT, cg.PLONK_GATE_PADDING}
    assert g["row_adds"][long_row] >= 129 and origin[start(long_row) + g["row_adds"][long_row]] == (cg.PLONK_GATE_CONSTRAINT, long_row, None)
    r = cg.R1cs(curve, path)
    try:
        for i in sorted(rows):
            assert r.plonk_gate_origin(i) == origin[i], i
        with pytest.raises(cg.BackendError):
            r.plonk_gate_origin(g["n"])
    finally:
        r.close()
