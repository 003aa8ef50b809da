"""Groth16 development keys from an .r1cs (cgh_setup_groth16_dev) and the column sums behind them (cg_qap_columns_dev).  Key file: header and
section 4 equal the shipped key's, the product's own validation accepts it, it is a function of the seed.  Key contents: u_i, v_i, w_i, the
L query exponents and the H exponents recomputed with Python integers from cgh_setup_toxic and the .r1cs, the points compared with host scalar
multiplications of the generators.  End to end: a proof on the new key verifies, equals the oracle's bit for bit, and a wrong witness fails."""
import numpy as np
import pytest

import oracle_lib as orc
import r1cs_tools as rt
from r1cs_tools import CURVES, NO_ROW, PAIRS, fx
from oracle_lib import BN254, BLS12_381, FR, G1, G2
from product import cg, ensure_built

pytestmark = pytest.mark.gpu
SEED = 20240607
G2_CHECKED = {"multiplier2", "multiplier2_example", "kyc"}       # host G2 products cost ~10x a G1 product: the small circuits only


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    """one development key per fixture pair, made once for the module: (curve_name, circuit) -> path"""
    ensure_built()
    d = tmp_path_factory.mktemp("devkeys")
    out = {}
    for curve_name, circuit in PAIRS:
        r = cg.R1cs(CURVES[curve_name], fx(curve_name, circuit, "circuit.r1cs"))
        out[(curve_name, circuit)] = str(d / f"{curve_name}_{circuit}.zkey")
        cg.setup_groth16(r, SEED, out[(curve_name, circuit)])
        r.close()
    return out


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_key_file(keys, curve_name, circuit, tmp_path):
    curve = CURVES[curve_name]
    path, shipped = keys[(curve_name, circuit)], fx(curve_name, circuit, "circuit.zkey")
    mine, theirs = rt.zkey_sections(path), rt.zkey_sections(shipped)
    assert sorted(mine) == list(range(1, 10))
    assert rt.zkey_header_numbers(curve, mine) == rt.zkey_header_numbers(curve, theirs)
    assert cg.host_zkey_info(curve, path) == cg.host_zkey_info(curve, shipped)
    assert mine[4] == theirs[4]
    assert [len(mine[i]) for i in (3, 5, 6, 7, 8, 9)] == [len(theirs[i]) for i in (3, 5, 6, 7, 8, 9)]
    cg.host_zkey_validate(curve, path)                                        # every point on its curve and in its subgroup
    r = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
    try:
        again, other = str(tmp_path / "again.zkey"), str(tmp_path / "other.zkey")
        cg.setup_groth16(r, SEED, again); cg.setup_groth16(r, SEED + 1, other)
    finally:
        r.close()
    data = open(path, "rb").read()
    assert open(again, "rb").read() == data
    assert open(other, "rb").read() != data
    assert rt.zkey_sections(other)[4] == mine[4]


def qap_by_integers(curve, p, toxic):
    """u, v, w per wire, the L-query exponents and the H exponents of the key, by Python integers"""
    mod = rt.modulus(curve)
    tau, alpha, beta, gamma, delta = toxic
    n_c, n_inp, n_w = p["n_constraints"], p["n_public"] + 1, p["n_wires"]
    m, power = 1, 0
    while m < n_c + n_inp:
        m, power = 2 * m, power + 1
    omega_m, g_m, m_orc = orc.groth16_domain(curve, power, n_c, n_inp)
    omega, g = rt.from_mont(curve, omega_m)[0], rt.from_mont(curve, g_m)[0]
    assert m_orc == m and pow(omega, m, mod) == 1 and (m == 1 or pow(omega, m // 2, mod) == mod - 1) and pow(g, m, mod) == mod - 1
    zt = (pow(tau, m, mod) - 1) * pow(m, -1, mod) % mod
    lag = [zt * pow(omega, j, mod) * pow(tau - pow(omega, j, mod), -1, mod) % mod for j in range(m)]
    sums = [[0] * n_w for _ in range(3)]
    for j, con in enumerate(p["constraints"]):
        for k in range(3):
            for wire, v in con[k]:
                sums[k][wire] = (sums[k][wire] + v * lag[j]) % mod
    for s in range(n_inp):
        sums[0][s] = (sums[0][s] + lag[n_c + s]) % mod
    u, v, w = sums
    lq = [(beta * u[i] + alpha * v[i] + w[i]) * pow(gamma if i < n_inp else delta, -1, mod) % mod for i in range(n_w)]
    hf = (pow(tau, 2 * m, mod) - 1) * pow(2 * m * delta, -1, mod) % mod
    h = [hf * g * pow(omega, i, mod) * pow(tau - g * pow(omega, i, mod), -1, mod) % mod for i in range(m)]
    return u, v, lq, h


def points_of(curve, group, scalars):
    gen = cg.point_generator(curve, group)
    return b"".join(cg.point_to_affine(curve, group, cg.point_scalar_mul(curve, group, gen, k)).tobytes() for k in rt.to_mont(curve, scalars))


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_key_contents_from_python_integers(keys, curve_name, circuit):
    curve = CURVES[curve_name]
    p = rt.parse_r1cs(fx(curve_name, circuit, "circuit.r1cs"))
    assert p["n_wires"] <= 243
    toxic = rt.from_mont(curve, cg.setup_toxic(curve, SEED))
    assert len(set(toxic)) == 5 and all(0 < t < rt.modulus(curve) for t in toxic)
    assert rt.from_mont(curve, cg.setup_toxic(curve, SEED + 1)) != toxic
    u, v, lq, h = qap_by_integers(curve, p, toxic)
    sec = rt.zkey_sections(keys[(curve_name, circuit)])
    n_inp = p["n_public"] + 1
    assert sec[5] == points_of(curve, G1, u)
    assert sec[6] == points_of(curve, G1, v)
    assert sec[3] == points_of(curve, G1, lq[:n_inp])
    assert sec[8] == points_of(curve, G1, lq[n_inp:])
    assert sec[9] == points_of(curve, G1, h)
    if circuit in G2_CHECKED:
        assert sec[7] == points_of(curve, G2, v)
    fq = 48 if curve == BLS12_381 else 32
    hdr = sec[2][4 + fq + 4 + 32 + 12:]
    tau, alpha, beta, gamma, delta = toxic
    want = points_of(curve, G1, [alpha, beta]) + points_of(curve, G2, [beta, gamma]) + points_of(curve, G1, [delta]) + points_of(curve, G2, [delta])
    assert hdr == want


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_proofs_on_the_new_key(keys, curve_name, circuit):
    curve = CURVES[curve_name]; mod = rt.modulus(curve)
    path = keys[(curve_name, circuit)]
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    z = orc.ZKey(curve, path)
    rng = np.random.default_rng(91)
    r, s = orc.random_field(curve, FR, 2, rng)
    proof = cg.prove_plain(curve, path, w, r, s)
    np.testing.assert_array_equal(proof, z.prove_plain(w, r, s))
    vk = cg.VerifyingKey.from_zkey(curve, path)
    r1 = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
    try:
        pub = w[1:1 + z.n_public]
        assert vk.verify(proof, pub)
        assert r1.check_witness(w) == (0, NO_ROW)
        if z.num_constraints:                                               # (sum_arrays has no constraint a witness could break)
            ints = rt.from_mont(curve, w); ints[-1] = (ints[-1] + 1) % mod
            bad = rt.to_mont(curve, ints)
            n_bad, first = r1.check_witness(bad)
            assert n_bad > 0 and first != NO_ROW
            assert not vk.verify(cg.prove_plain(curve, path, bad, r, s), pub)
    finally:
        vk.close(); r1.close(); z.close()


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_column_sums_on_the_skewed_circuit(curve):
    """cg_qap_columns_dev on the three matrices of the 4 099-row circuit against Python integers.  Wire 0's column of B has 1 367 entries (the
    workgroup sums it), the 512 output wires of rows with an empty C occur nowhere (empty columns), most columns hold one entry.  long_min:
    0 = the default (64: wire 0 and the busier base wires go to the workgroup), 1 = every non-empty column through the workgroup path,
    2^31 = every column summed by one lane; all three agree."""
    ensure_built()
    mod = rt.modulus(curve)
    n_wires, cons, _ = rt.skewed_circuit(curve)
    rng = np.random.default_rng(17)
    lag_m = orc.random_field(curve, FR, rt.ROWS, rng)
    lag = rt.from_mont(curve, lag_m)
    ctx = cg.Context(0)
    try:
        d_lag = ctx.to_device(lag_m)
        out = ctx.alloc(n_wires * 32)
        empty_everywhere = np.ones(n_wires, dtype=bool)
        for m in range(3):
            cols, col_ptr, rows, vals = rt.columns(cons, m, n_wires)
            lens = np.diff(col_ptr.astype(np.int64))
            empty_everywhere &= lens == 0
            if m == 1:
                assert lens[0] >= 1366
            assert (lens >= 64).sum() >= 1 and (lens == 0).sum() >= 300
            want = rt.to_mont(curve, [sum(v * lag[j] for j, v in col) % mod for col in cols])
            d_cp, d_rows, d_vals = ctx.to_device(col_ptr), ctx.to_device(rows), ctx.to_device(rt.to_mont(curve, vals))
            for long_min in (0, 1, 1 << 31):
                out.zero()
                ctx.qap_columns(curve, d_cp, d_rows, d_vals, n_wires, d_lag, out, long_min=long_min)
                ctx.sync()
                np.testing.assert_array_equal(out.download((n_wires, 4)), want, err_msg=f"matrix {m}, long_min {long_min}")
            ctx.free_many([d_cp, d_rows, d_vals])
        assert empty_everywhere.sum() >= 300
        ctx.free_many([d_lag, out])
    finally:
        ctx.close()
