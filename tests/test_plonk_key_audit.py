"""Is this key the key of my circuit?  cgh_plonk_session_audit on keys that must pass and on keys with one defect each: a mutation is applied
to a copy of a domain-8 or domain-64 fixture (plonk_audit_tools.patch_zkey; polynomial blocks that must stay self-consistent are recomputed
with Python integers) and the audit must set the named bits and leave the named bits clear.  Bits not named are free."""
import random
import struct

import pytest

import plonk_audit_tools as at
import plonk_setup_tools as pt
import r1cs_tools as rt
from oracle_lib import BN254, BLS12_381, G1, G2
from product import cg, ensure_built
from r1cs_tools import CURVES, NO_ROW

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
H, B, RW, SG, CM, SR, CI = (cg.PLONK_AUDIT_HEADER, cg.PLONK_AUDIT_BLOCKS, cg.PLONK_AUDIT_ROWS, cg.PLONK_AUDIT_SIGMA, cg.PLONK_AUDIT_COMMITMENTS,
                            cg.PLONK_AUDIT_SRS, cg.PLONK_AUDIT_CIRCUIT)
ALL = H | B | RW | SG | CM | SR | CI


def audit(curve, zkey, r1cs_path=None, seed=SEED):
    s = cg.PlonkSession(curve, zkey)
    r = cg.R1cs(curve, r1cs_path) if r1cs_path else None
    try:
        return s.audit(r1cs=r, seed=seed)
    finally:
        s.close()
        if r: r.close()


def names(bits):
    return [n for k, n in enumerate(cg.PLONK_AUDIT_NAMES) if bits >> k & 1]


def expect(result, must_set, must_clear):
    failed, detail = result
    assert failed & must_set == must_set and not failed & must_clear, f"set {names(failed)}: wanted {names(must_set)} set, {names(must_clear)} clear; detail {detail}"
    for k in range(len(cg.PLONK_AUDIT_NAMES)):
        assert (detail[k] == (None, None)) == (not failed >> k & 1), (k, detail[k])
    return detail


# ---- keys that must pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name,circuit", pt.PAIRS)
def test_shipped_pairs_pass_with_their_circuit(curve_name, circuit):
    ensure_built()
    res = audit(CURVES[curve_name], at.plonk_fx(curve_name, circuit, "circuit.zkey"), rt.fx(curve_name, circuit, "circuit.r1cs"))
    assert res == (0, [(None, None)] * 7)


@pytest.mark.parametrize("curve_name,circuit", at.FIXTURES)
def test_shipped_keys_pass_without_a_circuit(curve_name, circuit):
    ensure_built()
    for seed in (SEED, None):                                                         # a given seed, and OS entropy
        assert audit(CURVES[curve_name], at.plonk_fx(curve_name, circuit, "circuit.zkey"), seed=seed)[0] == 0


def test_compiled_branch_key_passes(tmp_path):
    """a setup_plonk key of the circuit that takes every branch of the gate compiler: domain 2^15"""
    ensure_built()
    curve = BN254; mod = rt.modulus(curve)
    n_wires, n_pub, cons, _ = pt.branch_circuit(curve)
    path, key = str(tmp_path / "branch.r1cs"), str(tmp_path / "branch.zkey")
    rt.write_r1cs(path, mod, n_wires, 0, n_pub, n_wires - 1 - n_pub, cons)
    r = cg.R1cs(curve, path)
    try:
        cg.setup_plonk(r, 77, key)
        assert r.plonk_info()["domain_size"] == 1 << 15
        s = cg.PlonkSession(curve, key)
        try:
            assert s.audit(r1cs=r, seed=SEED) == (0, [(None, None)] * 7)
        finally:
            s.close()
    finally:
        r.close()


def test_compiled_bls12_381_key_passes(tmp_path):
    ensure_built()
    curve = BLS12_381
    key, rp = str(tmp_path / "poseidon.zkey"), rt.fx("bls12_381", "poseidon", "circuit.r1cs")
    r = cg.R1cs(curve, rp)
    try:
        cg.setup_plonk(r, 78, key)
    finally:
        r.close()
    assert audit(curve, key, rp)[0] == 0


# ---- mutated keys -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("bn254", "kyc"), ("bls12_381", "kyc"), ("bn254", "multiplier2_example")], ids=lambda p: "-".join(p))
def fixture_key(request):
    ensure_built()
    curve_name, circuit = request.param
    curve = CURVES[curve_name]
    return dict(curve=curve, zkey=at.plonk_fx(curve_name, circuit, "circuit.zkey"), r1cs=rt.fx(curve_name, circuit, "circuit.r1cs"),
                key=at.Key(curve, at.plonk_fx(curve_name, circuit, "circuit.zkey")), name=(curve_name, circuit))


def mutate(fx, tmp_path, replace):
    return at.patch_zkey(fx["zkey"], str(tmp_path / "mutated.zkey"), replace)


def with_row_changed(fx, section, row):
    key = fx["key"]
    rows = at.rows_of_block(fx["curve"], key.sec[section], key.n)
    rows[row] = (rows[row] + 12345) % key.r
    return at.block_from_rows(fx["curve"], rows)


def test_one_stored_evaluation_changed(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]
    off = (key.n + 5) * 32                                                             # evaluation 5 of Ql; the coefficients stay
    sec = at.splice(key.sec[8], off, rt.to_mont(fx["curve"], [99]).tobytes())
    assert sec != key.sec[8]
    z = mutate(fx, tmp_path, {8: sec})
    detail = expect(audit(fx["curve"], z), B, ALL & ~B)
    assert detail[1] == (1, 5)
    expect(audit(fx["curve"], z, fx["r1cs"]), B, ALL & ~B)


def test_selector_changed_on_a_gate_row(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]
    row = key.nc - 1
    z = mutate(fx, tmp_path, {8: with_row_changed(fx, 8, row)})
    detail = expect(audit(fx["curve"], z), CM, B | RW | SG | SR)
    assert detail[4] == (1, None)
    detail = expect(audit(fx["curve"], z, fx["r1cs"]), CM | CI, B | RW | SG | SR)
    assert detail[6] == (8, row)


def test_selector_changed_on_a_padding_row(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]
    row = key.nc + 1
    z = mutate(fx, tmp_path, {9: with_row_changed(fx, 9, row)})
    detail = expect(audit(fx["curve"], z), RW | CM, 0)
    assert detail[2] == (2, row)
    # and a witness check on that key names the row: a padding row fails for every witness
    w, _ = at.read_witness(fx["curve"], at.plonk_fx(*fx["name"], "witness.wtns"))
    s = cg.PlonkSession(fx["curve"], z)
    try:
        assert s.check_witness(w) == (0, NO_ROW)                                       # (qr of a padding row multiplies b = 0: only qc fails it)
    finally:
        s.close()
    z = mutate(fx, tmp_path, {11: with_row_changed(fx, 11, row)})
    s = cg.PlonkSession(fx["curve"], z)
    try:
        assert s.check_witness(w) == (1, row)
    finally:
        s.close()


def sigma_blocks(key):
    n = key.n
    return [key.sec[12][w * 5 * n * 32:(w + 1) * 5 * n * 32] for w in range(3)]


def test_two_sigma_labels_exchanged(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    blocks = sigma_blocks(key)
    rows = [at.rows_of_block(curve, b, key.n) for b in blocks]
    i, j = 0, key.nc - 1                                                               # column a: rows of different wires
    assert key.maps[0][i] != key.maps[0][j] and rows[0][i] != rows[0][j]
    rows[0][i], rows[0][j] = rows[0][j], rows[0][i]
    z = mutate(fx, tmp_path, {12: at.block_from_rows(curve, rows[0]) + blocks[1] + blocks[2]})
    detail = expect(audit(curve, z), SG | CM, B | SR)
    assert detail[3] == (5, 0) and detail[4] == (5, None)


def test_one_map_entry_changed(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]
    row = key.nc - 1
    other = next(wire for wire in range(1, key.n_vars) if wire != key.maps[1][row])
    sec = at.splice(key.sec[5], 4 * row, struct.pack("<I", other))
    z = mutate(fx, tmp_path, {5: sec})
    detail = expect(audit(fx["curve"], z), SG, CM | B | SR)
    assert detail[3][0] in (5, 6, 7)
    detail = expect(audit(fx["curve"], z, fx["r1cs"]), SG | CI, CM | B | SR)
    assert detail[6] == (5, row)


def test_header_commitment_doubled(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    fq = at.fq_bytes(curve)
    which = 4 if any(key.vk[4 * 2 * fq:5 * 2 * fq]) else 1                            # Qc; Ql where Qc is the point at infinity (the domain-8 circuits)
    off = at.header_offsets(curve)["vk"] + which * 2 * fq
    new = at.double_point(cg, curve, G1, key.sec[2][off:off + 2 * fq])
    z = mutate(fx, tmp_path, {2: at.splice(key.sec[2], off, new)})
    detail = expect(audit(curve, z, fx["r1cs"]), CM, ALL & ~CM)
    assert detail[4] == (which, None)


def test_srs_point_doubled(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    fq = at.fq_bytes(curve)
    new = at.double_point(cg, curve, G1, key.sec[14][3 * 2 * fq:4 * 2 * fq])
    z = mutate(fx, tmp_path, {14: at.splice(key.sec[14], 3 * 2 * fq, new)})
    detail = expect(audit(curve, z), SR, 0)
    assert detail[5] == (1, None)
    # p_tau[0] replaced: the generator test names it
    new0 = at.double_point(cg, curve, G1, key.sec[14][:2 * fq])
    detail = expect(audit(curve, mutate(fx, tmp_path, {14: at.splice(key.sec[14], 0, new0)})), SR, 0)
    assert detail[5] == (0, 0)


def test_x2_doubled(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    fq = at.fq_bytes(curve)
    off = at.header_offsets(curve)["x2"]
    new = at.double_point(cg, curve, G2, key.sec[2][off:off + 4 * fq])
    z = mutate(fx, tmp_path, {2: at.splice(key.sec[2], off, new)})
    expect(audit(curve, z, fx["r1cs"]), SR, ALL & ~SR)


def test_k1_replaced(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    off = at.header_offsets(curve)["k1"]
    z = mutate(fx, tmp_path, {2: at.splice(key.sec[2], off, rt.to_mont(curve, [5]).tobytes())})
    detail = expect(audit(curve, z), H, 0)
    assert detail[0] == (2, 0)


def test_lagrange_block_of_the_wrong_row(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]; curve = fx["curve"]
    size = 5 * key.n * 32
    wrong = at.block_from_rows(curve, [int(i == 1) for i in range(key.n)])           # L_1 where L_0 belongs
    assert wrong == key.sec[13][size:2 * size]
    z = mutate(fx, tmp_path, {13: wrong + key.sec[13][size:]})
    detail = expect(audit(curve, z), RW, B)
    assert detail[2] == (8, 0)


def test_key_of_another_circuit(fixture_key):
    fx = fixture_key
    curve_name = fx["name"][0]
    other = "sum_arrays" if curve_name == "bn254" and fx["name"][1] != "sum_arrays" else "kyc"
    if (curve_name, other) == fx["name"]:
        other = "multiplier2"
    detail = expect(audit(fx["curve"], fx["zkey"], rt.fx(curve_name, other, "circuit.r1cs")), CI, H | B | RW | SG | CM | SR)
    assert detail[6][0] == 2
    # a circuit over the other curve: the bit, not an error
    cross = "bls12_381" if curve_name == "bn254" else "bn254"
    s = cg.PlonkSession(fx["curve"], fx["zkey"]); r = cg.R1cs(CURVES[cross], rt.fx(cross, "kyc", "circuit.r1cs"))
    try:
        assert s.audit(r1cs=r, seed=SEED)[0] == CI
    finally:
        s.close(); r.close()


def test_sizes_without_meaning_are_an_error(fixture_key, tmp_path):
    fx = fixture_key; key = fx["key"]
    sec = at.splice(key.sec[4], 0, struct.pack("<I", key.n_vars))                      # a map entry that is no variable
    s = cg.PlonkSession(fx["curve"], mutate(fx, tmp_path, {4: sec}))
    try:
        with pytest.raises(cg.BackendError, match="names wire"):
            s.audit()
    finally:
        s.close()


# ---- the two halves together -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
def test_a_changed_addition_factor(curve_name, tmp_path):
    """nothing but the circuit pins the additions: the audit without the .r1cs passes, with it CIRCUIT names section 3 and the addition, and
    the honest witness breaks the rows that read the addition - the restatement's rows, its own gate first"""
    ensure_built()
    curve = CURVES[curve_name]
    src = at.plonk_fx(curve_name, "kyc", "circuit.zkey")
    key = at.Key(curve, src)
    a = 7
    off = 72 * a + 8                                                                   # f1 of addition 7
    sec = at.splice(key.sec[3], off, rt.to_mont(curve, [key.adds[a][2] + 1]).tobytes())
    z = at.patch_zkey(src, str(tmp_path / "adds.zkey"), {3: sec})
    assert audit(curve, z)[0] == 0
    detail = expect(audit(curve, z, rt.fx(curve_name, "kyc", "circuit.r1cs")), CI, H | B | RW | SG | CM | SR)
    assert detail[6] == (3, a)
    w, w_ints = at.read_witness(curve, at.plonk_fx(curve_name, "kyc", "witness.wtns"))
    bad = at.Key(curve, z).bad_rows(w_ints)
    gate_row = next(i for i in range(key.nc) if key.maps[2][i] == key.n_vars - key.n_add + a)
    assert bad and bad[0] == gate_row
    s = cg.PlonkSession(curve, z)
    try:
        assert s.check_witness(w) == (len(bad), gate_row)
    finally:
        s.close()
