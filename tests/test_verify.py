"""Groth16 verification in the product (cgh_vk_*, cgh_groth16_verify, cgh_groth16_verify_batch, cgh_session_verify) against the oracle's
verifier: the shipped snarkjs proofs and their tampered variants on the host, randomised batches with per-proof verdicts on the GPU."""
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, G1, G2
from product import cg, ensure_built

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = {"bn254": BN254, "bls12_381": BLS12_381}
WITH_PROOF = [(c, k) for c in CURVES for k in ("multiplier2", "poseidon")]


def fx(curve_name, circuit, name):
    return os.path.join(GOLDEN, "groth16", curve_name, circuit, name)


def nq(curve):
    return 6 if curve == BLS12_381 else 4


def split(curve, proof):
    q = nq(curve)
    return proof[:2 * q].copy(), proof[2 * q:6 * q].copy(), proof[6 * q:].copy()


def neg_affine(curve, group, pt):
    return cg.point_to_affine(curve, group, cg.point_neg(curve, group, cg.point_from_affine(curve, group, pt)))


def add_affine(curve, group, a, b):
    return cg.point_to_affine(curve, group, cg.point_add(curve, group, cg.point_from_affine(curve, group, a), cg.point_from_affine(curve, group, b)))


def fixture(curve_name, circuit):
    curve = CURVES[curve_name]
    return (curve, orc.vk_from_json(curve, fx(curve_name, circuit, "verification_key.json")), orc.proof_from_json(curve, fx(curve_name, circuit, "circom.proof")),
            orc.public_from_json(curve, fx(curve_name, circuit, "public.json")))


def all_verification_keys():
    out = []
    for cn in CURVES:
        base = os.path.join(GOLDEN, "groth16", cn)
        out += [(cn, d) for d in sorted(os.listdir(base)) if os.path.exists(os.path.join(base, d, "verification_key.json"))]
    return out


@pytest.mark.parametrize("curve_name,circuit", all_verification_keys())
def test_prepared_alphabeta_equals_the_files_value(curve_name, circuit):
    """e(alpha, beta) is computed when the handle opens; it equals `vk_alphabeta_12` of the file limb for limb"""
    ensure_built()
    curve = CURVES[curve_name]
    path = fx(curve_name, circuit, "verification_key.json")
    vk = cg.VerifyingKey.from_json(curve, path)
    ab = json.load(open(path))["vk_alphabeta_12"]
    want = np.stack([np.stack([np.stack([orc.from_dec(curve, orc.FQ, ab[i][j][k]) for k in range(2)]) for j in range(3)]) for i in range(2)])
    np.testing.assert_array_equal(vk.alphabeta(), want)
    assert vk.n_public == json.load(open(path))["nPublic"]
    vk.close()


@pytest.mark.parametrize("curve_name,circuit", WITH_PROOF)
def test_single_proof_verdicts_match_the_oracle(curve_name, circuit):
    ensure_built()
    curve, ovk, proof, pub = fixture(curve_name, circuit)
    handles = [cg.VerifyingKey.from_json(curve, fx(curve_name, circuit, "verification_key.json")), cg.VerifyingKey.from_zkey(curve, fx(curve_name, circuit, "circuit.zkey"))]
    np.testing.assert_array_equal(handles[0].alphabeta(), handles[1].alphabeta())
    a, b, c = split(curve, proof)
    pub_plus = pub.copy(); pub_plus[0] = orc.field_op(curve, FR, "add", pub[0], orc.from_dec(curve, FR, 1))
    cases = {
        "shipped": (proof, pub, True),
        "public input + 1": (proof, pub_plus, False),
        "A and C exchanged": (np.concatenate([c, b, a]), pub, False),
        "B negated": (np.concatenate([a, neg_affine(curve, G2, b), c]), pub, False),
    }
    for name, (pf, pb, want) in cases.items():
        assert orc.verify(curve, ovk, pb, pf) == want, name
        for vk in handles:
            assert vk.verify(pf, pb) == want, name
    # a proof of the other circuit under this key
    other = "poseidon" if circuit == "multiplier2" else "multiplier2"
    _, other_vk, other_proof, other_pub = fixture(curve_name, other)
    if len(other_vk["ic"]) != len(ovk["ic"]):
        for vk in handles:
            with pytest.raises(cg.BackendError, match="public inputs"):
                vk.verify(other_proof, other_pub)
    else:
        assert not orc.verify(curve, ovk, other_pub, other_proof)
        for vk in handles:
            assert not vk.verify(other_proof, other_pub)
    # error statuses, not verdicts: a wrong count, a public input that is not below the modulus
    for vk in handles:
        with pytest.raises(cg.BackendError, match="public inputs"):
            vk.verify(proof, np.concatenate([pub, pub]))
        bad = pub.copy(); bad[0] = orc.int_to_limbs(orc.MODULI[(curve, FR)], 4)
        with pytest.raises(cg.BackendError, match="modulus"):
            vk.verify(proof, bad)
    # a proof point (x, y + 1) off the curve: ok = 0, no crash; for each of the three points
    one_q = orc.from_dec(curve, orc.FQ, 1); q = nq(curve)
    for lo in (q, 4 * q, 7 * q):                         # y of A, y.c0 of B, y of C
        off = proof.copy(); off[lo:lo + q] = orc.field_op(curve, orc.FQ, "add", proof[lo:lo + q], one_q)
        for vk in handles:
            assert not vk.verify(off, pub)
    for vk in handles:
        vk.close()


def test_multiplier2_wire_order_is_one_product_a_b():
    """the witnesses the batch tests make are [1, a b, a, b]: the fixture's own witness has that shape, and the oracle proves and
    verifies one made that way"""
    check_wire_order("bn254")


def test_multiplier2_wire_order_on_bls12_381():
    """the BLS12-381 batch relies on the same wire order"""
    check_wire_order("bls12_381")


def check_wire_order(curve_name):
    curve = CURVES[curve_name]
    w = orc.read_wtns(curve, fx(curve_name, "multiplier2", "witness.wtns"))
    assert w.shape[0] == 4
    np.testing.assert_array_equal(w[0], orc.from_dec(curve, FR, 1))
    np.testing.assert_array_equal(w[1], orc.field_op(curve, FR, "mul", w[2], w[3]))
    z = orc.ZKey(curve, fx(curve_name, "multiplier2", "circuit.zkey"))
    rng = np.random.default_rng(4)
    wit = make_witness(curve, rng)
    r, s = orc.random_field(curve, FR, 2, rng)
    ovk = orc.vk_from_json(curve, fx(curve_name, "multiplier2", "verification_key.json"))
    assert orc.verify(curve, ovk, wit[1:2], z.prove_plain(wit, r, s))


def make_witness(curve, rng):
    a, b = orc.random_field(curve, FR, 2, rng)
    return np.stack([orc.from_dec(curve, FR, 1), orc.field_op(curve, FR, "mul", a, b), a, b])


# ---- GPU: batches ------------------------------------------------------------------------------------------------------------------
_made = {}


def proofs_of_multiplier2(curve_name, n):
    """n proofs by the product's plain prover on one session, distinct (r, s), distinct witnesses [1, a b, a, b]; made once per curve"""
    have = _made.get(curve_name)
    if have is None or have[0].shape[0] < n:
        curve = CURVES[curve_name]
        rng = np.random.default_rng(1234 + curve)
        sess = cg.ProvingSession(curve, fx(curve_name, "multiplier2", "circuit.zkey"), precompute=False)
        proofs, pubs = [], []
        for _ in range(n):
            w = make_witness(curve, rng)
            r, s = orc.random_field(curve, FR, 2, rng)
            proofs.append(sess.prove_plain(w, r, s)[0]); pubs.append(w[1:2])
        sess.close()
        have = _made[curve_name] = (np.stack(proofs), np.stack(pubs))
    return have[0][:n].copy(), have[1][:n].copy()


@pytest.fixture(scope="module")
def keys():
    ensure_built()
    ks = {cn: cg.VerifyingKey.from_json(CURVES[cn], fx(cn, "multiplier2", "verification_key.json")) for cn in CURVES}
    yield ks
    for k in ks.values():
        k.close()


SEED = bytes(range(32))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,n", [("bn254", 1), ("bn254", 2), ("bn254", 65), ("bn254", 200), ("bls12_381", 65)])
def test_batch_of_valid_proofs_is_accepted(keys, curve_name, n):
    proofs, pubs = proofs_of_multiplier2(curve_name, n)
    ok, flags = keys[curve_name].verify_batch(proofs, pubs, seed=SEED, per_proof=True)
    assert ok and flags.all() and flags.shape == (n,)
    assert keys[curve_name].verify_batch(proofs, pubs, seed=SEED) is True                # a fixed seed: the same verdict again
    assert keys[curve_name].verify_batch(proofs, pubs)                                   # coefficients from OS entropy
    if n == 1:
        assert keys[curve_name].verify_batch(proofs[:0], pubs[:0])                       # an empty batch accepts
        ovk = orc.vk_from_json(CURVES[curve_name], fx(curve_name, "multiplier2", "verification_key.json"))
        assert orc.verify(CURVES[curve_name], ovk, pubs[0], proofs[0]) and keys[curve_name].verify(proofs[0], pubs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_tampered_proof_is_found(keys, where):
    curve = BN254; n = 65
    proofs, pubs = proofs_of_multiplier2("bn254", n)
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    pubs[i, 0] = orc.field_op(curve, FR, "add", pubs[i, 0], orc.from_dec(curve, FR, 1))
    ok, flags = keys["bn254"].verify_batch(proofs, pubs, seed=SEED, per_proof=True)
    assert not ok
    assert list(np.flatnonzero(~flags)) == [i]
    ovk = orc.vk_from_json(curve, fx("bn254", "multiplier2", "verification_key.json"))
    assert not orc.verify(curve, ovk, pubs[i], proofs[i])
    for j in ((i + 1) % n, (i + 7) % n):
        assert orc.verify(curve, ovk, pubs[j], proofs[j])
    assert keys["bn254"].verify_batch(proofs, pubs, seed=SEED) is False                  # a fixed seed: the same verdict again


@pytest.mark.gpu
def test_cancelling_pair_is_rejected_and_both_are_flagged(keys):
    """C_i + D and C_j - D: each proof alone is invalid and the UNWEIGHTED product of the n equations holds; only distinct coefficients
    r_i != r_j tell (this is the test that fails if the coefficients are constant)"""
    curve = BN254; n = 65; i, j = 5, 40
    proofs, pubs = proofs_of_multiplier2("bn254", n)
    D = orc.generator_mul(curve, G1, orc.random_field(curve, FR, 1, np.random.default_rng(99))[0])
    q = nq(curve)
    proofs[i, 6 * q:] = add_affine(curve, G1, proofs[i, 6 * q:], D)
    proofs[j, 6 * q:] = add_affine(curve, G1, proofs[j, 6 * q:], neg_affine(curve, G1, D))
    # the unweighted product is one: sum of the C points unchanged
    ovk = orc.vk_from_json(curve, fx("bn254", "multiplier2", "verification_key.json"))
    assert not orc.verify(curve, ovk, pubs[i], proofs[i]) and not orc.verify(curve, ovk, pubs[j], proofs[j])
    ok, flags = keys["bn254"].verify_batch(proofs, pubs, seed=SEED, per_proof=True)
    assert not ok
    assert list(np.flatnonzero(~flags)) == [i, j]
    assert keys["bn254"].verify_batch(proofs, pubs, seed=SEED) is False                  # the same seed, the same coefficients, the same verdict
    assert keys["bn254"].verify_batch(proofs, pubs, seed=bytes(32)) is False             # and another seed rejects too
    ok2, flags2 = keys["bn254"].verify_batch(proofs, pubs, per_proof=True)              # OS entropy: the same verdict
    assert not ok2 and list(np.flatnonzero(~flags2)) == [i, j]


@pytest.mark.gpu
def test_b_outside_the_g2_subgroup_is_rejected(keys):
    from test_gpu_parity import off_subgroup_point
    curve = BN254; n = 2
    proofs, pubs = proofs_of_multiplier2("bn254", n)
    q = nq(curve)
    bad = off_subgroup_point(curve, G2)
    assert orc.on_curve(curve, G2, bad) and not cg.point_validate(curve, G2, bad)
    proofs[1, 2 * q:6 * q] = bad
    ok, flags = keys["bn254"].verify_batch(proofs, pubs, seed=SEED, per_proof=True)
    assert not ok and list(flags) == [True, False]
    assert not keys["bn254"].verify(proofs[1], pubs[1])


@pytest.mark.gpu
def test_session_verifies_the_proof_it_has_just_made():
    ensure_built()
    curve = BN254
    w = orc.read_wtns(curve, fx("bn254", "poseidon", "witness.wtns"))
    sess = cg.ProvingSession(curve, fx("bn254", "poseidon", "circuit.zkey"), precompute=False)
    rng = np.random.default_rng(8)
    r, s = orc.random_field(curve, FR, 2, rng)
    proof, _ = sess.prove_plain(w, r, s)
    n_pub = sess.info["n_public"]
    assert sess.verify(proof, w[1:1 + n_pub])
    bad = w[1:1 + n_pub].copy(); bad[0] = orc.field_op(curve, FR, "add", bad[0], orc.from_dec(curve, FR, 1))
    assert not sess.verify(proof, bad)
    sess.close()
