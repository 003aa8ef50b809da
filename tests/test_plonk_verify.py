"""Plonk verification in the product (cgh_plonk_vk_*, cgh_plonk_verify, cgh_plonk_verify_batch, cgh_plonk_session_verify and the per-proof
layer cg_plonk_verify_scalars / cg_g1_lincomb_batch) against the oracle's verifier and an independent restatement of the scalar algebra:
keys, the shipped snarkjs proofs and their tampered variants and every fixture circuit on the host; the scalar kernel, the linear
combinations, randomised batches with per-proof verdicts and the session entry on the GPU."""
import glob
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR, FQ, G1, PLONK_COMMITS, PLONK_EVALS
from product import cg, ensure_built

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = {"bn254": BN254, "bls12_381": BLS12_381}
KEY_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")


def fx(curve_name, circuit, name):
    return os.path.join(GOLDEN, "plonk", curve_name, circuit, name)


def nq(curve):
    return 6 if curve == BLS12_381 else 4


def all_keys():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "plonk", "*", "*", "verification_key.json"))):
        circuit = os.path.basename(os.path.dirname(p)); cn = os.path.basename(os.path.dirname(os.path.dirname(p)))
        out.append((cn, circuit))
    return out


def F(curve, op, a, b):
    return orc.field_op(curve, FR, op, a, b)


def plus_one(curve, x):
    return F(curve, "add", x, orc.from_dec(curve, FR, 1))


def limbs_plus(limbs, modulus):
    """the limbs of (value of limbs) + modulus: the same residue, not reduced"""
    v = sum(int(x) << (64 * i) for i, x in enumerate(limbs)) + modulus
    assert v < 1 << (64 * len(limbs))
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(len(limbs))], dtype=np.uint64)


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name,circuit", all_keys())
def test_json_and_zkey_handles_agree_with_the_oracle(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]
    js = json.load(open(fx(curve_name, circuit, "verification_key.json")))
    a = cg.PlonkVerifyingKey.from_json(curve, fx(curve_name, circuit, "verification_key.json"))
    b = cg.PlonkVerifyingKey.from_zkey(curve, fx(curve_name, circuit, "circuit.zkey"))
    fa, fb = a.fields(), b.fields()
    want = orc.plonk_zkey_vk(curve, fx(curve_name, circuit, "circuit.zkey"))
    for k in KEY_POINTS + ("X_2", "k1", "k2"):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
        np.testing.assert_array_equal(fa[k], want[k], err_msg=k)
    np.testing.assert_array_equal(fa["w"], fb["w"])
    np.testing.assert_array_equal(fa["w"], orc.from_dec(curve, FR, js["w"]))
    np.testing.assert_array_equal(fa["w"], orc.roots_of_unity(curve)[1][js["power"]])
    assert (a.n_public, a.power) == (b.n_public, b.power) == (js["nPublic"], js["power"])
    a.close(); b.close()


def test_opening_a_wrong_key_is_an_error(tmp_path):
    ensure_built()
    good = fx("bn254", "multiplier2", "verification_key.json")
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_json(BN254, os.path.join(GOLDEN, "groth16", "bn254", "multiplier2", "verification_key.json"))
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_zkey(BN254, os.path.join(GOLDEN, "groth16", "bn254", "multiplier2", "circuit.zkey"))
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_json(BLS12_381, good)
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_json(BN254, fx("bls12_381", "multiplier2", "verification_key.json"))
    js = json.load(open(good))
    roots = orc.roots_of_unity(BN254)[1]
    js["w"] = orc.to_dec(BN254, FR, roots[js["power"] + 1])                              # a root of unity, of another order
    bad = tmp_path / "other_root.json"; bad.write_text(json.dumps(js))
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_json(BN254, str(bad))
    js = json.load(open(good)); js["power"] = 29                                          # beyond BN254's two-adicity (28)
    bad = tmp_path / "power.json"; bad.write_text(json.dumps(js))
    with pytest.raises(cg.BackendError):
        cg.PlonkVerifyingKey.from_json(BN254, str(bad))


# ---- verdicts with snarkjs' own proofs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name", list(CURVES))
def test_snarkjs_proof_verdicts_match_the_oracle(curve_name):
    ensure_built()
    curve = CURVES[curve_name]
    zp = fx(curve_name, "multiplier2", "circuit.zkey")
    proof = orc.plonk_proof_from_json(curve, fx(curve_name, "multiplier2", "circom.proof"))
    pub = orc.public_from_json(curve, fx(curve_name, "multiplier2", "public.json"))
    handles = [cg.PlonkVerifyingKey.from_json(curve, fx(curve_name, "multiplier2", "verification_key.json")), cg.PlonkVerifyingKey.from_zkey(curve, zp)]
    other = orc.generator_mul(curve, G1, orc.from_dec(curve, FR, 7))
    cases = {"shipped": (proof, pub, True)}
    for k in PLONK_COMMITS:                                                                 # another valid point in its place
        bad = dict(proof); bad[k] = other
        cases["commitment " + k] = (bad, pub, False)
    for k in PLONK_EVALS:
        bad = dict(proof); bad[k] = plus_one(curve, proof[k])
        cases[k + " + 1"] = (bad, pub, False)
    for j in range(pub.shape[0]):
        p2 = pub.copy(); p2[j] = plus_one(curve, pub[j])
        cases[f"public input {j} + 1"] = (proof, p2, False)
    assert len(cases) == 1 + 9 + 6 + pub.shape[0]
    for name, (pr, pb, want) in cases.items():
        assert orc.plonk_verify(curve, zp, pr, pb) is want, name
        for vk in handles:
            assert vk.verify(pr, pb) is want, name
    # what the reference's proof parser refuses: the product says 0, it does not raise
    q = nq(curve)
    bad = dict(proof); bad["a"] = proof["a"].copy(); bad["a"][q:] = limbs_plus(proof["a"][q:], orc.MODULI[(curve, FQ)])
    assert handles[0].verify(bad, pub) is False
    bad = dict(proof); bad["eval_zw"] = limbs_plus(proof["eval_zw"], orc.MODULI[(curve, FR)])
    assert handles[0].verify(bad, pub) is False
    from test_gpu_parity import off_subgroup_point
    bad = dict(proof); bad["z"] = off_subgroup_point(BLS12_381, G1) if curve == BLS12_381 else np.concatenate([proof["z"][:q], proof["a"][q:]])   # outside the subgroup / off the curve
    assert handles[0].verify(bad, pub) is False
    # error statuses, not verdicts
    with pytest.raises(cg.BackendError):
        handles[0].verify(proof, pub[:1])
    with pytest.raises(cg.BackendError):
        handles[0].verify(proof, np.concatenate([pub, pub[:1]]))
    p2 = pub.copy(); p2[0] = limbs_plus(pub[0], orc.MODULI[(curve, FR)])
    with pytest.raises(cg.BackendError):
        handles[0].verify(proof, p2)
    for vk in handles:
        vk.close()


@pytest.mark.parametrize("curve_name,circuit", all_keys())
def test_every_fixture_circuit_proves_and_verifies(curve_name, circuit):
    """nPublic 2, 4, 6; power 3 and 6; both curves: the oracle's plain prover on the committed witness, the product's host verifier"""
    ensure_built()
    curve = CURVES[curve_name]
    zp = fx(curve_name, circuit, "circuit.zkey")
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    info = orc.plonk_zkey_info(curve, zp)
    npub = info["n_public"]
    w = w[:info["n_vars"] - info["n_additions"]]
    proof = orc.plonk_prove_plain(curve, zp, w, orc.random_field(curve, FR, 11, np.random.default_rng(8)), upto=5)
    pub = w[1:npub + 1]
    vk = cg.PlonkVerifyingKey.from_json(curve, fx(curve_name, circuit, "verification_key.json"))
    assert vk.n_public == npub
    assert orc.plonk_verify(curve, zp, proof, pub) and vk.verify(proof, pub)
    wrong = pub.copy(); wrong[npub - 1] = plus_one(curve, wrong[npub - 1])
    assert not vk.verify(proof, wrong) and not orc.plonk_verify(curve, zp, proof, wrong)
    vk.close()


# ---- the scalars against an independent restatement -------------------------------------------------------------------------------------
def random_points(curve, n, rng):
    return np.stack([orc.generator_mul(curve, G1, k) for k in orc.random_field(curve, FR, n, rng)])


def random_case(curve, n_pub, power, n, seed, key_infinities=0):
    """a random key and n random (not valid) proofs: the scalars are functions of the bytes, not of validity"""
    rng = np.random.default_rng(seed)
    pool = random_points(curve, 12, rng)
    kp = pool[:8].copy()
    for i in range(key_infinities):
        kp[2 + 2 * i] = 0                                                                  # Qr, Qc
    k1, k2 = orc.random_field(curve, FR, 2, rng)
    key = dict(points=kp, k1=k1, k2=k2, omega=orc.roots_of_unity(curve)[1][power], power=power)
    commits = pool[rng.integers(0, 12, size=(n, 9))]
    evals = orc.random_field(curve, FR, n * 6, rng).reshape(n, 6, 4)
    pubs = orc.random_field(curve, FR, max(1, n * n_pub), rng)[:n * n_pub].reshape(n, n_pub, 4)
    return key, commits, evals, pubs


def restate(curve, key, commits, evals, pubs):
    """plonk.rs:47-271 from the oracle's transcript and field operations: (6 challenges, 11 proof-point scalars, 9 key-point scalars)"""
    add = lambda a, b: F(curve, "add", a, b); sub = lambda a, b: F(curve, "sub", a, b); mul = lambda a, b: F(curve, "mul", a, b)
    inv = lambda a: orc.field_inverse(curve, FR, a)
    one = orc.from_dec(curve, FR, 1); zero = np.zeros(4, dtype=np.uint64)
    S = lambda x: ("scalar", x); P = lambda x: ("point", x)
    T = lambda items: orc.plonk_transcript(curve, items)
    ea, eb, ec, es1, es2, ezw = evals
    beta = T([P(p) for p in key["points"]] + [S(p) for p in pubs] + [P(commits[i]) for i in range(3)])
    gamma = T([S(beta)])
    alpha = T([S(beta), S(gamma), P(commits[3])])
    xi = T([S(alpha)] + [P(commits[i]) for i in (4, 5, 6)])
    v = T([S(xi)] + [S(e) for e in evals])
    u = T([P(commits[7]), P(commits[8])])
    xin, n = xi, one
    for _ in range(key["power"]):
        xin = mul(xin, xin); n = add(n, n)
    zh = sub(xin, one)
    ls, w = [], one
    for _ in range(max(1, pubs.shape[0])):
        ls.append(mul(mul(w, zh), inv(mul(n, sub(xi, w))))); w = mul(w, key["omega"])
    pi = zero
    for p, l in zip(pubs, ls):
        pi = sub(pi, mul(l, p))
    e2 = mul(mul(alpha, alpha), ls[0])
    e3a = add(add(ea, mul(es1, beta)), gamma); e3b = add(add(eb, mul(es2, beta)), gamma); e3c = add(ec, gamma)
    e3 = mul(mul(mul(mul(e3a, e3b), e3c), ezw), alpha)
    r0 = sub(sub(pi, e2), e3)
    bx = mul(beta, xi)
    d2a = mul(mul(mul(add(add(ea, bx), gamma), add(add(eb, mul(bx, key["k1"])), gamma)), add(add(ec, mul(bx, key["k2"])), gamma)), alpha)
    vs = [v]
    for _ in range(4):
        vs.append(mul(vs[-1], v))
    e = sub(add(add(add(add(add(mul(vs[0], ea), mul(vs[1], eb)), mul(vs[2], ec)), mul(vs[3], es1)), mul(vs[4], es2)), mul(u, ezw)), r0)
    neg = lambda x: sub(zero, x)
    nzh = neg(zh)
    sp = [one, u, vs[0], vs[1], vs[2], add(add(d2a, e2), u), nzh, mul(nzh, xin), mul(mul(nzh, xin), xin), xi, mul(mul(u, xi), key["omega"])]
    sk = [mul(ea, eb), ea, eb, ec, one, vs[3], vs[4], neg(mul(mul(mul(mul(e3a, e3b), alpha), beta), ezw)), neg(e)]
    return np.stack([beta, gamma, alpha, xi, v, u]), np.stack(sp), np.stack(sk)


# (curve, n_pub, power, key points at infinity).  BN254 n_pub 12 and BLS12-381 n_pub 1 make the first transcript a whole number of 136-byte
# blocks (8 x 136 = 1 088 bytes): the padding block stands alone.  n_pub 0: L_0 is still needed.
SHAPES = [(BN254, 0, 3, 0), (BN254, 1, 3, 0), (BN254, 2, 3, 2), (BN254, 12, 4, 0), (BLS12_381, 0, 3, 0), (BLS12_381, 1, 3, 0), (BLS12_381, 6, 3, 2),
          (BN254, 2, 0, 0), (BN254, 2, 16, 0), (BLS12_381, 2, 16, 0)]


def first_transcript_bytes(curve, n_pub):
    return 11 * 2 * 8 * nq(curve) + 32 * n_pub                                             # 8 key points, 3 commitments, n_pub scalars


def test_the_shapes_cover_the_hash_and_the_loop():
    """the cases the comparison below is for are really among SHAPES, and the host twin gets the block-boundary ones right: a transcript of
    exactly 8 blocks differs from the oracle's unless the padding block is absorbed on its own"""
    ensure_built()
    boundary = [(c, p) for c, p, _, _ in SHAPES if first_transcript_bytes(c, p) % 136 == 0]
    assert (BN254, 12) in boundary and (BLS12_381, 1) in boundary and first_transcript_bytes(BN254, 12) == first_transcript_bytes(BLS12_381, 1) == 8 * 136
    assert {(c, p) for c, p, _, _ in SHAPES} >= {(BN254, 0), (BN254, 1), (BN254, 2), (BN254, 12), (BLS12_381, 0), (BLS12_381, 1), (BLS12_381, 6)}
    assert {w for _, _, w, _ in SHAPES} >= {0, 16} and any(i == 2 for _, _, _, i in SHAPES)
    for curve, n_pub in boundary:
        key, commits, evals, pubs = random_case(curve, n_pub, 3, 1, 7)
        got = cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs)
        beta = orc.plonk_transcript(curve, [("point", p) for p in key["points"]] + [("scalar", p) for p in pubs[0]] + [("point", commits[0, i]) for i in range(3)])
        np.testing.assert_array_equal(got["challenges"][0, 0], beta)


@pytest.mark.parametrize("curve,n_pub,power,infs", SHAPES)
def test_host_scalars_equal_the_restatement(curve, n_pub, power, infs):
    ensure_built()
    n = 2
    key, commits, evals, pubs = random_case(curve, n_pub, power, n, 100 + 7 * n_pub + power + curve, infs)
    got = cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs)
    assert list(got["valid"]) == [1] * n
    sums = np.zeros((9, 4), dtype=np.uint64)
    for i in range(n):
        ch, sp, sk = restate(curve, key, commits[i], evals[i], pubs[i])
        np.testing.assert_array_equal(got["challenges"][i], ch)
        np.testing.assert_array_equal(got["proof_scalars"][i], sp)
        np.testing.assert_array_equal(got["key_scalars"][i], sk)
        sums = F(curve, "add", sums, sk)
    np.testing.assert_array_equal(got["key_sums"], sums)
    # with a coefficient, every scalar is r times the one without; the challenges are untouched
    rng = np.random.default_rng(5)
    coeff = rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64) * 2 + 1
    coeff[0] = (1, 0)
    with_r = cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs, coeff128=coeff)
    np.testing.assert_array_equal(with_r["challenges"], got["challenges"])
    for i in range(n):
        r = orc.from_dec(curve, FR, int(coeff[i, 0]) + (int(coeff[i, 1]) << 64))
        for name, k in (("proof_scalars", 11), ("key_scalars", 9)):
            np.testing.assert_array_equal(with_r[name][i], F(curve, "mul", got[name][i], np.tile(r, (k, 1))), err_msg=name)
    np.testing.assert_array_equal(with_r["proof_scalars"][0], got["proof_scalars"][0])     # r_0 = 1


# ---- GPU: the scalar kernel --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    ensure_built()
    c = cg.Context(0)
    yield c
    c.close()


def assert_same_scalars(got, want):
    for k in ("challenges", "proof_scalars", "key_scalars", "valid", "key_sums"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("curve,n_pub,power,infs", SHAPES)
def test_device_scalars_equal_the_host_twin(ctx, curve, n_pub, power, infs):
    n = 3
    key, commits, evals, pubs = random_case(curve, n_pub, power, n, 100 + 7 * n_pub + power + curve, infs)
    assert_same_scalars(ctx.plonk_verify_scalars(curve, key, commits, evals, pubs), cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs))
    coeff = np.random.default_rng(6).integers(0, 1 << 63, size=(n, 2), dtype=np.uint64)
    assert_same_scalars(ctx.plonk_verify_scalars(curve, key, commits, evals, pubs, coeff128=coeff), cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs, coeff128=coeff))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_device_scalars_with_idle_lanes_and_several_workgroups(ctx, n):
    curve = BN254
    key, commits, evals, pubs = random_case(curve, 2, 3, n, 900 + n)
    coeff = np.random.default_rng(n).integers(0, 1 << 63, size=(n, 2), dtype=np.uint64)
    got = ctx.plonk_verify_scalars(curve, key, commits, evals, pubs, coeff128=coeff)
    assert_same_scalars(got, cg.plonk_verify_scalars_host(curve, key, commits, evals, pubs, coeff128=coeff))
    sums = np.zeros((9, 4), dtype=np.uint64)
    for i in range(n):
        sums = F(curve, "add", sums, got["key_scalars"][i])
    np.testing.assert_array_equal(got["key_sums"], sums)


# ---- GPU: linear combinations ------------------------------------------------------------------------------------------------------------
def neg_affine(curve, pt):
    return cg.point_to_affine(curve, G1, cg.point_neg(curve, G1, cg.point_from_affine(curve, G1, pt)))


def lincomb_reference(curve, points, scalars):
    groups, k = scalars.shape[:2]
    prods = orc.points_mul(curve, G1, points.reshape(groups * k, -1), scalars.reshape(groups * k, 4)).reshape(groups, k, -1)
    out = []
    for g in range(groups):
        acc = prods[g, 0]
        for j in range(1, k):
            acc = orc.point_add(curve, G1, acc, prods[g, j])
        out.append(acc)
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("curve,groups,k", [(BN254, 1, 1), (BN254, 3, 1), (BN254, 1, 2), (BN254, 3, 2), (BN254, 70, 2), (BN254, 1, 20), (BN254, 3, 20), (BN254, 70, 20), (BN254, 70, 1),
                                            (BLS12_381, 3, 20)])
def test_g1_lincomb_batch_against_the_oracle(ctx, curve, groups, k):
    rng = np.random.default_rng(40 + groups * 31 + k + curve)
    pool = random_points(curve, 8, rng)
    points = pool[rng.integers(0, 8, size=(groups, k))]
    scalars = orc.random_field(curve, FR, groups * k, rng).reshape(groups, k, 4)
    r_minus_1 = orc.from_dec(curve, FR, orc.MODULI[(curve, FR)] - 1)
    g = groups - 1                                                                          # the last group: also the last lanes of a partly filled workgroup
    if k == 1:
        points[0, 0] = 0                                                                    # infinity alone
        if groups > 1:
            scalars[1, 0] = 0; scalars[g, 0] = r_minus_1
    if k >= 2:
        points[g, 1] = neg_affine(curve, points[g, 0]); scalars[g, 1] = scalars[g, 0]       # P and -P, equal scalars: the sum passes through infinity
        points[0, 1] = points[0, 0]; scalars[0, 1] = scalars[0, 0]                          # P and P: a doubling (groups == 1: replaces the line above)
    if k >= 20:
        points[g, 2] = 0                                                                    # a point at infinity
        scalars[g, 3] = 0                                                                   # a zero scalar
        scalars[g, 4] = r_minus_1
        points[g, 6] = points[g, 5]; scalars[g, 6] = scalars[g, 5]
    got = ctx.g1_lincomb_batch(curve, points, scalars)
    np.testing.assert_array_equal(got, lincomb_reference(curve, points, scalars))


@pytest.mark.gpu
def test_g1_lincomb_of_opposite_points_is_infinity(ctx):
    curve = BN254
    rng = np.random.default_rng(77)
    p = random_points(curve, 1, rng)[0]; s = orc.random_field(curve, FR, 1, rng)[0]
    points = np.stack([np.stack([p, neg_affine(curve, p)]), np.stack([p, p])]); scalars = np.tile(s, (2, 2, 1))
    got = ctx.g1_lincomb_batch(curve, points, scalars)
    assert not got[0].any()
    np.testing.assert_array_equal(got[1], lincomb_reference(curve, points, scalars)[1])


# ---- GPU: batches ------------------------------------------------------------------------------------------------------------------------
_made = {}
DISTINCT = 16


def make_witness(curve, rng):
    a, b = orc.random_field(curve, FR, 2, rng)
    return np.stack([orc.from_dec(curve, FR, 1), F(curve, "mul", a, b), a, b])


def proofs_of_multiplier2(curve_name, n):
    """16 distinct proofs by the product's plain Plonk prover on one session (random blinding, witnesses [1, a b, a, b]), tiled to n; made
    once per curve.  Returns (commits (n, 9, words), evals (n, 6, 4), pubs (n, n_public, 4), the first proof as a dict)"""
    if curve_name not in _made:
        curve = CURVES[curve_name]
        rng = np.random.default_rng(4321 + curve)
        sess = cg.PlonkSession(curve, fx(curve_name, "multiplier2", "circuit.zkey"), precompute=False)
        npub = sess.info["n_public"]
        dicts, pubs = [], []
        for _ in range(DISTINCT):
            w = make_witness(curve, rng)
            dicts.append(sess.prove_plain(w, orc.random_field(curve, FR, 11, rng))[0]); pubs.append(w[1:1 + npub])
        sess.close()
        _made[curve_name] = (np.stack([np.stack([d[k] for k in PLONK_COMMITS]) for d in dicts]), np.stack([np.stack([d[k] for k in PLONK_EVALS]) for d in dicts]), np.stack(pubs), dicts[0])
    c, e, p, first = _made[curve_name]
    idx = np.arange(n) % DISTINCT
    return c[idx].copy(), e[idx].copy(), p[idx].copy(), first


def as_dict(commits, evals, i):
    d = dict(zip(PLONK_COMMITS, commits[i])); d.update(zip(PLONK_EVALS, evals[i])); return d


@pytest.fixture(scope="module")
def keys():
    ensure_built()
    ks = {cn: cg.PlonkVerifyingKey.from_json(CURVES[cn], fx(cn, "multiplier2", "verification_key.json")) for cn in CURVES}
    yield ks
    for k in ks.values():
        k.close()


SEED = bytes(range(32))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,n", [("bn254", 1), ("bn254", 2), ("bn254", 65), ("bn254", 200), ("bls12_381", 65)])
def test_batch_of_valid_proofs_is_accepted(keys, curve_name, n):
    commits, evals, pubs, first = proofs_of_multiplier2(curve_name, n)
    vk = keys[curve_name]
    ok, flags = vk.verify_batch((commits, evals), pubs, seed=SEED, per_proof=True)
    assert ok and flags.all() and flags.shape == (n,)
    assert vk.verify_batch((commits, evals), pubs, seed=SEED) is True                      # a fixed seed: the same verdict again
    assert vk.verify_batch((commits, evals), pubs)                                         # coefficients from OS entropy
    if n == 1:
        assert vk.verify_batch((commits[:0], evals[:0]), pubs[:0])                         # an empty batch accepts
        assert vk.verify_batch([first], pubs[:1], seed=SEED)                               # a list of proof dicts
        assert orc.plonk_verify(CURVES[curve_name], fx(curve_name, "multiplier2", "circuit.zkey"), first, pubs[0]) and vk.verify(first, pubs[0])   # pins the witness order


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["public input", "eval_zw"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_bad_proof_is_found(keys, where, what):
    curve = BN254; n = 65
    commits, evals, pubs, _ = proofs_of_multiplier2("bn254", n)
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    if what == "public input":
        pubs[i, 0] = plus_one(curve, pubs[i, 0])
    else:
        evals[i, 5] = plus_one(curve, evals[i, 5])
    ok, flags = keys["bn254"].verify_batch((commits, evals), pubs, seed=SEED, per_proof=True)
    assert not ok
    assert list(np.flatnonzero(~flags)) == [i]
    zp = fx("bn254", "multiplier2", "circuit.zkey")
    assert not orc.plonk_verify(curve, zp, as_dict(commits, evals, i), pubs[i])
    for j in ((i + 1) % n, (i + 7) % n):
        assert orc.plonk_verify(curve, zp, as_dict(commits, evals, j), pubs[j])
    assert keys["bn254"].verify_batch((commits, evals), pubs, seed=SEED) is False          # a fixed seed: the same verdict again


@pytest.mark.gpu
def test_commitment_outside_the_subgroup_is_rejected(keys):
    from test_gpu_parity import off_subgroup_point
    curve = BLS12_381; n = 3
    commits, evals, pubs, _ = proofs_of_multiplier2("bls12_381", n)
    bad = off_subgroup_point(curve, G1)                                                    # on the curve, not multiplied by the cofactor
    assert orc.on_curve(curve, G1, bad) and not cg.point_validate(curve, G1, bad)
    commits[1, 3] = bad
    ok, flags = keys["bls12_381"].verify_batch((commits, evals), pubs, seed=SEED, per_proof=True)
    assert not ok and list(flags) == [True, False, True]
    assert not keys["bls12_381"].verify(as_dict(commits, evals, 1), pubs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 3, 7])
def test_commitment_at_infinity_passes_through_the_batch(keys, which):
    """the point at infinity is a legal encoding: the point passes accept it, the scalar kernel hashes it as zero bytes and both MSMs carry
    it as a base; the batch says what the single-proof check and the oracle say (reject), without an error, and flags that proof alone"""
    curve = BN254; n = 5; i = 2
    commits, evals, pubs, _ = proofs_of_multiplier2("bn254", n)
    commits[i, which] = 0
    zp = fx("bn254", "multiplier2", "circuit.zkey")
    want = orc.plonk_verify(curve, zp, as_dict(commits, evals, i), pubs[i])
    assert want is False and keys["bn254"].verify(as_dict(commits, evals, i), pubs[i]) is want
    ok, flags = keys["bn254"].verify_batch((commits, evals), pubs, seed=SEED, per_proof=True)
    assert ok is want and list(np.flatnonzero(~flags)) == [i]
    ok1 = keys["bn254"].verify_batch((commits[i:i + 1], evals[i:i + 1]), pubs[i:i + 1], seed=SEED)     # alone: r_0 = 1, the batch equation is the proof's own
    assert ok1 is want


@pytest.mark.gpu
def test_session_verifies_the_proof_it_has_just_made():
    ensure_built()
    curve = BN254
    zp = fx("bn254", "sum_arrays", "circuit.zkey")
    info = orc.plonk_zkey_info(curve, zp)
    w = orc.read_wtns(curve, fx("bn254", "sum_arrays", "witness.wtns"))[:info["n_vars"] - info["n_additions"]]
    sess = cg.PlonkSession(curve, zp, precompute=False)
    proof, _ = sess.prove_plain(w, orc.random_field(curve, FR, 11, np.random.default_rng(8)))
    n_pub = sess.info["n_public"]
    assert sess.verify(proof, w[1:1 + n_pub])
    bad = w[1:1 + n_pub].copy(); bad[0] = plus_one(curve, bad[0])
    assert not sess.verify(proof, bad)
    sess.close()
