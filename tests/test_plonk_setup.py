"""Plonk keys from an .r1cs (cgh_setup_plonk_dev) and the gate compiler behind them (cg_plonk_gates_*_dev, cg_plonk_sigma_labels_dev).
Yardstick: snarkjs' algorithm restated with Python integers (plonk_setup_tools.py), which reproduces the four shipped (.r1cs, Plonk .zkey)
pairs byte for byte without a GPU.  On the GPU: the product's keys equal the shipped ones in everything but the points, the points equal
multiples of the generators computed from tau and the written coefficients, the kernels equal the restatement on a circuit that takes
every branch, and proofs made on the new keys verify - for the first time on the Poseidon circuits."""
import os
import struct

import numpy as np
import pytest

import oracle_lib as orc
import plonk_setup_tools as pt
import r1cs_tools as rt
from oracle_lib import BN254, BLS12_381, FR, G1, G2
from product import cg, ensure_built
from r1cs_tools import CURVES, NO_ROW

SEED = 20240611


def plonk_fx(curve_name, circuit, f):
    return os.path.join(rt.GOLDEN, "plonk", curve_name, circuit, f)


# ---- CPU: the yardstick ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve_name,circuit", pt.PAIRS)
def test_restatement_reproduces_the_shipped_keys(curve_name, circuit):
    """header numbers and sections 3-13 of the shipped key from its .r1cs by Python integers and a naive DFT (domains 8 and 64)"""
    curve = CURVES[curve_name]
    p = rt.parse_r1cs(rt.fx(curve_name, circuit, "circuit.r1cs"))
    theirs = rt.zkey_sections(plonk_fx(curve_name, circuit, "circuit.zkey"))
    hdr, sec, g = pt.key_sections(p["n_wires"], p["n_public"], p["constraints"], rt.modulus(curve))
    assert hdr == pt.plonk_header(curve, theirs[2])[0]
    assert (hdr["k1"], hdr["k2"]) == (2, 3) and hdr["domain_size"] in (8, 64)
    for i in range(3, 14):
        assert sec[i] == theirs[i], f"section {i}"


@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_branch_circuit_takes_every_branch(curve):
    """the circuit of the kernel and proof tests does what its description says (integers only)"""
    mod = rt.modulus(curve)
    n_wires, n_pub, cons, w = pt.branch_circuit(curve)
    assert len(cons) >= 4099 and rt.evaluate(cons, w, mod) == (0, NO_ROW)
    kinds, joined_left, mul_lengths, cancelled, const_sides = set(), set(), set(), 0, set()
    for a, b, c in cons:
        (ka, ta), (kb, tb), (kc, tc) = (pt.canonical(x, mod) for x in (a, b, c))
        ya, yb = pt.lc_type(ka, ta), pt.lc_type(kb, tb)
        kinds.add((ya, yb))
        if "0" not in (ya, yb) and "k" in (ya, yb):
            k, x = (ka, (kb, tb)) if ya == "k" else (kb, (ka, ta))
            wires = {wire for wire, _ in x[1]} | {wire for wire, _ in tc}
            d = {}
            for wire, v in x[1]: d[wire] = k * v % mod
            for wire, v in tc: d[wire] = (d.get(wire, 0) - v) % mod
            left = sum(1 for v in d.values() if v)
            cancelled += len(wires) - left
            joined_left.add(min(left, 6))
        elif "0" not in (ya, yb):
            mul_lengths |= {len(ta), len(tb), len(tc)}
            const_sides.add((bool(ka), bool(kb), bool(kc)))
            if not tc: assert kc
    assert {("0", "n"), ("n", "0"), ("k", "n"), ("n", "k"), ("k", "k"), ("n", "n")} <= kinds
    assert {0, 1, 2, 3, 4, 5} <= joined_left and cancelled >= 256
    assert {0, 1, 2, 3, 64, 65, 130} <= mul_lengths
    assert len(const_sides) == 8
    assert any([wire for wire, _ in a] != sorted(wire for wire, _ in a) for a, _, _ in cons)
    assert any(len({wire for wire, _ in b}) < len(b) for _, b, _ in cons)
    g = pt.compile_gates(n_wires, n_pub, cons, mod)
    adds = g["row_adds"]
    assert g["n"] == 1 << 15 and len(adds) > 2 * 2048
    for edge in (2048, 4096):                                  # uneven counts on both sides of the scan's tile edges
        assert adds[edge - 1] > 0 and adds[edge] > 0 and adds[edge - 1] != adds[edge] and adds[edge - 2] != adds[edge - 1]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    """one development key per fixture circuit, made once for the module: (curve_name, circuit) -> path"""
    ensure_built()
    d = tmp_path_factory.mktemp("plonkkeys")
    out = {}
    for curve_name, circuit in pt.PAIRS + pt.POSEIDON:
        r = cg.R1cs(CURVES[curve_name], rt.fx(curve_name, circuit, "circuit.r1cs"))
        out[(curve_name, circuit)] = str(d / f"{curve_name}_{circuit}.zkey")
        try:
            cg.setup_plonk(r, SEED, out[(curve_name, circuit)])
        finally:
            r.close()
    return out


@pytest.fixture(scope="module")
def branch(tmp_path_factory):
    """curve -> (r1cs path, key path, the circuit, its compiled gates by integers): the branch circuit written in its own (unsorted, repeated) term order"""
    ensure_built()
    d = tmp_path_factory.mktemp("branch")
    out = {}
    for curve in (BN254, BLS12_381):
        mod = rt.modulus(curve)
        n_wires, n_pub, cons, w = pt.branch_circuit(curve)
        path, key = str(d / f"branch{curve}.r1cs"), str(d / f"branch{curve}.zkey")
        rt.write_r1cs(path, mod, n_wires, 0, n_pub, n_wires - 1 - n_pub, cons)
        out[curve] = (path, key, (n_wires, n_pub, cons, w), pt.compile_gates(n_wires, n_pub, cons, mod))
    return out


def fq_bytes(curve):
    return 48 if curve == BLS12_381 else 32


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,circuit", pt.PAIRS)
def test_key_equals_the_shipped_key_but_for_the_points(keys, curve_name, circuit, tmp_path):
    curve = CURVES[curve_name]
    mine, theirs = rt.zkey_sections(keys[(curve_name, circuit)]), rt.zkey_sections(plonk_fx(curve_name, circuit, "circuit.zkey"))
    assert sorted(mine) == list(range(1, 15))
    (h_mine, vk_mine, x2_mine), (h_theirs, vk_theirs, x2_theirs) = pt.plonk_header(curve, mine[2]), pt.plonk_header(curve, theirs[2])
    assert h_mine == h_theirs
    for i in range(3, 14):
        assert mine[i] == theirs[i], f"section {i}"
    assert mine[1] == theirs[1] and len(mine[2]) == len(theirs[2]) and len(mine[14]) == len(theirs[14]) == (h_mine["domain_size"] + 6) * 2 * fq_bytes(curve)
    assert (len(vk_mine), len(x2_mine)) == (len(vk_theirs), len(x2_theirs))
    assert cg.host_plonk_zkey_info(curve, keys[(curve_name, circuit)]) == cg.host_plonk_zkey_info(curve, plonk_fx(curve_name, circuit, "circuit.zkey"))
    r = cg.R1cs(curve, rt.fx(curve_name, circuit, "circuit.r1cs"))
    try:
        info = r.plonk_info()
        assert info == dict(n_additions=h_mine["n_additions"], n_constraints=h_mine["n_constraints"], n_vars=h_mine["n_vars"], domain_size=h_mine["domain_size"])
        again, other = str(tmp_path / "again.zkey"), str(tmp_path / "other.zkey")
        cg.setup_plonk(r, SEED, again); cg.setup_plonk(r, SEED + 1, other)
    finally:
        r.close()
    data = open(keys[(curve_name, circuit)], "rb").read()
    assert open(again, "rb").read() == data                                     # a function of the seed
    o = rt.zkey_sections(other)
    assert o[14] != mine[14] and o[2] != mine[2] and all(o[i] == mine[i] for i in range(3, 14))


def g1_multiples(curve, scalars):
    return b"".join(orc.generator_mul(curve, G1, k).tobytes() for k in rt.to_mont(curve, scalars))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,circuit", pt.PAIRS)
def test_points_from_python_integers(keys, curve_name, circuit):
    """section 14 = [tau^i] G1, X_2 = tau G2, each commitment = (sum coef_i tau^i) G1 with the coefficients as written, tau from setup_toxic"""
    curve = CURVES[curve_name]; mod = rt.modulus(curve)
    tau = rt.from_mont(curve, cg.setup_toxic(curve, SEED))[0]
    sec = rt.zkey_sections(keys[(curve_name, circuit)])
    hdr, vk, x2 = pt.plonk_header(curve, sec[2])
    n = hdr["domain_size"]
    assert pow(tau, n, mod) != 1
    assert sec[14] == g1_multiples(curve, [pow(tau, i, mod) for i in range(n + 6)])
    assert x2 == orc.generator_mul(curve, G2, rt.to_mont(curve, [tau])[0]).tobytes()
    coefs = [np.frombuffer(sec[7 + i][:n * 32], dtype=np.uint64) for i in range(5)] + [np.frombuffer(sec[12][w * 5 * n * 32:(w * 5 + 1) * n * 32], dtype=np.uint64) for w in range(3)]
    at_tau = [sum(c * pow(tau, i, mod) for i, c in enumerate(rt.from_mont(curve, co))) % mod for co in coefs]
    assert vk == g1_multiples(curve, at_tau)


def canonical_csr(curve, cons):
    """the three matrices as the kernels take them: per row the constant first, then ascending wires, repeated wires summed, zeros dropped"""
    mod = rt.modulus(curve)
    mats = []
    for m in range(3):
        row_ptr, col, val = [0], [], []
        for con in cons:
            k, terms = pt.canonical(con[m], mod)
            for wire, v in ([(0, k)] if k else []) + terms:
                col.append(wire); val.append(v)
            row_ptr.append(len(col))
        mats.append((np.array(row_ptr, dtype=np.uint32), np.array(col, dtype=np.uint32), rt.to_mont(curve, val)))
    return mats


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_gate_kernels_equal_the_restatement(branch, curve):
    """count, scan, emit and the sigma labels on the branch circuit, no files: counts, offsets, maps, the five q vectors (padding rows
    included), the addition records and the permutation rows equal the integer restatement exactly"""
    mod = rt.modulus(curve)
    _, _, (n_wires, n_pub, cons, _), g = branch[curve]
    rows, n, nc, n_add = len(cons), g["n"], g["n_constraints"], len(g["adds"])
    mats = canonical_csr(curve, cons)
    ctx = cg.Context(0)
    try:
        d_mats = [tuple(ctx.to_device(x) for x in m) for m in mats]
        counts, offsets = ctx.alloc((rows + 1) * 4), ctx.alloc((rows + 1) * 4)
        total = ctx.plonk_gates_count(curve, d_mats, rows, sum(len(m[1]) for m in mats), counts, offsets)
        assert total == n_add
        want_counts = np.array(g["row_adds"] + [0], dtype=np.uint32)
        np.testing.assert_array_equal(counts.download((rows + 1,), np.uint32), want_counts)
        np.testing.assert_array_equal(offsets.download((rows + 1,), np.uint32), np.concatenate([[0], np.cumsum(want_counts[:-1])]).astype(np.uint32))
        maps = [ctx.alloc(nc * 4) for _ in range(3)]
        q = [ctx.to_device(np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)) for _ in range(5)]     # (the padding rows must come back zero)
        add_ids, add_f = ctx.alloc(2 * n_add * 4), ctx.alloc(2 * n_add * 32)
        ctx.plonk_gates_emit(curve, d_mats, rows, n_wires, n_pub, counts, offsets, n_add, n, maps, q, add_ids, add_f)
        ctx.sync()
        for w in range(3):
            np.testing.assert_array_equal(maps[w].download((nc,), np.uint32), np.array([gate[0][w] for gate in g["gates"]], dtype=np.uint32), err_msg=f"map {w}")
        for i in range(5):
            np.testing.assert_array_equal(q[i].download((n, 4)), rt.to_mont(curve, [gate[1][i] for gate in g["gates"]] + [0] * (n - nc)), err_msg=f"q {i}")
        np.testing.assert_array_equal(add_ids.download((n_add, 2), np.uint32), np.array([a[:2] for a in g["adds"]], dtype=np.uint32))
        np.testing.assert_array_equal(add_f.download((2 * n_add, 4)), rt.to_mont(curve, [f for a in g["adds"] for f in a[2:]]))
        # the permutation rows from the previous positions
        prev = np.array(pt.sigma_prev(g), dtype=np.uint32)
        k1, k2 = pt.coset_shifts(n, mod)
        omega = pt.snarkjs_roots(mod)[n.bit_length() - 1]
        wp = [1] * n
        for i in range(1, n):
            wp[i] = wp[i - 1] * omega % mod
        d_prev, d_wp, sigma = ctx.to_device(prev), ctx.to_device(rt.to_mont(curve, wp)), ctx.alloc(3 * n * 32)
        ctx.plonk_sigma_labels(curve, d_prev, d_wp, n, rt.to_mont(curve, [k1])[0], rt.to_mont(curve, [k2])[0], sigma)
        ctx.sync()
        want = rt.to_mont(curve, [(1, k1, k2)[p // n] * wp[p % n] % mod for p in prev.tolist()])
        np.testing.assert_array_equal(sigma.download((3 * n, 4)), want)
        ctx.free_many([x for m in d_mats for x in m] + [counts, offsets, add_ids, add_f, d_prev, d_wp, sigma] + maps + q)
    finally:
        ctx.close()


def prove_and_verify(curve, r1cs_path, key_path, w):
    """the witness satisfies the R1CS, a session on the key proves, the key's verifying key accepts, and rejects a changed public input"""
    r1 = cg.R1cs(curve, r1cs_path)
    sess = cg.PlonkSession(curve, key_path)
    vk = cg.PlonkVerifyingKey.from_zkey(curve, key_path)
    try:
        assert r1.check_witness(w) == (0, NO_ROW)
        info = sess.info
        assert info["n_vars"] - info["n_additions"] == r1.info["n_wires"] == w.shape[0] and info["n_public"] == r1.info["n_public"]
        proof, _ = sess.prove_plain(w, orc.random_field(curve, FR, 11, np.random.default_rng(8)))
        n_pub = info["n_public"]
        pub = w[1:1 + n_pub]
        assert vk.verify(proof, pub)
        wrong = pub.copy()
        wrong[n_pub - 1] = rt.to_mont(curve, [rt.from_mont(curve, wrong[n_pub - 1])[0] + 1])[0]
        assert not vk.verify(proof, wrong)
    finally:
        vk.close(); sess.close(); r1.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,circuit", pt.PAIRS + pt.POSEIDON)
def test_proofs_on_the_new_keys(keys, curve_name, circuit):
    """the shipped witnesses; for the Poseidon circuits (domains of a few thousand rows, hundreds of additions) the .r1cs and witness of
    the Groth16 fixtures - the first real circuits above domain 64 that co-plonk proves"""
    curve = CURVES[curve_name]
    w = orc.read_wtns(curve, rt.fx(curve_name, circuit, "witness.wtns"))
    if circuit.startswith("poseidon"):
        assert cg.host_plonk_zkey_info(curve, keys[(curve_name, circuit)])["domain_size"] > 64
    prove_and_verify(curve, rt.fx(curve_name, circuit, "circuit.r1cs"), keys[(curve_name, circuit)], w)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [BN254, BLS12_381], ids=["bn254", "bls12_381"])
def test_branch_circuit_through_the_file(branch, curve):
    """the same circuit through the .r1cs reader and the host's canonical form (terms in descending order, wires named twice): counts, header,
    additions and maps equal the restatement, and a proof verifies - which pins the sign of k * B - C and the merge of repeated wires: a key
    compiled with another convention is satisfied by no honest witness"""
    path, key, (n_wires, n_pub, cons, w), g = branch[curve]
    mod = rt.modulus(curve)
    r = cg.R1cs(curve, path)
    try:
        assert r.plonk_info() == dict(n_additions=len(g["adds"]), n_constraints=g["n_constraints"], n_vars=g["n_vars"], domain_size=g["n"])
        cg.setup_plonk(r, SEED, key)
    finally:
        r.close()
    sec = rt.zkey_sections(key)
    k1, k2 = pt.coset_shifts(g["n"], mod)
    assert pt.plonk_header(curve, sec[2])[0] == dict(n_vars=g["n_vars"], n_public=n_pub, domain_size=g["n"], n_additions=len(g["adds"]), n_constraints=g["n_constraints"], k1=k1, k2=k2)
    ids = np.frombuffer(sec[3], dtype=np.uint32).reshape(-1, 18)[:, :2]
    np.testing.assert_array_equal(ids, np.array([a[:2] for a in g["adds"]], dtype=np.uint32))
    fs = np.frombuffer(sec[3], dtype=np.uint64).reshape(-1, 9)[:, 1:].reshape(-1, 4)
    np.testing.assert_array_equal(fs, rt.to_mont(curve, [f for a in g["adds"] for f in a[2:]]))
    for wi in range(3):
        np.testing.assert_array_equal(np.frombuffer(sec[4 + wi], dtype=np.uint32), np.array([gate[0][wi] for gate in g["gates"]], dtype=np.uint32))
    prove_and_verify(curve, path, key, rt.to_mont(curve, w))


@pytest.mark.gpu
@pytest.mark.parametrize("n_constraints,domain", [(8, 8), (9, 16), (16, 16), (64, 64)])
def test_edges_of_the_domain_rule(tmp_path, n_constraints, domain):
    """nConstraints exactly 8, exactly 9 and exactly a power of two: the smallest power of two that holds the gates, at least 8; a full
    domain (no padding row) proves and verifies"""
    ensure_built()
    curve = BN254
    n_wires, n_pub, cons, w = pt.chain_circuit(curve, 1, n_constraints - 1)
    path, key = str(tmp_path / "chain.r1cs"), str(tmp_path / "chain.zkey")
    rt.write_r1cs(path, rt.modulus(curve), n_wires, 0, n_pub, n_wires - 1 - n_pub, cons)
    r = cg.R1cs(curve, path)
    try:
        assert r.plonk_info() == dict(n_additions=0, n_constraints=n_constraints, n_vars=n_wires, domain_size=domain)
        cg.setup_plonk(r, SEED, key)
    finally:
        r.close()
    prove_and_verify(curve, path, key, rt.to_mont(curve, w))


@pytest.mark.gpu
def test_refusals(tmp_path):
    """each with a message through cgh_last_error (BackendError carries it)"""
    ensure_built()
    curve = BN254; mod = rt.modulus(curve)
    src = rt.fx("bn254", "multiplier2_example", "circuit.r1cs")
    with pytest.raises(cg.BackendError, match="prime is not the curve"):          # the curve is the handle's: the other curve's file never becomes one
        cg.R1cs(BLS12_381, src)
    r = cg.R1cs(curve, src)
    try:
        assert r.plonk_info()["domain_size"] == 8
        with pytest.raises(cg.BackendError, match="null argument"):
            cg.setup_plonk(r, SEED, None)
        with pytest.raises(cg.BackendError, match="cannot write"):
            cg.setup_plonk(r, SEED, str(tmp_path / "no_such_directory" / "key.zkey"))
        omega8 = pt.snarkjs_roots(mod)[3]
        for tau in (1, omega8, pow(omega8, 3, mod)):                               # tau^8 = 1: on the domain
            with pytest.raises(cg.BackendError, match="tau lies on the evaluation domain"):
                cg.setup_plonk_tau(r, rt.to_mont(curve, [tau])[0], str(tmp_path / "key.zkey"))
        with pytest.raises(cg.BackendError, match="tau is zero"):
            cg.setup_plonk_tau(r, np.zeros(4, dtype=np.uint64), str(tmp_path / "key.zkey"))
        with pytest.raises(cg.BackendError, match="not below the modulus"):
            cg.setup_plonk_tau(r, np.array(orc.int_to_limbs(mod, 4)), str(tmp_path / "key.zkey"))
        assert not os.path.exists(str(tmp_path / "key.zkey"))
        cg.setup_plonk_tau(r, rt.to_mont(curve, [pow(omega8, 3, mod) + 1])[0], str(tmp_path / "key.zkey"))      # next to the domain: accepted
    finally:
        r.close()
    ctx = cg.Context(0)
    try:                                                                          # the kernel layer names its curve: an unknown one, or a domain it cannot hold
        mats = canonical_csr(curve, [([(1, 1)], [(2, 1)], [(3, 1)])])
        d_mats = [tuple(ctx.to_device(x) if len(x) else ctx.alloc(16) for x in m) for m in mats]
        counts, offsets = ctx.alloc(8), ctx.alloc(8)
        with pytest.raises(cg.BackendError, match="unknown curve"):
            ctx.plonk_gates_count(7, d_mats, 1, 3, counts, offsets)
        assert ctx.plonk_gates_count(curve, d_mats, 1, 3, counts, offsets) == 0
        maps, q = [ctx.alloc(16) for _ in range(3)], [ctx.alloc(8 * 32) for _ in range(5)]
        ids, fs = ctx.alloc(16), ctx.alloc(64)
        with pytest.raises(cg.BackendError, match="domain is smaller"):
            ctx.plonk_gates_emit(curve, d_mats, 1, 4, 2, counts, offsets, 0, 2, maps, q, ids, fs)
        with pytest.raises(cg.BackendError, match="power of two"):
            ctx.plonk_sigma_labels(curve, ids, fs, 12, rt.to_mont(curve, [2])[0], rt.to_mont(curve, [3])[0], q[0])
        ctx.sync()
    finally:
        ctx.close()
