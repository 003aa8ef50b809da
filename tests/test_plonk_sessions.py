"""co-plonk proving sessions (cgh_plonk_session_*): the zkey is read once and what a proof reads from it stays on the device (PlonkResident),
the witness additions run on the GPU by dependency level, and round 3's pointwise work is fused kernels.  The per-call file entries go through
the same code, so a session proof equals the file entry's and the oracle's bit for bit, and a REP3 party's messages and ChaCha positions do
not move.
CPU: the session refuses a missing file, a Groth16 zkey and a NULL session before any device is touched.
GPU (-m gpu): the session on the example keys (additions, 1..6 public inputs, both curves) == the file entry == the oracle; three REP3
parties on sessions of their own == the plain proof and == the file entry (outputs and ChaCha positions); proofs back to back on one
session; a wrong witness length is refused and the session keeps working."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR
from product import cg, ensure_built

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = {"bn254": BN254, "bls12_381": BLS12_381}
EXAMPLES = [("bn254", "kyc"), ("bls12_381", "kyc"), ("bn254", "sum_arrays"), ("bn254", "multiplier2_example"),
            ("bn254", "multiplier2"), ("bls12_381", "multiplier2")]


def fx(curve_name, circuit, f):
    return os.path.join(GOLDEN, "plonk", curve_name, circuit, f)


def rep3_share(curve, vals, rng):
    a = orc.random_field(curve, FR, vals.shape[0], rng); b = orc.random_field(curve, FR, vals.shape[0], rng)
    c = orc.field_op(curve, FR, "sub", orc.field_op(curve, FR, "sub", vals, a), b)
    return [a, b, c], [c, a, b]


def assert_same(got, want, what=""):
    for key in cg.PLONK_COMMITS + cg.PLONK_CHALLENGES + cg.PLONK_EVALS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what} {key}")


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_session_open_refuses_bad_files_without_a_gpu():
    """a missing file and a Groth16 zkey are refused with the reader's message: the file is read before a context exists"""
    ensure_built()
    h = cg.load_host()
    out = C.c_void_p(123)
    assert h.cgh_plonk_session_open(0, BN254, b"/nonexistent/circuit.zkey", -1, 0, C.byref(out)) != 0
    assert b"nonexistent" in h.cgh_last_error() or b"open" in h.cgh_last_error().lower()
    assert out.value is None
    g16 = os.path.join(GOLDEN, "groth16", "bn254", "multiplier2", "circuit.zkey").encode()
    assert h.cgh_plonk_session_open(0, BN254, g16, -1, 0, C.byref(out)) != 0
    assert b"not a plonk zkey" in h.cgh_last_error()
    with pytest.raises(cg.BackendError, match="not a plonk zkey"):
        cg.PlonkSession(BN254, g16.decode())


def test_session_calls_on_a_null_session_fail_without_a_gpu():
    ensure_built()
    h = cg.load_host()
    buf = np.zeros((64, 4), dtype=np.uint64); out = np.zeros((9, 8), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    net = cg.Rep3NetTable(); rnd = cg.Rep3RandTable()
    assert h.cgh_plonk_session_prove_plain(None, p(buf), p(buf), p(out), None, None, None) != 0
    assert b"null session" in h.cgh_last_error()
    assert h.cgh_plonk_session_prove_rep3_party(None, p(buf), p(buf), p(buf), None, None, C.byref(net), C.byref(rnd), None, p(out), None, None, None) != 0
    assert b"null session" in h.cgh_last_error()
    info = (C.c_size_t * 6)()
    assert h.cgh_plonk_session_info(None, info) != 0
    assert h.cgh_plonk_session_close(None) == 0


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,circuit", EXAMPLES)
def test_gpu_session_plain_equals_file_entry_and_oracle(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]
    zp = fx(curve_name, circuit, "circuit.zkey")
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    blind = orc.random_field(curve, FR, 11, np.random.default_rng(5))
    s = cg.PlonkSession(curve, zp)
    try:
        assert s.info == cg.host_plonk_zkey_info(curve, zp)
        npub = s.info["n_public"]
        got, sec = s.prove_plain(w[:s.info["n_vars"] - s.info["n_additions"]], blind)
        assert sec > 0
    finally:
        s.close()
    assert_same(got, cg.plonk_prove_plain(curve, zp, w, blind, upto=5), "file entry")
    assert_same(got, orc.plonk_prove_plain(curve, zp, w, blind, upto=5), "oracle")
    assert orc.plonk_verify(curve, zp, got, w[1:npub + 1])


def _session_parties(curve, sessions, pub, wa, wb, seeds, blind=None):
    """three threads, one session each, LoopbackHub transport, ChaChaRand randomness drawn on the GPU: (outputs, final positions)"""
    hub = cg.LoopbackHub()
    rnds = [cg.ChaChaRand(curve, seeds[i], seeds[(i + 2) % 3]) for i in range(3)]
    got, errs = [None] * 3, [None] * 3

    def run(i):
        try:
            ba, bb = (None, None) if blind is None else (blind[0][i], blind[1][i])
            got[i] = sessions[i].prove_rep3_party(pub, wa[i], wb[i], hub.net(i), rnds[i].table, ba, bb, streams_table=rnds[i].streams)[0]
        except Exception as e:                                                          # noqa: BLE001 (reported below, peers released)
            errs[i] = e; hub.abort()
    th = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    for t in th: t.start()
    for t in th: t.join(600)
    pos = [r.positions() for r in rnds]
    for r in rnds: r.close()
    hub.close()
    assert errs == [None] * 3, errs
    return got, pos


def _file_parties(curve, zp, pub, wa, wb, seeds, blind=None):
    hub = cg.LoopbackHub()
    rnds = [cg.ChaChaRand(curve, seeds[i], seeds[(i + 2) % 3]) for i in range(3)]
    got, errs = [None] * 3, [None] * 3

    def run(i):
        try:
            ba, bb = (None, None) if blind is None else (blind[0][i], blind[1][i])
            got[i] = cg.plonk_prove_rep3_party(curve, zp, pub, wa[i], wb[i], hub.net(i), rnds[i].table, ba, bb, upto=5, streams_table=rnds[i].streams)
        except Exception as e:                                                          # noqa: BLE001
            errs[i] = e; hub.abort()
    th = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    for t in th: t.start()
    for t in th: t.join(600)
    pos = [r.positions() for r in rnds]
    for r in rnds: r.close()
    hub.close()
    assert errs == [None] * 3, errs
    return got, pos


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,circuit", [("bn254", "kyc"), ("bls12_381", "kyc"), ("bn254", "sum_arrays")])
def test_gpu_session_rep3_parties_equal_plain_and_file_entry(curve_name, circuit):
    """kyc: 19 additions, some over public inputs — party 2 holds no public component, so the GPU additions must leave it out there"""
    ensure_built()
    curve = CURVES[curve_name]
    zp = fx(curve_name, circuit, "circuit.zkey")
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    rng = np.random.default_rng(31)
    blind = orc.random_field(curve, FR, 11, rng)
    sessions = [cg.PlonkSession(curve, zp) for _ in range(3)]
    try:
        info = sessions[0].info
        npub = info["n_public"]; nw = info["n_vars"] - info["n_additions"]
        wa, wb = rep3_share(curve, w[npub + 1:nw], rng)
        ba, bb = rep3_share(curve, blind, rng)
        seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
        want = orc.plonk_prove_plain(curve, zp, w, blind, upto=5)
        got, pos = _session_parties(curve, sessions, w[:npub + 1], wa, wb, seeds, (ba, bb))
        for party in range(3):
            assert_same(got[party], want, f"party {party}")
        ref, ref_pos = _file_parties(curve, zp, w[:npub + 1], wa, wb, seeds, (ba, bb))
        for party in range(3):
            assert_same(got[party], ref[party], f"file entry, party {party}")
        assert pos == ref_pos
        # blinding drawn with rand() on the session, the same as on the file entry
        got, pos = _session_parties(curve, sessions, w[:npub + 1], wa, wb, seeds)
        ref, ref_pos = _file_parties(curve, zp, w[:npub + 1], wa, wb, seeds)
        for party in range(3):
            assert_same(got[party], ref[party], f"drawn blinding, party {party}")
        assert pos == ref_pos
        assert orc.plonk_verify(curve, zp, got[0], w[1:npub + 1])
        # the same sessions prove plainly afterwards, as a fresh session does
        again, _ = sessions[1].prove_plain(w[:nw], blind)
        assert_same(again, want, "plain after REP3")
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
def test_gpu_session_reuse_and_bad_witness_length(curve_name):
    """proofs back to back on one session all verify and equal the oracle; a witness of the wrong length is refused and the session
    proves correctly afterwards"""
    ensure_built()
    curve = CURVES[curve_name]
    zp = fx(curve_name, "kyc", "circuit.zkey")
    w = orc.read_wtns(curve, fx(curve_name, "kyc", "witness.wtns"))
    rng = np.random.default_rng(99)
    s = cg.PlonkSession(curve, zp, precompute=False)
    try:
        npub = s.info["n_public"]; nw = s.info["n_vars"] - s.info["n_additions"]
        for _ in range(2):
            blind = orc.random_field(curve, FR, 11, rng)
            got, _ = s.prove_plain(w[:nw], blind)
            assert_same(got, orc.plonk_prove_plain(curve, zp, w, blind, upto=5), "reuse")
            assert orc.plonk_verify(curve, zp, got, w[1:npub + 1])
        with pytest.raises(cg.BackendError, match="elements"):
            s.prove_plain(w[:nw - 1], blind)
        got, _ = s.prove_plain(w[:nw], blind)
        assert_same(got, orc.plonk_prove_plain(curve, zp, w, blind, upto=5), "after a refused witness")
    finally:
        s.close()


# ---- synthetic Plonk circuits (cgh_synth_plonk_circuit) --------------------------------------------------------------------------------
def _sections(path):
    """the binary container's sections: {id: bytes}"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"zkey"
    nsec = int.from_bytes(raw[8:12], "little"); off = 12; out = {}
    for _ in range(nsec):
        sid = int.from_bytes(raw[off:off + 4], "little"); ln = int.from_bytes(raw[off + 4:off + 12], "little")
        out[sid] = raw[off + 12:off + 12 + ln]; off += 12 + ln
    return out


def _synth(tmp_path, curve, log_n, seed, n_public, n_additions):
    zp, wp = str(tmp_path / f"p{log_n}_{seed}.zkey"), str(tmp_path / f"p{log_n}_{seed}.wtns")
    cg.host_synth_plonk_circuit(curve, log_n, seed, zp, wp, n_public=n_public, n_additions=n_additions)
    return zp, orc.read_wtns(curve, wp)


def _depth(ids, base, n_priv):
    lvl = []
    for a, (i1, i2) in enumerate(ids):
        lvl.append(1 + max([lvl[i - base - n_priv] if i >= base + n_priv else 0 for i in (int(i1), int(i2))]))
    return max(lvl) if lvl else 0


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
@pytest.mark.parametrize("log_n,n_public,n_additions", [(8, 1, 40), (10, 3, 256)])
def test_gpu_synthetic_plonk_circuit(tmp_path, curve_name, log_n, n_public, n_additions):
    """the requested shape in both readers; the header's eight commitments = MSM(p_tau, coefficients); the oracle's proof verifies and
    fails with a public input changed; the session, the file entry and the oracle agree bit for bit"""
    ensure_built()
    curve = CURVES[curve_name]
    zp, w = _synth(tmp_path, curve, log_n, 11 + log_n, n_public, n_additions)
    n = 1 << log_n
    info = orc.plonk_zkey_info(curve, zp)
    assert cg.host_plonk_zkey_info(curve, zp) == info
    assert (info["domain_size"], info["n_public"], info["n_additions"]) == (n, n_public, n_additions)
    assert w.shape[0] == info["n_vars"] - n_additions
    maps, ids, _, p_tau = orc.plonk_zkey_data(curve, zp)
    n_priv = info["n_vars"] - n_additions - n_public - 1
    assert _depth(ids, n_public + 1, n_priv) >= 4
    assert any(int(i) <= n_public for i in ids[:, 1])                                  # additions over public inputs
    assert np.array_equal(maps[0][:n_public], np.arange(1, n_public + 1))              # public-input rows
    sec = _sections(zp)
    coef = [np.frombuffer(sec[7 + i], dtype=np.uint64)[:4 * n].reshape(n, 4) for i in range(5)]
    coef += [np.frombuffer(sec[12], dtype=np.uint64)[20 * n * k:20 * n * k + 4 * n].reshape(n, 4) for k in range(3)]
    vk = orc.plonk_zkey_vk(curve, zp)
    for key, co in zip(("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"), coef):
        np.testing.assert_array_equal(vk[key], orc.msm(curve, orc.G1, p_tau[:n], co, threads=4), err_msg=key)
    blind = orc.random_field(curve, FR, 11, np.random.default_rng(log_n))
    want = orc.plonk_prove_plain(curve, zp, w, blind, upto=5)
    pub = w[1:n_public + 1]
    assert orc.plonk_verify(curve, zp, want, pub)
    wrong = pub.copy(); wrong[-1] = orc.field_op(curve, FR, "add", wrong[-1:], orc.from_dec(curve, FR, "1")[None])[0]
    assert not orc.plonk_verify(curve, zp, want, wrong)
    if log_n == 10:
        s = cg.PlonkSession(curve, zp)
        try: got, _ = s.prove_plain(w, blind)
        finally: s.close()
        assert_same(got, want, "session")
        assert_same(cg.plonk_prove_plain(curve, zp, w, blind, upto=5), want, "file entry")


@pytest.mark.gpu
def test_gpu_additions_on_the_gpu_equal_the_oracle_for_every_party(tmp_path):
    """n_additions = n / 4 in chains six deep, some over public inputs: each REP3 party (party 2 holds no public component) reports the
    oracle's values, on sessions and on the file entry alike (ChaCha positions included)"""
    ensure_built()
    curve = BN254
    zp, w = _synth(tmp_path, curve, 10, 7, 3, 256)
    rng = np.random.default_rng(12)
    blind = orc.random_field(curve, FR, 11, rng)
    want = orc.plonk_prove_plain(curve, zp, w, blind, upto=5)
    sessions = [cg.PlonkSession(curve, zp) for _ in range(3)]
    try:
        wa, wb = rep3_share(curve, w[4:], rng)
        ba, bb = rep3_share(curve, blind, rng)
        seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
        got, pos = _session_parties(curve, sessions, w[:4], wa, wb, seeds, (ba, bb))
        for party in range(3):
            assert_same(got[party], want, f"party {party}")
        ref, ref_pos = _file_parties(curve, zp, w[:4], wa, wb, seeds, (ba, bb))
        for party in range(3):
            assert_same(ref[party], want, f"file entry, party {party}")
        assert pos == ref_pos
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
def test_gpu_rep3_sessions_at_2_14(tmp_path):
    ensure_built()
    curve = BN254
    zp, w = _synth(tmp_path, curve, 14, 3, 2, 1 << 12)
    rng = np.random.default_rng(14)
    blind = orc.random_field(curve, FR, 11, rng)
    sessions = [cg.PlonkSession(curve, zp) for _ in range(3)]
    try:
        want, _ = sessions[0].prove_plain(w, blind)
        wa, wb = rep3_share(curve, w[3:], rng)
        ba, bb = rep3_share(curve, blind, rng)
        seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
        got, _ = _session_parties(curve, sessions, w[:3], wa, wb, seeds, (ba, bb))
        for party in range(3):
            assert_same(got[party], want, f"party {party}")
        assert orc.plonk_verify(curve, zp, want, w[1:3])
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,log_n", [("bn254", 14), ("bn254", 16), ("bls12_381", 14)])
def test_gpu_session_proofs_at_scale_verify(tmp_path, curve_name, log_n):
    """plain session proofs at 2^14 / 2^16 verify; two different witnesses (two synthetic circuits' keys differ, so: two blindings and a
    second proof) back to back on one session both verify"""
    ensure_built()
    curve = CURVES[curve_name]
    zp, w = _synth(tmp_path, curve, log_n, 5, 1, 1 << (log_n - 2))
    rng = np.random.default_rng(log_n)
    s = cg.PlonkSession(curve, zp)
    try:
        for _ in range(2):
            got, _ = s.prove_plain(w, orc.random_field(curve, FR, 11, rng))
            assert orc.plonk_verify(curve, zp, got, w[1:2])
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rep3_session_proof_at_2_16_verifies(tmp_path):
    ensure_built()
    curve = BN254
    zp, w = _synth(tmp_path, curve, 16, 9, 1, 1 << 14)
    rng = np.random.default_rng(16)
    sessions = [cg.PlonkSession(curve, zp) for _ in range(3)]
    try:
        wa, wb = rep3_share(curve, w[2:], rng)
        seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
        got, _ = _session_parties(curve, sessions, w[:2], wa, wb, seeds)
        for party in (1, 2):
            assert_same(got[party], got[0], f"party {party}")
        assert orc.plonk_verify(curve, zp, got[0], w[1:2])
    finally:
        for s in sessions: s.close()
