"""ONE Shamir party of co-plonk behind the callback ABI (cgh_plonk_prove_shamir_party, cgh_plonk_session_prove_shamir_party{,_seeded},
cgh_plonk_session_shamir_pairs) and the two kernels under it (cg_shamir_share_dev, cg_plonk_r2_factors_dev).  Every comparison is exact.
CPU: the entries refuse NULL sessions / arguments, a round outside 1..5 and 2t + 1 > n before a file or a device is looked at.
GPU (-m gpu): n parties over the loopback == cgh_plonk_prove_shamir == the plain proof, file entry and session receive the same bytes message
by message; at size (2^14, 2^16) on preprocessed pairs that never leave the device, with the pair count the formula gives; lazy batches;
(5, 2); blindings drawn inside; session reuse and error returns; the kernels alone against Python integers."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
from oracle_lib import BN254, BLS12_381, FR
from product import cg, ensure_built
from vec_ref import Mont, from_ints, to_ints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = {"bn254": BN254, "bls12_381": BLS12_381}
KEYS = cg.PLONK_COMMITS + cg.PLONK_CHALLENGES + cg.PLONK_EVALS


def fx(curve_name, circuit, f):
    return os.path.join(GOLDEN, "plonk", curve_name, circuit, f)


def assert_same(got, want, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what} {key}")


def pairs_formula(n, with_blinding=False):
    """round 2: 4n (num b, den b, num c, den c) + 2 (4n + 2) (array_prod_mul) + 2n (inv_many, z); round 3: 36 products of 4n; 11 scalar rand()"""
    return 14 * n + 4 + 36 * 4 * n + (11 if with_blinding else 0)


def stream_len(n_domain, t):
    """draws of one party that proves on lazy batches: whole batches of 1024 secrets (1 + 3t draws each) + the king's t coefficients per re-shared element"""
    pairs = pairs_formula(n_domain, True)
    batches = -(-pairs // (1024 * (t + 1)))
    return batches * 1024 * (1 + 3 * t) + t * pairs + 64


class PartyEnd:
    """party i's callback tables in Python over a loopback table: keeps what it receives (sender, bytes), serves the party's private
    randomness from a stream, and can fail its k-th send (an error RETURN of the callback)"""

    def __init__(self, inner, stream=None, fail_after=None):
        self.inner, self.stream, self.k, self.received, self.sends, self.fail_after = inner, stream, 0, [], 0, fail_after
        self._cbs = (cg._SH_SEND(self._send), cg._SH_RECV(self._recv), cg._SH_RAND(self._rand))
        self.net = cg.ShamirNetTable(None, inner.party_id, inner.num_parties, self._cbs[0], self._cbs[1])
        self.rand = cg.ShamirRandTable(None, self._cbs[2])

    def _send(self, u, to, data, nbytes):
        self.sends += 1
        if self.fail_after is not None and self.sends > self.fail_after: return 5
        return self.inner.send(self.inner.user, to, data, nbytes)

    def _recv(self, u, frm, data, nbytes):
        rc = self.inner.recv(self.inner.user, frm, data, nbytes)
        if rc == 0: self.received.append((frm, C.string_at(data, nbytes)))
        return rc

    def _rand(self, u, n, out):
        if self.stream is None or self.k + n > self.stream.shape[0]: return 1
        C.memmove(out, self.stream[self.k:self.k + n].ctypes.data, 32 * n); self.k += n
        return 0


def run_parties(n, call):
    """n threads; call(i, hub) -> result; a failing party releases its peers.  Returns (results, errors)."""
    hub = cg.ShamirLoopbackHub(n)
    got, errs = [None] * n, [None] * n

    def run(i):
        try: got[i] = call(i, hub)
        except Exception as e:                                                          # noqa: BLE001 (reported to the caller, peers released)
            errs[i] = e; hub.abort()
    th = [threading.Thread(target=run, args=(i,)) for i in range(n)]
    for x in th: x.start()
    for x in th: x.join(900)
    hub.close()
    return got, errs


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_shamir_party_entries_refuse_bad_arguments_without_a_gpu():
    ensure_built()
    h = cg.load_host()
    buf = np.zeros((64, 4), dtype=np.uint64); out = np.zeros((9, 8), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = cg._SH_SEND(lambda *a: 0), cg._SH_RECV(lambda *a: 0), cg._SH_RAND(lambda *a: 0)
    net3 = cg.ShamirNetTable(None, 0, 3, ok[0], ok[1]); rnd = cg.ShamirRandTable(None, ok[2])
    seed = bytes(32)
    zp = b"/nonexistent/circuit.zkey"
    err = lambda: h.cgh_last_error()
    file_entry = lambda t, net, rnd_, upto, commits=out, wit=buf: h.cgh_plonk_prove_shamir_party(
        0, BN254, zp, t, p(buf), None if wit is None else p(wit), None, None if net is None else C.byref(net), None if rnd_ is None else C.byref(rnd_),
        C.c_size_t(0), upto, None if commits is None else p(commits), None, None, None, None, None)
    # the file entry: NULL arguments, upto, threshold — all before the (missing) file is opened
    assert file_entry(1, None, rnd, 5) != 0 and b"null argument" in err()
    assert file_entry(1, net3, None, 5) != 0 and b"null argument" in err()
    assert file_entry(1, net3, rnd, 5, commits=None) != 0 and b"null argument" in err()
    assert file_entry(1, net3, rnd, 5, wit=None) != 0 and b"null argument" in err()
    for upto in (0, 6, -1):
        assert file_entry(1, net3, rnd, upto) != 0 and b"upto" in err()
    assert file_entry(2, net3, rnd, 5) != 0 and b"Threshold too large" in err()
    assert file_entry(-1, net3, rnd, 5) != 0 and b"Threshold too large" in err()
    assert file_entry(1, net3, rnd, 5) != 0 and b"Threshold" not in err() and b"null" not in err()      # now the file is looked for
    # the session entries
    ses = lambda s, t, net, rnd_: h.cgh_plonk_session_prove_shamir_party(s, t, p(buf), p(buf), None, None if net is None else C.byref(net), None if rnd_ is None else C.byref(rnd_),
                                                                       C.c_size_t(0), p(out), None, None, None, None, None)
    seeded = lambda s, t, net, sd: h.cgh_plonk_session_prove_shamir_party_seeded(s, t, p(buf), p(buf), None, None if net is None else C.byref(net), sd,
                                                                               C.c_size_t(0), p(out), None, None, None, None, None)
    assert ses(None, 1, net3, rnd) != 0 and b"null session" in err()
    assert seeded(None, 1, net3, seed) != 0 and b"null session" in err()
    assert ses(None, 1, None, rnd) != 0 and b"null argument" in err()
    assert ses(None, 1, net3, None) != 0 and b"null argument" in err()
    assert seeded(None, 1, net3, None) != 0 and b"null argument" in err()
    assert seeded(None, 1, None, seed) != 0 and b"null argument" in err()
    assert ses(None, 2, net3, rnd) != 0 and b"Threshold too large" in err()
    assert seeded(None, 2, net3, seed) != 0 and b"Threshold too large" in err()
    net2 = cg.ShamirNetTable(None, 0, 2, ok[0], ok[1])
    assert seeded(None, 0, net2, seed) != 0 and b"at least 3 parties" in err()
    nopairs = C.c_size_t(7)
    assert h.cgh_plonk_session_shamir_pairs(None, 1, 0, C.byref(nopairs)) != 0 and b"null session" in err()
    assert h.cgh_plonk_session_shamir_pairs(None, 1, 0, None) != 0 and b"null argument" in err()
    assert h.cgh_plonk_session_shamir_pairs(None, -1, 0, C.byref(nopairs)) != 0 and b"threshold" in err()
    assert nopairs.value == 7


def test_new_device_exports_refuse_bad_arguments_without_a_gpu():
    ensure_built()
    lib = cg.load()
    assert lib.cg_shamir_share_dev(None, BN254, None, None, C.c_int64(0), C.c_int64(1), C.c_size_t(1), 1, 3, None, C.c_int64(0), C.c_int64(1)) != 0
    assert lib.cg_plonk_r2_factors_dev(None, BN254, 1, 0, C.c_size_t(8), None, C.c_size_t(4), None, C.c_size_t(4), None, None, None) != 0


# ---- GPU: fixtures ---------------------------------------------------------------------------------------------------------------------
def _fixture(curve_name, circuit, n, t, seed):
    curve = CURVES[curve_name]
    zp = fx(curve_name, circuit, "circuit.zkey")
    info = orc.plonk_zkey_info(curve, zp)
    npub = info["n_public"]
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    rng = np.random.default_rng(seed)
    blind = orc.random_field(curve, FR, 11, rng)
    wits = orc.shamir_share(curve, w[npub + 1:info["n_vars"] - info["n_additions"]], n, t, rng)
    blinds = orc.shamir_share(curve, blind, n, t, rng)
    streams = [orc.random_field(curve, FR, stream_len(info["domain_size"], t), rng) for _ in range(n)]
    return curve, zp, info, w, blind, wits, blinds, streams


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
@pytest.mark.parametrize("circuit", ["kyc", "multiplier2"])
@pytest.mark.parametrize("n,t", [(3, 1), (5, 2)])
def test_gpu_fixture_parties_equal_the_in_process_entry_and_the_plain_proof(curve_name, circuit, n, t):
    ensure_built()
    curve, zp, info, w, blind, wits, blinds, streams = _fixture(curve_name, circuit, n, t, 100 + n)
    npub = info["n_public"]; pub = w[:npub + 1]
    ref = cg.plonk_prove_shamir(curve, zp, n, t, pub, wits, blinds, streams, upto=5)
    plain = orc.plonk_prove_plain(curve, zp, w, blind, upto=5)
    # the FILE party entry, lazy batches, the same streams behind randomness callbacks
    ends = [None] * n

    def file_party(i, hub):
        ends[i] = PartyEnd(hub.net(i, record=True), streams[i])
        return cg.plonk_prove_shamir_party(curve, zp, t, pub, wits[i], ends[i].net, ends[i].rand, blind=blinds[i], preprocess=0, upto=5)
    got, errs = run_parties(n, file_party)
    assert errs == [None] * n, errs
    for i in range(n):
        out, sec, st = got[i]
        assert_same(out, ref[i], f"in-process entry, party {i}")
        assert_same(out, plain, f"plain proof, party {i}")
        assert sec > 0
        assert st["pairs_consumed"] == pairs_formula(info["domain_size"]) and st["pairs_from_device"] == 0
        assert st["lazy_batches"] == -(-st["pairs_consumed"] // (1024 * (t + 1)))
        assert st["pairs_left"] == st["lazy_batches"] * 1024 * (t + 1) - st["pairs_consumed"]
    assert orc.plonk_verify(curve, zp, got[0][0], w[1:npub + 1])
    file_log = [e.received for e in ends]
    # the SESSION entry on the same streams: the same bytes arrive, message by message
    sessions = [cg.PlonkSession(curve, zp) for _ in range(n)]
    try:
        def session_party(i, hub):
            ends[i] = PartyEnd(hub.net(i, record=True), streams[i])
            return sessions[i].prove_shamir_party(t, pub, wits[i], ends[i].net, ends[i].rand, blind=blinds[i], preprocess=0)
        got2, errs = run_parties(n, session_party)
        assert errs == [None] * n, errs
    finally:
        for s in sessions: s.close()
    for i in range(n):
        assert_same(got2[i][0], plain, f"session, party {i}")
        assert len(ends[i].received) == len(file_log[i]) and len(file_log[i]) > 0
        for m, (a, b) in enumerate(zip(ends[i].received, file_log[i])):
            assert a[0] == b[0] and a[1] == b[1], f"party {i}: message {m} differs between the session and the file entry"


@pytest.mark.gpu
@pytest.mark.parametrize("upto", [1, 2, 3, 4])
def test_gpu_fixture_parties_stop_after_the_requested_round(upto):
    ensure_built()
    n, t = 3, 1
    curve, zp, info, w, blind, wits, blinds, streams = _fixture("bn254", "kyc", n, t, 7)
    pub = w[:info["n_public"] + 1]
    ref = cg.plonk_prove_shamir(curve, zp, n, t, pub, wits, blinds, streams, upto=upto)

    def party(i, hub):
        e = PartyEnd(hub.net(i), streams[i])
        return cg.plonk_prove_shamir_party(curve, zp, t, pub, wits[i], e.net, e.rand, blind=blinds[i], upto=upto), e
    got, errs = run_parties(n, party)
    assert errs == [None] * n, errs
    reached = {1: 3, 2: 4, 3: 7, 4: 7}[upto]
    for i in range(n):
        out = got[i][0][0]
        assert_same(out, ref[i], f"party {i}")
        for j, key in enumerate(cg.PLONK_COMMITS):
            assert bool(np.any(out[key])) == (j < reached), key
        assert bool(np.any(out["eval_a"])) == (upto >= 4)


# ---- GPU: at size ----------------------------------------------------------------------------------------------------------------------
def _synth(tmp_path, curve, log_n, seed, n_public, n_additions):
    zp, wp = str(tmp_path / f"p{log_n}_{seed}.zkey"), str(tmp_path / f"p{log_n}_{seed}.wtns")
    cg.host_synth_plonk_circuit(curve, log_n, seed, zp, wp, n_public=n_public, n_additions=n_additions)
    return zp, orc.read_wtns(curve, wp)


def _seeded_sessions(sessions, t, pub, wits, blinds, seeds, preprocess):
    n = len(sessions)
    got, errs = run_parties(n, lambda i, hub: sessions[i].prove_shamir_party_seeded(t, pub, wits[i], hub.net(i), seeds[i], blind=None if blinds is None else blinds[i],
                                                                                     preprocess=preprocess, timing=(i == 0)))
    assert errs == [None] * n, errs
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,log_n", [("bn254", 14), ("bn254", 16), ("bls12_381", 14)])
def test_gpu_seeded_session_parties_at_size(tmp_path, curve_name, log_n):
    """(3, 1) on preprocessed pairs: every party == the plain session proof with the blinding values that were shared, the proof verifies,
    and the pair buffers were used exactly as cgh_plonk_session_shamir_pairs says — all of them read on the device, none made lazily.
    2^14: the same circuit on lazy batches with callback randomness (the host path) gives the same proof."""
    ensure_built()
    curve = CURVES[curve_name]
    n, t = 3, 1
    zp, w = _synth(tmp_path, curve, log_n, 5, 1, 1 << (log_n - 2))
    rng = np.random.default_rng(200 + log_n)
    blind = orc.random_field(curve, FR, 11, rng)
    wits = orc.shamir_share(curve, w[2:], n, t, rng)
    blinds = orc.shamir_share(curve, blind, n, t, rng)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    sessions = [cg.PlonkSession(curve, zp) for _ in range(n)]
    try:
        want, _ = sessions[0].prove_plain(w, blind)
        pairs = sessions[0].shamir_pairs(t, False)
        assert pairs == pairs_formula(1 << log_n) == 158 * (1 << log_n) + 4
        assert sessions[0].shamir_pairs(t, True) == pairs + 11
        got = _seeded_sessions(sessions, t, w[:2], wits, blinds, seeds, -(-pairs // (t + 1)))
        for i in range(n):
            out, sec, st = got[i]
            assert_same(out, want, f"party {i}")
            assert st["pairs_consumed"] == pairs, st
            assert st["lazy_batches"] == 0 and st["pairs_left"] < t + 1, st
            assert st["pairs_from_device"] == pairs, st                                  # blindings given: no scalar pop at all
        assert orc.plonk_verify(curve, zp, want, w[1:2])
        rs = got[0][2]["round_seconds"]
        assert len(rs) == 6 and all(x > 0 for x in rs) and sum(rs) <= got[0][1] * 1.001
        if log_n == 14 and curve == BN254:
            streams = [orc.random_field(curve, FR, stream_len(1 << log_n, t), rng) for _ in range(n)]

            def lazy_party(i, hub):
                e = PartyEnd(hub.net(i), streams[i])
                return sessions[i].prove_shamir_party(t, w[:2], wits[i], hub.net(i), e.rand, blind=blinds[i], preprocess=0), e
            lazy, errs = run_parties(n, lazy_party)
            assert errs == [None] * n, errs
            for i in range(n):
                out, _, st = lazy[i][0]
                assert_same(out, want, f"lazy batches, party {i}")
                assert st["pairs_consumed"] == pairs and st["pairs_from_device"] == 0 and st["lazy_batches"] == -(-pairs // (1024 * (t + 1))), st
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
def test_gpu_five_parties_threshold_two_at_2_12(tmp_path):
    ensure_built()
    curve, n, t = BN254, 5, 2
    zp, w = _synth(tmp_path, curve, 12, 21, 2, 1 << 10)
    rng = np.random.default_rng(52)
    blind = orc.random_field(curve, FR, 11, rng)
    wits = orc.shamir_share(curve, w[3:], n, t, rng)
    blinds = orc.shamir_share(curve, blind, n, t, rng)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    sessions = [cg.PlonkSession(curve, zp) for _ in range(n)]
    try:
        want, _ = sessions[0].prove_plain(w, blind)
        pairs = sessions[0].shamir_pairs(t, False)
        got = _seeded_sessions(sessions, t, w[:3], wits, blinds, seeds, -(-pairs // (t + 1)))
        for i in range(n):
            assert_same(got[i][0], want, f"party {i}")
            st = got[i][2]
            assert st["pairs_consumed"] == st["pairs_from_device"] == pairs and st["lazy_batches"] == 0 and st["pairs_left"] < t + 1, st
        assert orc.plonk_verify(curve, zp, want, w[1:3])
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
def test_gpu_blindings_drawn_inside(tmp_path):
    """blind = NULL: b_1..b_11 are rand() draws — eleven scalar pops from the device-resident block; the parties agree and the proof verifies"""
    ensure_built()
    curve, n, t = BN254, 3, 1
    zp, w = _synth(tmp_path, curve, 12, 22, 1, 1 << 10)
    rng = np.random.default_rng(53)
    wits = orc.shamir_share(curve, w[2:], n, t, rng)
    seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    sessions = [cg.PlonkSession(curve, zp) for _ in range(n)]
    try:
        pairs = sessions[0].shamir_pairs(t, True)
        assert pairs == 158 * 4096 + 4 + 11
        got = _seeded_sessions(sessions, t, w[:2], wits, None, seeds, -(-pairs // (t + 1)))
        for i in range(n):
            assert_same(got[i][0], got[0][0], f"party {i}")
            st = got[i][2]
            assert st["pairs_consumed"] == pairs and st["pairs_from_device"] == pairs - 11 and st["lazy_batches"] == 0 and st["pairs_left"] < t + 1, st
        assert orc.plonk_verify(curve, zp, got[0][0], w[1:2])
    finally:
        for s in sessions: s.close()


@pytest.mark.gpu
def test_gpu_session_reuse_and_error_returns():
    """two proofs back to back with different seeds; a witness of the wrong length and a network callback that returns an error inside round 2
    (the peers released by cgh_shamir_loopback_abort) end with an error, and the sessions prove correctly afterwards"""
    ensure_built()
    n, t = 3, 1
    curve, zp, info, w, blind, wits, blinds, _ = _fixture("bn254", "kyc", n, t, 9)
    npub = info["n_public"]; pub = w[:npub + 1]
    want = orc.plonk_prove_plain(curve, zp, w, blind, upto=5)
    rng = np.random.default_rng(61)
    sessions = [cg.PlonkSession(curve, zp) for _ in range(n)]
    try:
        pre = -(-sessions[0].shamir_pairs(t, False) // (t + 1))
        for _ in range(2):
            seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
            got = _seeded_sessions(sessions, t, pub, wits, blinds, seeds, pre)
            for i in range(n):
                assert_same(got[i][0], want, f"party {i}")
            assert orc.plonk_verify(curve, zp, got[0][0], w[1:npub + 1])
        with pytest.raises(cg.BackendError, match="elements"):
            sessions[1].prove_shamir_party_seeded(t, pub, wits[1][:-1], cg.ShamirNetTable(), seeds[1], blind=blinds[1])
        # party 1 sends 2 messages while preprocessing and 3 in round 1 (three openings): its 9th send is the fourth product of round 2
        ends = [None] * n

        def failing(i, hub):
            ends[i] = PartyEnd(hub.net(i), fail_after=8 if i == 1 else None)
            return sessions[i].prove_shamir_party_seeded(t, pub, wits[i], ends[i].net, seeds[i], blind=blinds[i], preprocess=pre)
        got, errs = run_parties(n, failing)
        assert all(isinstance(e, cg.BackendError) for e in errs), errs
        assert ends[1].sends == 9 and "send" in str(errs[1])
        got = _seeded_sessions(sessions, t, pub, wits, blinds, seeds, pre)
        for i in range(n):
            assert_same(got[i][0], want, f"after the failed proof, party {i}")
    finally:
        for s in sessions: s.close()


# ---- GPU: the kernels alone, against Python integers ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
@pytest.mark.parametrize("degree,parties", [pytest.param(d, n, id=f"{n}-{d}") for n in (3, 5, 7) for d in (1, 2, 4)] +
                         [pytest.param(d, n, id=f"{n}-{d}") for d, n in ((0, 3), (5, 3), (5, 7), (6, 5), (9, 19))])
def test_gpu_shamir_share_kernel_equals_horner_in_python_integers(curve_name, degree, parties):
    """degrees 1, 2, 4 stay in k_shamir_share's registers (SHARE_REG_DEGREE = 4); 5 is the first that re-reads its coefficients per receiver,
    6 and 9 (19 receivers) go on from there; degree 0 copies the secrets.  The reference is quadratic in the degree, so 2^16 + 3 elements run
    on the register path only."""
    ensure_built()
    curve = CURVES[curve_name]; F = Mont(curve)
    ctx = cg.Context(0)
    rng = np.random.default_rng(1000 * degree + parties)
    coeff_off, coeff_stride, out_off, out_stride = 3, degree + 2, 1, 2
    try:
        for ln in (1, 63, 64, 65, 1000, (1 << 16) + 3) if degree in (1, 2, 4) else (1, 65, 1000):
            sec = orc.random_field(curve, FR, ln, rng)
            for j, v in enumerate((0, 1, F.r - 1, F.R)[:ln]): sec[j] = from_ints([v])[0]
            co = orc.random_field(curve, FR, coeff_off + ln * coeff_stride, rng)
            d_sec, d_co = ctx.to_device(sec), ctx.to_device(co)
            outs = [ctx.alloc((out_off + ln * out_stride) * 32).zero() for _ in range(parties)]
            ctx.shamir_share(curve, d_sec, d_co, coeff_off, coeff_stride, ln, degree, outs, out_off, out_stride)
            s, c = to_ints(sec), to_ints(co)
            for p in range(parties):
                x = F.of(p + 1)
                want = [0] * (out_off + ln * out_stride)
                for i in range(ln):
                    acc = 0
                    for j in range(degree - 1, -1, -1): acc = F.mul((acc + c[coeff_off + i * coeff_stride + j]) % F.r, x)
                    want[out_off + i * out_stride] = (acc + s[i]) % F.r
                got = outs[p].download((out_off + ln * out_stride, 4))
                np.testing.assert_array_equal(got, from_ints(want), err_msg=f"len {ln} party {p}")
            for b in outs + [d_sec, d_co]: b.free()
        # the king's layout: the party's own share written over the secrets
        ln = 1000
        sec = orc.random_field(curve, FR, ln, rng); co = orc.random_field(curve, FR, max(1, ln * degree), rng)
        d_sec, d_co = ctx.to_device(sec), ctx.to_device(co)
        outs = [d_sec] + [ctx.alloc(ln * 32) for _ in range(parties - 1)]
        ctx.shamir_share(curve, d_sec, d_co, 0, degree, ln, degree, outs)
        s, c = to_ints(sec), to_ints(co)
        for p in (0, parties - 1):
            x = F.of(p + 1); want = []
            for i in range(ln):
                acc = 0
                for j in range(degree - 1, -1, -1): acc = F.mul((acc + c[i * degree + j]) % F.r, x)
                want.append((acc + s[i]) % F.r)
            np.testing.assert_array_equal(outs[p].download((ln, 4)), from_ints(want), err_msg=f"in place, party {p}")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["bn254", "bls12_381"])
@pytest.mark.parametrize("log_n", [3, 12])
@pytest.mark.parametrize("k,pc", [(1, -1), (1, 0), (2, -1), (2, 0), (2, 1)])
def test_gpu_r2_factors_kernel_equals_python_integers(curve_name, log_n, k, pc):
    ensure_built()
    curve = CURVES[curve_name]; F = Mont(curve)
    n = 1 << log_n
    rng = np.random.default_rng(31 * log_n + 7 * k + pc)
    _, roots, _ = orc.roots_of_unity(curve)
    w4 = to_ints(roots[log_n + 2])[0]
    omega = F.mul(F.mul(w4, w4), F.mul(w4, w4))
    pw = [F.R]
    for _ in range(4 * n - 1): pw.append(F.mul(pw[-1], w4))
    beta, gamma, k1, k2 = to_ints(orc.random_field(curve, FR, 4, rng))
    sigma = [orc.random_field(curve, FR, 4 * n, rng) for _ in range(3)]
    wires = [orc.random_field(curve, FR, n, rng) for _ in range(3 * k)]                  # [a0, (a1), b0, (b1), c0, (c1)]
    ctx = cg.Context(0)
    try:
        d_pw = ctx.to_device(from_ints(pw)); d_sigma = [ctx.to_device(x) for x in sigma]; d_w = [ctx.to_device(x) for x in wires]
        outs = [ctx.alloc(n * 32) for _ in range(6 * k)]
        ctx.plonk_r2_factors(curve, k, pc, n, d_pw, 4, d_sigma, 4, from_ints([beta, F.mul(beta, k1), F.mul(beta, k2), gamma]), d_w, outs)
        kw = (F.R, k1, k2)
        wi = [to_ints(x) for x in wires]; sg = [to_ints(x) for x in sigma]
        x = F.R; xs = []
        for _ in range(n): xs.append(x); x = F.mul(x, omega)
        for w in range(3):
            for j in range(k):
                num = [(wi[w * k + j][i] + (F.mul(F.mul(beta, kw[w]), xs[i]) + gamma if j == pc else 0)) % F.r for i in range(n)]
                den = [(wi[w * k + j][i] + (F.mul(beta, sg[w][4 * i]) + gamma if j == pc else 0)) % F.r for i in range(n)]
                np.testing.assert_array_equal(outs[w * k + j].download((n, 4)), from_ints(num), err_msg=f"num wire {w} component {j}")
                np.testing.assert_array_equal(outs[(3 + w) * k + j].download((n, 4)), from_ints(den), err_msg=f"den wire {w} component {j}")
    finally:
        ctx.close()
