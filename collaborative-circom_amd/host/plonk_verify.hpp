// Plonk verification (co-circom/co-plonk/src/plonk.rs:133-271) over the C ABI: verifying-key handles from a verification_key.json
// (circom-types/src/plonk/verification_key.rs) or a zkey header, the single-proof check on the host, and the randomised batch check on the GPU.
//
// Per proof, cg_plonk_verify_scalars (csrc/plonk_verify.hpp) gives the six challenges and the coefficients of two G1 linear combinations
//     A1 = wxi + u wxiw,      B1 = 9 terms over the proof's commitments + 8 terms over the key's points + (-e) G
// with: the proof satisfies plonk.rs:254-271 iff e(A1, X_2) e(-B1, G_2) = 1.
// Single proof: 20 host scalar multiplications and cg_pairing_check over two pairs.
// Batch of n proofs under one key: with r_0 = 1 and r_1.. uniform 128-bit coefficients, accept iff
//     e(sum_i r_i A1_i, X_2) e(-sum_i r_i B1_i, G_2) = 1:
// the kernel multiplies proof i's scalars by r_i, one MSM over the 2n A-side points and one over the 9n B-side points give the sums (the
// key's points take the scalars summed over the proofs), and two pairings remain for the whole batch.  Soundness is the argument of
// verify.hpp word for word: with proof i's check written t_i = 1 in the target group of prime order r, the batch accepts iff
// prod t_i^(r_i) = 1, which at most a 2^-128 fraction of the coefficient vectors satisfies when some t_i != 1; the coefficients are drawn
// after the proofs are fixed.
#pragma once
#include "plonk.hpp"
#include "verify.hpp"

namespace cgh {

struct PlonkVerifyingKey {
    Curve c;
    size_t n_public = 0, power = 0;
    Fr k1, k2, omega;
    Bytes pts;                                  // Qm, Ql, Qr, Qo, Qc, S1, S2, S3: packed affine G1
    Bytes x2, g2, neg_g2, g1;                   // X_2; the generators (packed affine), -G_2
};

// validates the key's points and the domain; omega = the product's own 2^power-th root
static void prepare_plonk_vk(PlonkVerifyingKey& vk, const Fr* claimed_w) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1);
    static const char* names[8] = {"Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"};
    if (vk.pts.size() != 8 * g1 || vk.x2.size() != c.aff(CG_G2)) throw std::runtime_error("plonk verifying key: wrong point sizes");
    for (int i = 0; i < 8; i++) if (!point_valid(c, CG_G1, vk.pts.data() + i * g1)) throw std::runtime_error(std::string("plonk verifying key: ") + names[i] + " is not a valid G1 point");
    if (!point_valid(c, CG_G2, vk.x2.data())) throw std::runtime_error("plonk verifying key: X_2 is not a valid G2 point");
    const SnarkjsRoots& rt = snarkjs_roots_cached(c);
    if (vk.power > (size_t)rt.two_adicity) throw std::runtime_error("plonk verifying key: power " + std::to_string(vk.power) + " exceeds the field's two-adicity");
    vk.omega = rt.roots[vk.power];
    if (claimed_w && !fr_eq(*claimed_w, vk.omega)) throw std::runtime_error("plonk verifying key: w is not the domain's root of unity");
    int32_t ok = 0; const Fr ks[2] = {vk.k1, vk.k2};
    CG(cg_fr_is_canonical(c.id, ks, 2, &ok)); if (!ok) throw std::runtime_error("plonk verifying key: k1 / k2 not below the scalar modulus");
    vk.g1 = pt_to_affine(c, pt_generator(c, CG_G1));
    vk.g2 = pt_to_affine(c, pt_generator(c, CG_G2));
    vk.neg_g2 = neg_affine(c, CG_G2, vk.g2);
}

static size_t json_uint_after(const std::string& js, const char* key) {
    size_t pos = js.find(std::string("\"") + key + "\"");
    if (pos == std::string::npos) throw std::runtime_error(std::string("missing key ") + key);
    pos = js.find(':', pos);
    if (pos == std::string::npos) throw std::runtime_error(std::string("key without a value: ") + key);
    pos++;
    while (pos < js.size() && (js[pos] == ' ' || js[pos] == '\t' || js[pos] == '\n' || js[pos] == '\r' || js[pos] == '"')) pos++;
    if (pos >= js.size() || js[pos] < '0' || js[pos] > '9') throw std::runtime_error(std::string("not a number: ") + key);
    size_t v = 0;
    for (; pos < js.size() && js[pos] >= '0' && js[pos] <= '9'; pos++) { if (v > ((size_t)1 << 40)) throw std::runtime_error(std::string("number too large: ") + key); v = v * 10 + (size_t)(js[pos] - '0'); }
    return v;
}
static PlonkVerifyingKey plonk_vk_from_json(int curve_id, const std::string& path) {
    const Bytes raw = slurp(path);
    const std::string js(raw.begin(), raw.end());
    PlonkVerifyingKey vk; vk.c = Curve{curve_id};
    const Curve& c = vk.c;
    if (js.find("\"protocol\"") == std::string::npos || json_numbers_after(js, "protocol", 1)[0] != "plonk") throw std::runtime_error("not a plonk verification key");
    if (js.find("\"curve\"") == std::string::npos || json_numbers_after(js, "curve", 1)[0] != curve_name(c)) throw std::runtime_error("verification key is for another curve");
    const int nl = (int)c.fq() / 8;
    auto put = [&](const std::string& d, uint8_t* dst) { uint64_t can[6] = {0}; dec_to_limbs(d, can, nl); CG(cg_fq_from_canonical(c.id, can, dst, 1)); };
    auto fr = [&](const char* key) {
        uint64_t can[4] = {0}; dec_to_limbs(json_numbers_after(js, key, 1)[0], can, 4);
        int32_t ok = 0; CG(cg_fr_is_canonical(c.id, can, 1, &ok)); if (!ok) throw std::runtime_error(std::string(key) + " is not below the scalar modulus");
        Fr r; CG(cg_fr_from_canonical(c.id, can, r.v, 1)); return r;
    };
    vk.n_public = json_uint_after(js, "nPublic"); vk.power = json_uint_after(js, "power");
    vk.k1 = fr("k1"); vk.k2 = fr("k2");
    static const char* names[8] = {"Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"};
    vk.pts.assign(8 * c.aff(CG_G1), 0);
    for (int i = 0; i < 8; i++) {
        const auto v = json_array_strings(js, names[i]);
        if (v.size() != 3) throw std::runtime_error(std::string(names[i]) + ": a G1 point has three coordinates");
        uint8_t* dst = vk.pts.data() + i * c.aff(CG_G1);
        if (v[2] == "0") continue;                                                          // infinity: Qr and Qc of the multiplier2 keys
        if (v[2] != "1") throw std::runtime_error("only z = 1 / z = 0 G1 encodings are produced by circom tools");
        put(v[0], dst); put(v[1], dst + c.fq());
    }
    const auto x = json_array_strings(js, "X_2");
    if (x.size() != 6) throw std::runtime_error("X_2: a G2 point has six coordinates");
    vk.x2.assign(c.aff(CG_G2), 0);
    if (!(x[4] == "0" && x[5] == "0")) {
        if (x[4] != "1" || x[5] != "0") throw std::runtime_error("only z = (1, 0) G2 encodings are produced by circom tools");
        for (int i = 0; i < 4; i++) put(x[i], vk.x2.data() + i * c.fq());
    }
    const Fr w = fr("w");
    prepare_plonk_vk(vk, &w);
    return vk;
}
static PlonkVerifyingKey plonk_vk_from_zkey_data(const PlonkZKey& z) {
    PlonkVerifyingKey vk; vk.c = z.curve;
    vk.n_public = z.n_public; vk.power = z.power; vk.k1 = z.k1; vk.k2 = z.k2; vk.pts = z.vk_g1; vk.x2 = z.x_2;
    prepare_plonk_vk(vk, nullptr);
    return vk;
}

static void plonk_check_public(const PlonkVerifyingKey& vk, const uint64_t* pub, size_t n_pub, size_t n_proofs) {
    if (n_pub != vk.n_public) throw std::runtime_error("plonk verify: " + std::to_string(n_pub) + " public inputs for a key with " + std::to_string(vk.n_public));
    if (n_pub && n_proofs) { int32_t ok = 0; CG(cg_fr_is_canonical(vk.c.id, pub, n_pub * n_proofs, &ok)); if (!ok) throw std::runtime_error("plonk verify: a public input is not below the scalar modulus"); }
}
// what the reference's proof parser checks (circom-types/src/plonk/proof.rs through traits.rs:107-155): coordinates below q, on the curve, in the subgroup; evaluations below r
static bool plonk_proof_wellformed(const PlonkVerifyingKey& vk, const uint8_t* commits, const uint64_t* evals) {
    const Curve& c = vk.c;
    if (!coords_below_modulus(c, commits, 18)) return false;
    for (int i = 0; i < 9; i++) if (!point_valid(c, CG_G1, commits + i * c.aff(CG_G1))) return false;
    int32_t ok = 0; CG(cg_fr_is_canonical(c.id, evals, 6, &ok));
    return ok != 0;
}
struct PlonkScalars { std::vector<Fr> ch, sp, sk; std::vector<int32_t> valid; Fr sums[9]; };
static PlonkScalars plonk_scalars(cg_ctx* ctx, const PlonkVerifyingKey& vk, const uint8_t* commits, const uint64_t* evals, const uint64_t* pubs, size_t n, const uint64_t* r128) {
    PlonkScalars s; s.ch.resize(6 * n); s.sp.resize(11 * n); s.sk.resize(9 * n); s.valid.resize(n);
    if (ctx) CG(cg_plonk_verify_scalars(ctx, vk.c.id, vk.pts.data(), vk.k1.v, vk.k2.v, vk.omega.v, (int32_t)vk.power, commits, evals, pubs, vk.n_public, n, r128,
                                        s.ch.data(), s.sp.data(), s.sk.data(), s.valid.data(), s.sums));
    else CG(cg_plonk_verify_scalars_host(vk.c.id, vk.pts.data(), vk.k1.v, vk.k2.v, vk.omega.v, (int32_t)vk.power, commits, evals, pubs, vk.n_public, n, r128,
                                         s.ch.data(), s.sp.data(), s.sk.data(), s.valid.data(), s.sums));
    return s;
}
// sum_k key_scalar[k] * key point k, the generator last
static Point plonk_key_part(const PlonkVerifyingKey& vk, const Fr* sk) {
    const Curve& c = vk.c;
    Point acc = pt_mul_generator(c, CG_G1, sk[8]);
    for (int k = 0; k < 8; k++) acc = pt_add(c, acc, pt_mul(c, pt_from_affine(c, CG_G1, vk.pts.data() + k * c.aff(CG_G1)), sk[k]));
    return acc;
}
// e(A, X_2) e(-B, G_2) == 1
static bool plonk_pairing_check(const PlonkVerifyingKey& vk, const Point& a, const Point& b) {
    const Curve& c = vk.c;
    Bytes g1s = pt_to_affine(c, a), g2s = vk.x2;
    const Bytes nb = pt_to_affine(c, pt_neg(c, b));
    g1s.insert(g1s.end(), nb.begin(), nb.end()); g2s.insert(g2s.end(), vk.g2.begin(), vk.g2.end());
    int32_t ok = 0; CG(cg_pairing_check(c.id, g1s.data(), g2s.data(), 2, &ok));
    return ok != 0;
}

static bool plonk_verify(const PlonkVerifyingKey& vk, const uint8_t* commits, const uint64_t* evals, const uint64_t* pub, size_t n_pub) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1);
    plonk_check_public(vk, pub, n_pub, 1);
    if (!plonk_proof_wellformed(vk, commits, evals)) return false;
    const PlonkScalars s = plonk_scalars(nullptr, vk, commits, evals, pub, 1, nullptr);
    if (!s.valid[0]) return false;
    auto term = [&](int commit, const Fr& k) { return pt_mul(c, pt_from_affine(c, CG_G1, commits + commit * g1), k); };
    const Point a1 = pt_add(c, term(7, s.sp[0]), term(8, s.sp[1]));
    Point b1 = plonk_key_part(vk, s.sk.data());
    for (int k = 0; k < 9; k++) b1 = pt_add(c, b1, term(k, s.sp[2 + k]));
    return plonk_pairing_check(vk, a1, b1);
}

// seconds (optional, 5): point checks, scalar kernel, A-side MSM, B-side MSM, host tail
static bool plonk_verify_batch(int device, const PlonkVerifyingKey& vk, const uint8_t* commits, const uint64_t* evals, const uint64_t* pubs, size_t n_pub, size_t n,
                               const uint8_t* seed32, uint8_t* per_proof, double* seconds) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1);
    plonk_check_public(vk, pubs, n_pub, n);
    if (seconds) for (int i = 0; i < 5; i++) seconds[i] = 0;
    if (n == 0) return true;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](int slot, std::chrono::steady_clock::time_point& t0) { const auto t1 = now(); if (seconds) seconds[slot] += std::chrono::duration<double>(t1 - t0).count(); t0 = t1; };
    // coefficients: r_0 = 1, the others 128 bits of the ChaCha12 stream (drawn as groth16_verify_batch draws them)
    uint8_t seed[32];
    if (seed32) memcpy(seed, seed32, 32);
    else { std::random_device rd; for (int i = 0; i < 8; i++) { const uint32_t w = rd(); memcpy(seed + 4 * i, &w, 4); } }
    ChaCha12 rng(seed);
    std::vector<uint64_t> r128(2 * n);
    for (size_t i = 0; i < n; i++) { r128[2 * i] = i ? rng.next_u64() : 1; r128[2 * i + 1] = i ? rng.next_u64() : 0; }
    auto t0 = now();                                                                        // (the context's creation counts with the point checks)
    VerifyCtx cx; CG(cg_ctx_create(device, &cx.ctx));
    // on the curve and in the subgroup: the passes of the zkey validation, over the 9n commitments; then the evaluations below r
    bool points_ok = coords_below_modulus(c, commits, n * 18);
    VerifyBases ba, bb;
    if (points_ok) {
        CG(cg_bases_register(cx.ctx, c.id, CG_G1, commits, 9 * n, g1, -1, &bb.b));
        uint64_t bad = 0;
        CG(cg_bases_check_on_curve(cx.ctx, bb.b, &bad, nullptr)); if (bad) points_ok = false;
        if (points_ok) { CG(cg_bases_check_subgroup(cx.ctx, bb.b, &bad, nullptr)); if (bad) points_ok = false; }
    }
    bool accept = points_ok;
    if (accept) { int32_t ok = 0; CG(cg_fr_is_canonical(c.id, evals, 6 * n, &ok)); accept = ok != 0; }
    lap(0, t0);
    if (accept) {
        const PlonkScalars s = plonk_scalars(cx.ctx, vk, commits, evals, pubs, n, r128.data());
        for (size_t i = 0; i < n; i++) if (!s.valid[i]) accept = false;
        lap(1, t0);
        if (accept) {
            Bytes as(2 * n * g1); std::vector<Fr> sa(2 * n), sb(9 * n);
            for (size_t i = 0; i < n; i++) {
                memcpy(&as[2 * i * g1], commits + (9 * i + 7) * g1, 2 * g1);
                sa[2 * i] = s.sp[11 * i]; sa[2 * i + 1] = s.sp[11 * i + 1];
                for (int k = 0; k < 9; k++) sb[9 * i + k] = s.sp[11 * i + 2 + k];
            }
            Point sum_a{Bytes(c.jac(CG_G1)), CG_G1}, sum_b{Bytes(c.jac(CG_G1)), CG_G1};
            CG(cg_bases_register(cx.ctx, c.id, CG_G1, as.data(), 2 * n, g1, -1, &ba.b));
            const void* pa[1] = {sa.data()}; const void* pb[1] = {sb.data()};
            CG(cg_msm(cx.ctx, ba.b, 0, 2 * n, pa, 1, sum_a.b.data()));
            lap(2, t0);
            CG(cg_msm(cx.ctx, bb.b, 0, 9 * n, pb, 1, sum_b.b.data()));
            lap(3, t0);
            accept = plonk_pairing_check(vk, sum_a, pt_add(c, sum_b, plonk_key_part(vk, s.sums)));
            lap(4, t0);
        }
    }
    if (per_proof) {
        if (accept) memset(per_proof, 1, n);
        else {   // every proof on its own: A1_i and B1_i as linear combinations on the device, two Miller loops and a final exponentiation per lane
            std::vector<uint8_t> wellformed(n);
            Bytes cm(commits, commits + 9 * n * g1); std::vector<uint64_t> ev(evals, evals + 24 * n), pb(pubs ? pubs : nullptr, pubs ? pubs + 4 * n * n_pub : nullptr);
            for (size_t i = 0; i < n; i++) {
                if (points_ok) { int32_t ok = 0; CG(cg_fr_is_canonical(c.id, evals + 24 * i, 6, &ok)); wellformed[i] = ok != 0; }   // (the device passes accepted every commitment)
                else wellformed[i] = plonk_proof_wellformed(vk, commits + 9 * i * g1, evals + 24 * i);
                if (!wellformed[i]) { memset(&cm[9 * i * g1], 0, 9 * g1); memset(&ev[24 * i], 0, 24 * 8); }   // (points at infinity: the lanes compute 1 and the proof is flagged 0 below)
            }
            const PlonkScalars s = plonk_scalars(cx.ctx, vk, cm.data(), ev.data(), pb.data(), n, nullptr);
            Bytes pa(2 * n * g1), pbb(20 * n * g1, 0), a1(n * g1), b1(n * g1);
            std::vector<Fr> sa(2 * n), sb(20 * n);
            for (size_t i = 0; i < n; i++) {
                memcpy(&pa[2 * i * g1], &cm[(9 * i + 7) * g1], 2 * g1);
                sa[2 * i] = s.sp[11 * i]; sa[2 * i + 1] = s.sp[11 * i + 1];
                if (wellformed[i] && s.valid[i]) {
                    memcpy(&pbb[20 * i * g1], &cm[9 * i * g1], 9 * g1); memcpy(&pbb[(20 * i + 9) * g1], vk.pts.data(), 8 * g1); memcpy(&pbb[(20 * i + 17) * g1], vk.g1.data(), g1);
                } else memset(&pa[2 * i * g1], 0, 2 * g1);
                for (int k = 0; k < 9; k++) { sb[20 * i + k] = s.sp[11 * i + 2 + k]; sb[20 * i + 9 + k] = s.sk[9 * i + k]; }
                sb[20 * i + 18] = sb[20 * i + 19] = fr_from_u64(c, 0);                      // (K = 20: the 18 terms and two idle ones)
            }
            CG(cg_g1_lincomb_batch(cx.ctx, c.id, pa.data(), sa.data(), n, 2, a1.data()));
            CG(cg_g1_lincomb_batch(cx.ctx, c.id, pbb.data(), sb.data(), n, 20, b1.data()));
            Bytes g1s(2 * n * g1), g2s(2 * n * c.aff(CG_G2));
            for (size_t i = 0; i < n; i++) {   // e(A1, X_2) e(B1, -G_2)
                memcpy(&g1s[2 * i * g1], &a1[i * g1], g1); memcpy(&g1s[(2 * i + 1) * g1], &b1[i * g1], g1);
                memcpy(&g2s[2 * i * c.aff(CG_G2)], vk.x2.data(), c.aff(CG_G2)); memcpy(&g2s[(2 * i + 1) * c.aff(CG_G2)], vk.neg_g2.data(), c.aff(CG_G2));
            }
            const size_t fp12 = 12 * c.fq();
            Bytes vals(2 * n * fp12), one(fp12); std::vector<int32_t> ok(n);
            CG(cg_miller_loop(c.id, nullptr, nullptr, 0, one.data()));
            CG(cg_miller_batch(cx.ctx, c.id, g1s.data(), g2s.data(), 2 * n, vals.data()));
            CG(cg_final_exp_check_batch(cx.ctx, c.id, vals.data(), 2, n, one.data(), ok.data()));
            for (size_t i = 0; i < n; i++) per_proof[i] = wellformed[i] && s.valid[i] && ok[i] ? 1 : 0;
        }
    }
    return accept;
}

}  // namespace cgh
