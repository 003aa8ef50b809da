// Groth16 verification (co-circom/co-groth16/src/verifier.rs:23-43, which wraps ark-groth16's prepare_verifying_key + verify_proof) over
// the C ABI's pairing layer: verifying-key handles from a verification_key.json (circom-types/src/groth16/verification_key.rs) or a
// zkey, the single-proof check on the host, and the randomised batch check on the GPU.
//
// Single proof: accept iff e(A, B) e(vk_x, -gamma) e(C, -delta) == e(alpha, beta), vk_x = IC_0 + sum pub_i IC_(i+1): three Miller
// loops, one final exponentiation, compared with the prepared e(alpha, beta).
// Batch of n proofs under one key: with r_0 = 1 and r_1.. uniform 128-bit coefficients,
//     FE( prod_i Miller(r_i A_i, B_i) * Miller(sum_i r_i vk_x_i, -gamma) * Miller(sum_i r_i C_i, -delta) ) == e(alpha, beta)^(sum_i r_i).
// If every proof satisfies its equation the product does too.  If some proof does not, write the i-th equation as t_i = 1 in the target
// group (order r, prime): the batch accepts iff prod t_i^(r_i) = 1, a non-trivial linear relation over F_r in the exponents' r_i, which
// at most a 2^-128 fraction of the coefficient vectors satisfies (Schwartz-Zippel in one variable, the others fixed).  The coefficients
// are drawn after the proofs are fixed (ChaCha12 from the caller's seed or from OS entropy), so a forger cannot aim at them.
#pragma once
#include "codecs.hpp"
#include "chacha.hpp"
#include <random>

namespace cgh {

struct VerifyingKey {
    Curve c;
    Bytes alpha1, beta2, gamma2, delta2, neg_gamma2, neg_delta2;     // packed affine
    std::vector<uint8_t> ic; size_t n_ic = 0;                         // n_ic packed affine G1 points, back to back
    Bytes alphabeta;                                                  // e(alpha, beta), computed
    size_t fp12() const { return 12 * c.fq(); }
    size_t proof_bytes() const { return 2 * c.aff(CG_G1) + c.aff(CG_G2); }
};

static Bytes neg_affine(const Curve& c, int g, const Bytes& aff) { return pt_to_affine(c, pt_neg(c, pt_from_affine(c, g, aff.data()))); }
static bool point_valid(const Curve& c, int g, const uint8_t* aff) { int32_t ok = 0; CG(cg_point_validate(c.id, g, aff, &ok)); return ok != 0; }

// validates the key's points and prepares what ark_groth16::prepare_verifying_key prepares
static void prepare_vk(VerifyingKey& vk) {
    const Curve& c = vk.c;
    if (vk.n_ic < 1 || vk.ic.size() != vk.n_ic * c.aff(CG_G1)) throw std::runtime_error("verifying key: IC must hold at least one point");
    if (!point_valid(c, CG_G1, vk.alpha1.data())) throw std::runtime_error("verifying key: alpha_1 is not a valid G1 point");
    const Bytes* g2s[3] = {&vk.beta2, &vk.gamma2, &vk.delta2}; const char* names[3] = {"beta_2", "gamma_2", "delta_2"};
    for (int i = 0; i < 3; i++) if (!point_valid(c, CG_G2, g2s[i]->data())) throw std::runtime_error(std::string("verifying key: ") + names[i] + " is not a valid G2 point");
    for (size_t i = 0; i < vk.n_ic; i++) if (!point_valid(c, CG_G1, vk.ic.data() + i * c.aff(CG_G1))) throw std::runtime_error("verifying key: IC[" + std::to_string(i) + "] is not a valid G1 point");
    vk.neg_gamma2 = neg_affine(c, CG_G2, vk.gamma2); vk.neg_delta2 = neg_affine(c, CG_G2, vk.delta2);
    vk.alphabeta.resize(vk.fp12());
    CG(cg_pairing(c.id, vk.alpha1.data(), vk.beta2.data(), vk.alphabeta.data()));
}

// the quoted strings of the JSON array that follows `key` (nested arrays flattened)
static std::vector<std::string> json_array_strings(const std::string& js, const char* key) {
    size_t pos = js.find(std::string("\"") + key + "\"");
    if (pos == std::string::npos) throw std::runtime_error(std::string("missing key ") + key);
    pos = js.find('[', pos);
    if (pos == std::string::npos) throw std::runtime_error(std::string("key without an array: ") + key);
    std::vector<std::string> out; int depth = 0;
    for (; pos < js.size(); pos++) {
        const char ch = js[pos];
        if (ch == '[') depth++;
        else if (ch == ']') { if (--depth == 0) return out; }
        else if (ch == '"') { const size_t q1 = js.find('"', pos + 1); if (q1 == std::string::npos) break; out.push_back(js.substr(pos + 1, q1 - pos - 1)); pos = q1; }
    }
    throw std::runtime_error(std::string("truncated array: ") + key);
}
static VerifyingKey vk_from_json(int curve_id, const std::string& path) {
    const Bytes raw = slurp(path);
    const std::string js(raw.begin(), raw.end());
    VerifyingKey vk; vk.c = Curve{curve_id};
    const Curve& c = vk.c;
    if (js.find("\"groth16\"") == std::string::npos) throw std::runtime_error("not a groth16 verification key");
    if (js.find(std::string("\"") + curve_name(c) + "\"") == std::string::npos) throw std::runtime_error("verification key is for another curve");
    const int nl = (int)c.fq() / 8;
    auto put = [&](const std::string& d, uint8_t* dst) { uint64_t can[6] = {0}; dec_to_limbs(d, can, nl); CG(cg_fq_from_canonical(c.id, can, dst, 1)); };
    auto g1 = [&](const std::string* v, uint8_t* dst) {
        if (v[2] == "0") { memset(dst, 0, c.aff(CG_G1)); return; }
        if (v[2] != "1") throw std::runtime_error("only z = 1 / z = 0 G1 encodings are produced by circom tools");
        put(v[0], dst); put(v[1], dst + c.fq());
    };
    auto g2 = [&](const char* key) {
        const auto v = json_array_strings(js, key);
        if (v.size() != 6) throw std::runtime_error(std::string(key) + ": a G2 point has six coordinates");
        Bytes b(c.aff(CG_G2), 0);
        if (v[4] == "0" && v[5] == "0") return b;
        if (v[4] != "1" || v[5] != "0") throw std::runtime_error("only z = (1, 0) G2 encodings are produced by circom tools");
        for (int i = 0; i < 4; i++) put(v[i], b.data() + i * c.fq());
        return b;
    };
    const auto a = json_array_strings(js, "vk_alpha_1");
    if (a.size() != 3) throw std::runtime_error("vk_alpha_1: a G1 point has three coordinates");
    vk.alpha1.assign(c.aff(CG_G1), 0); g1(a.data(), vk.alpha1.data());
    vk.beta2 = g2("vk_beta_2"); vk.gamma2 = g2("vk_gamma_2"); vk.delta2 = g2("vk_delta_2");
    const auto ic = json_array_strings(js, "IC");
    if (ic.empty() || ic.size() % 3) throw std::runtime_error("IC: a sequence of G1 points with three coordinates each");
    vk.n_ic = ic.size() / 3; vk.ic.assign(vk.n_ic * c.aff(CG_G1), 0);
    for (size_t i = 0; i < vk.n_ic; i++) g1(ic.data() + 3 * i, vk.ic.data() + i * c.aff(CG_G1));
    prepare_vk(vk);
    return vk;
}
static VerifyingKey vk_from_zkey_data(const ZKey& z) {
    VerifyingKey vk; vk.c = z.curve;
    vk.alpha1 = z.alpha_g1; vk.beta2 = z.beta_g2; vk.gamma2 = z.gamma_g2; vk.delta2 = z.delta_g2;
    vk.n_ic = z.n_public + 1; vk.ic.assign(z.ic.begin(), z.ic.end());
    prepare_vk(vk);
    return vk;
}

static bool coords_below_modulus(const Curve& c, const uint8_t* p, size_t n_coords) {
    const int nl = (int)c.fq() / 8;
    for (size_t k = 0; k < n_coords; k++) {
        uint64_t v[6]; memcpy(v, p + k * c.fq(), c.fq());
        bool below = false;
        for (int l = nl - 1; l >= 0; l--) { if (v[l] != MOD_Q[c.id][l]) { below = v[l] < MOD_Q[c.id][l]; break; } }
        if (!below) return false;
    }
    return true;
}
// the error statuses shared by the single and the batch entry: public-input count and canonical form
static void check_public(const VerifyingKey& vk, const uint64_t* pub, size_t n_pub, size_t n_proofs) {
    if (n_pub != vk.n_ic - 1) throw std::runtime_error("verify: " + std::to_string(n_pub) + " public inputs for a key with " + std::to_string(vk.n_ic - 1));
    if (n_pub && n_proofs) { int32_t ok = 0; CG(cg_fr_is_canonical(vk.c.id, pub, n_pub * n_proofs, &ok)); if (!ok) throw std::runtime_error("verify: a public input is not below the scalar modulus"); }
}
// what the reference's proof parser checks per point (traits.rs:107-155)
static bool proof_points_valid(const VerifyingKey& vk, const uint8_t* proof) {
    const Curve& c = vk.c;
    return point_valid(c, CG_G1, proof) && point_valid(c, CG_G2, proof + c.aff(CG_G1)) && point_valid(c, CG_G1, proof + c.aff(CG_G1) + c.aff(CG_G2));
}
static Bytes vk_x_affine(const VerifyingKey& vk, const uint64_t* pub) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1);
    Point acc = pt_from_affine(c, CG_G1, vk.ic.data());
    for (size_t i = 0; i + 1 < vk.n_ic; i++) { Fr k; memcpy(k.v, pub + 4 * i, 32); acc = pt_add(c, acc, pt_mul(c, pt_from_affine(c, CG_G1, vk.ic.data() + (i + 1) * g1), k)); }
    return pt_to_affine(c, acc);
}
// g1s / g2s of the three pairs (A, B), (vk_x, -gamma), (C, -delta) appended to the two arrays
static void append_pairs(const VerifyingKey& vk, const uint8_t* proof, const Bytes& vkx, Bytes& g1s, Bytes& g2s) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1), g2 = c.aff(CG_G2);
    g1s.insert(g1s.end(), proof, proof + g1); g2s.insert(g2s.end(), proof + g1, proof + g1 + g2);
    g1s.insert(g1s.end(), vkx.begin(), vkx.end()); g2s.insert(g2s.end(), vk.neg_gamma2.begin(), vk.neg_gamma2.end());
    g1s.insert(g1s.end(), proof + g1 + g2, proof + 2 * g1 + g2); g2s.insert(g2s.end(), vk.neg_delta2.begin(), vk.neg_delta2.end());
}

static bool groth16_verify(const VerifyingKey& vk, const uint8_t* proof, const uint64_t* pub, size_t n_pub) {
    check_public(vk, pub, n_pub, 1);
    if (!proof_points_valid(vk, proof)) return false;
    Bytes g1s, g2s; append_pairs(vk, proof, vk_x_affine(vk, pub), g1s, g2s);
    Bytes m(vk.fp12()), e(vk.fp12());
    CG(cg_miller_loop(vk.c.id, g1s.data(), g2s.data(), 3, m.data()));
    CG(cg_final_exp(vk.c.id, m.data(), e.data()));
    return e == vk.alphabeta;
}

struct VerifyCtx { cg_ctx* ctx = nullptr; ~VerifyCtx() { if (ctx) cg_ctx_destroy(ctx); } };
struct VerifyBases { cg_bases* b = nullptr; ~VerifyBases() { if (b) cg_bases_release(b); } };

// seconds (optional, 5): point checks, Miller kernel + product, MSM of the C points, MSM over IC (with the host's scalar sums), host tail
static bool groth16_verify_batch(int device, const VerifyingKey& vk, const uint8_t* proofs, const uint64_t* pubs, size_t n_pub, size_t n, const uint8_t* seed32,
                                 uint8_t* per_proof, double* seconds) {
    const Curve& c = vk.c; const size_t g1 = c.aff(CG_G1), g2 = c.aff(CG_G2), pb = vk.proof_bytes();
    check_public(vk, pubs, n_pub, n);
    if (seconds) for (int i = 0; i < 5; i++) seconds[i] = 0;
    if (n == 0) return true;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](int slot, std::chrono::steady_clock::time_point& t0) { const auto t1 = now(); if (seconds) seconds[slot] += std::chrono::duration<double>(t1 - t0).count(); t0 = t1; };
    // coefficients: r_0 = 1, the others 128 bits of the ChaCha12 stream
    uint8_t seed[32];
    if (seed32) memcpy(seed, seed32, 32);
    else { std::random_device rd; for (int i = 0; i < 8; i++) { const uint32_t w = rd(); memcpy(seed + 4 * i, &w, 4); } }
    ChaCha12 rng(seed);
    std::vector<uint64_t> r128(2 * n); std::vector<Fr> r_can(n), r(n);
    for (size_t i = 0; i < n; i++) {
        r128[2 * i] = i ? rng.next_u64() : 1; r128[2 * i + 1] = i ? rng.next_u64() : 0;
        r_can[i] = Fr{{r128[2 * i], r128[2 * i + 1], 0, 0}};
    }
    CG(cg_fr_from_canonical(c.id, r_can.data(), r.data(), n));
    Bytes as(n * g1), bs(n * g2), cs(n * g1);
    for (size_t i = 0; i < n; i++) { const uint8_t* p = proofs + i * pb; memcpy(&as[i * g1], p, g1); memcpy(&bs[i * g2], p + g1, g2); memcpy(&cs[i * g1], p + g1 + g2, g1); }
    auto t0 = now();                                                                        // (the context's creation counts with the point checks)
    VerifyCtx cx; CG(cg_ctx_create(device, &cx.ctx));
    bool accept = coords_below_modulus(c, proofs, n * 8);                                  // (a proof is 8 base-field coordinates)
    VerifyBases ba, bb, bc, bic;
    if (accept) {   // on the curve and in the subgroup: the passes of the zkey validation, over the A, B, C arrays
        CG(cg_bases_register(cx.ctx, c.id, CG_G1, as.data(), n, g1, -1, &ba.b));
        CG(cg_bases_register(cx.ctx, c.id, CG_G2, bs.data(), n, g2, -1, &bb.b));
        CG(cg_bases_register(cx.ctx, c.id, CG_G1, cs.data(), n, g1, -1, &bc.b));
        for (cg_bases* t : {ba.b, bb.b, bc.b}) {
            uint64_t bad = 0;
            CG(cg_bases_check_on_curve(cx.ctx, t, &bad, nullptr)); if (bad) { accept = false; break; }
            CG(cg_bases_check_subgroup(cx.ctx, t, &bad, nullptr)); if (bad) { accept = false; break; }
        }
    }
    lap(0, t0);
    if (accept) {
        Bytes F(vk.fp12());
        CG(cg_miller_product(cx.ctx, c.id, as.data(), bs.data(), r128.data(), n, F.data()));
        lap(1, t0);
        const void* sc[1] = {r.data()};
        Point sum_c{Bytes(c.jac(CG_G1)), CG_G1}, sum_x{Bytes(c.jac(CG_G1)), CG_G1};
        CG(cg_msm(cx.ctx, bc.b, 0, n, sc, 1, sum_c.b.data()));
        lap(2, t0);
        // sum_i r_i vk_x_i = (sum r_i) IC_0 + sum_j (sum_i r_i pub_ij) IC_(j+1)
        std::vector<Fr> s(vk.n_ic);
        s[0] = fr_from_u64(c, 0); for (size_t i = 0; i < n; i++) s[0] = fr_add(c, s[0], r[i]);
        for (size_t j = 0; j < n_pub; j++) {
            Fr acc = fr_from_u64(c, 0);
            for (size_t i = 0; i < n; i++) { Fr p; memcpy(p.v, pubs + 4 * (i * n_pub + j), 32); acc = fr_add(c, acc, fr_mul(c, r[i], p)); }
            s[j + 1] = acc;
        }
        CG(cg_bases_register(cx.ctx, c.id, CG_G1, vk.ic.data(), vk.n_ic, g1, -1, &bic.b));
        const void* ss[1] = {s.data()};
        CG(cg_msm(cx.ctx, bic.b, 0, vk.n_ic, ss, 1, sum_x.b.data()));
        lap(3, t0);
        Bytes g1s, g2s;
        const Bytes ax = pt_to_affine(c, sum_x), ac = pt_to_affine(c, sum_c);
        g1s.insert(g1s.end(), ax.begin(), ax.end()); g2s.insert(g2s.end(), vk.neg_gamma2.begin(), vk.neg_gamma2.end());
        g1s.insert(g1s.end(), ac.begin(), ac.end()); g2s.insert(g2s.end(), vk.neg_delta2.begin(), vk.neg_delta2.end());
        Bytes m(vk.fp12()), t(vk.fp12()), e(vk.fp12()), want(vk.fp12());
        CG(cg_miller_loop(c.id, g1s.data(), g2s.data(), 2, m.data()));
        CG(cg_fp12_mul(c.id, F.data(), m.data(), t.data()));
        CG(cg_final_exp(c.id, t.data(), e.data()));
        Fr s0; CG(cg_fr_to_canonical(c.id, s[0].v, s0.v, 1));
        CG(cg_fp12_pow(c.id, vk.alphabeta.data(), s0.v, 4, want.data()));
        accept = e == want;
        lap(4, t0);
    }
    if (per_proof) {
        if (accept) memset(per_proof, 1, n);
        else {   // every proof on its own: three Miller loops and a final exponentiation per lane
            Bytes g1s, g2s; std::vector<uint8_t> valid(n);
            const Bytes inf1(g1, 0), zero_proof(pb, 0);
            for (size_t i = 0; i < n; i++) {
                const uint8_t* p = proofs + i * pb;
                valid[i] = coords_below_modulus(c, p, 8) && proof_points_valid(vk, p);
                if (valid[i]) append_pairs(vk, p, vk_x_affine(vk, pubs + 4 * i * n_pub), g1s, g2s);
                else append_pairs(vk, zero_proof.data(), inf1, g1s, g2s);           // (points at infinity: the lane computes 1 and is flagged 0 below)
            }
            Bytes vals(3 * n * vk.fp12()); std::vector<int32_t> ok(n);
            CG(cg_miller_batch(cx.ctx, c.id, g1s.data(), g2s.data(), 3 * n, vals.data()));
            CG(cg_final_exp_check_batch(cx.ctx, c.id, vals.data(), 3, n, vk.alphabeta.data(), ok.data()));
            for (size_t i = 0; i < n; i++) per_proof[i] = valid[i] && ok[i] ? 1 : 0;
        }
    }
    return accept;
}

}  // namespace cgh
