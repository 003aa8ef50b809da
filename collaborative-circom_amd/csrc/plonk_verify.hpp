// Plonk verification, the per-proof part, host and device from one source: Keccak-256, the reference's Fiat-Shamir transcript
// (co-plonk/src/types.rs:122-176), the six challenges of co-plonk/src/plonk.rs:47-122 and the scalar algebra of plonk.rs:133-271 that
// turns one proof into the coefficients of two linear combinations of G1 points:
//     A1 = wxi + u wxiw
//     B1 = sum over the proof's nine commitments + sum over the key's eight points + (-e) G        (table below)
// The proof satisfies plonk.rs:254-271 iff e(A1, X_2) e(-B1, G_2) = 1.  Nothing here touches a curve point except to hash it: the
// point arithmetic is the caller's (20 scalar multiplications for one proof, two MSMs for a batch).
//
//   A-side (2)             wxi: 1            wxiw: u
//   B-side, proof (9)      a: v    b: v^2    c: v^3    z: d2a + e2 + u    t1: -z_h    t2: -z_h xi^n    t3: -z_h xi^2n    wxi: xi    wxiw: u xi omega
//   B-side, key (9)        Qm: a b   Ql: a   Qr: b   Qo: c   Qc: 1   S1: v^4   S2: v^5   S3: -e3a e3b alpha beta zw   G: -e
// (a, b, c, s1, s2, zw on the right-hand sides are the proof's evaluations; e2, e3a, e3b, d2a, r0 as in calculate_r0_d, e as in calculate_e.)
#pragma once
#include "curve.hpp"

namespace cg {

// ---- Keccak-256 (rate 136, pad 0x01 .. 0x80: the original Keccak, what sha3::Keccak256 computes) ------------------------------------
// Every lane index and rotation count below is a compile-time constant once the 5 x 5 loops are unrolled, so the 25-word state (and
// the rho/pi copy) stays in registers: a state walked with run-time indices would be placed in scratch memory.
constexpr uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
constexpr int KECCAK_ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // [x + 5 y]
constexpr int KECCAK_RATE_WORDS = 17;

template <int S> CG_HD uint64_t keccak_rotl(uint64_t v) { if constexpr (S == 0) return v; else return (v << S) | (v >> (64 - S)); }
// B[y, 2x + 3y] = rotl(A[x, y], r[x, y]), one lane per instantiation
template <int I> CG_HD void keccak_rho_pi(const uint64_t (&a)[25], uint64_t (&b)[25]) {
    constexpr int x = I % 5, y = I / 5;
    b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rotl<KECCAK_ROT[I]>(a[I]);
    if constexpr (I + 1 < 25) keccak_rho_pi<I + 1>(a, b);
}
CG_HD void keccak_f1600(uint64_t (&a)[25]) {
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
        _Pragma("unroll") for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
        _Pragma("unroll") for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ keccak_rotl<1>(c[(x + 1) % 5]);
            _Pragma("unroll") for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
        }
        keccak_rho_pi<0>(a, b);
        _Pragma("unroll") for (int y = 0; y < 25; y += 5) {
            _Pragma("unroll") for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        }
        a[0] ^= KECCAK_RC[round];
    }
}
CG_HD uint64_t bswap64(uint64_t v) {
    v = ((v & 0x00ff00ff00ff00ffull) << 8) | ((v >> 8) & 0x00ff00ff00ff00ffull);
    v = ((v & 0x0000ffff0000ffffull) << 16) | ((v >> 16) & 0x0000ffff0000ffffull);
    return (v << 32) | (v >> 32);
}

// One transcript.  Everything the reference absorbs is a whole number of 64-bit words (32-byte scalars, 2 x 32 or 2 x 48-byte points), so
// the sponge works on words: word k of the stream is the byte-swapped limb the big-endian encoding puts there.
template <class Fr>
struct PlonkTranscript {
    uint64_t a[25]; int pos;
    CG_HD PlonkTranscript() : pos(0) { _Pragma("unroll") for (int i = 0; i < 25; i++) a[i] = 0; }
    // a[pos] ^= w with the index as a constant in every arm (pos is the same in every lane: a scalar branch on the device)
    CG_HD void absorb_word(uint64_t w) {
        switch (pos) {
            case 0: a[0] ^= w; break;   case 1: a[1] ^= w; break;   case 2: a[2] ^= w; break;   case 3: a[3] ^= w; break;
            case 4: a[4] ^= w; break;   case 5: a[5] ^= w; break;   case 6: a[6] ^= w; break;   case 7: a[7] ^= w; break;
            case 8: a[8] ^= w; break;   case 9: a[9] ^= w; break;   case 10: a[10] ^= w; break; case 11: a[11] ^= w; break;
            case 12: a[12] ^= w; break; case 13: a[13] ^= w; break; case 14: a[14] ^= w; break; case 15: a[15] ^= w; break;
            default: a[16] ^= w; break;
        }
        if (++pos == KECCAK_RATE_WORDS) { keccak_f1600(a); pos = 0; }
    }
    // a field element in Montgomery form, as its canonical value's big-endian bytes
    template <class F> CG_HD void add_field(const F& m) {
        const F c = m.from_mont();
        _Pragma("unroll") for (int j = F::N / 2 - 1; j >= 0; j--) absorb_word(bswap64(((uint64_t)c.v[2 * j + 1] << 32) | c.v[2 * j]));
    }
    CG_HD void add_scalar(const Fr& s) { add_field(s); }
    // x || y; the point at infinity is all zero bytes, which is what its packed form (0, 0) encodes to
    template <class Fq> CG_HD void add_point(const Affine<Fq>& p) { add_field(p.x); add_field(p.y); }
};

// Padding and challenge.  The stream ends on a word boundary: 0x01 opens word `pos`, 0x80 closes the block (the same word when pos = 16;
// a stream that ends on a block boundary gets a block of padding alone).  The digest is read as a big-endian 256-bit integer and reduced
// mod r (it can be up to ~5 r for BN254, ~2 r for BLS12-381), then brought to Montgomery form.
template <class Fr>
CG_HD Fr plonk_transcript_finish(PlonkTranscript<Fr>& t) {
    uint64_t w16 = 0x8000000000000000ull;
    switch (t.pos) {
        case 0: t.a[0] ^= 1; break;   case 1: t.a[1] ^= 1; break;   case 2: t.a[2] ^= 1; break;   case 3: t.a[3] ^= 1; break;
        case 4: t.a[4] ^= 1; break;   case 5: t.a[5] ^= 1; break;   case 6: t.a[6] ^= 1; break;   case 7: t.a[7] ^= 1; break;
        case 8: t.a[8] ^= 1; break;   case 9: t.a[9] ^= 1; break;   case 10: t.a[10] ^= 1; break; case 11: t.a[11] ^= 1; break;
        case 12: t.a[12] ^= 1; break; case 13: t.a[13] ^= 1; break; case 14: t.a[14] ^= 1; break; case 15: t.a[15] ^= 1; break;
        default: w16 ^= 1; break;
    }
    t.a[16] ^= w16;
    keccak_f1600(t.a);
    t.pos = 0;
    uint32_t d[8];
    _Pragma("unroll") for (int j = 0; j < 4; j++) { const uint64_t l = bswap64(t.a[3 - j]); d[2 * j] = (uint32_t)l; d[2 * j + 1] = (uint32_t)(l >> 32); }
    Fr r = Fr::reduce_once(d);
    for (int k = 0; k < 5; k++) r = Fr::reduce_once(r.v);                                       // 2^256 < 6 r for both curves
    return r.to_mont();
}

// ---- the key as the per-proof function reads it, and its outputs -------------------------------------------------------------------
constexpr int PLONK_N_COMMITS = 9, PLONK_N_EVALS = 6, PLONK_N_CHALLENGES = 6, PLONK_N_PROOF_SCALARS = 11, PLONK_N_KEY_SCALARS = 9;

template <class C>
struct PlonkVerifyKey {
    Affine<typename C::Fq> pts[8];            // Qm, Ql, Qr, Qo, Qc, S1, S2, S3
    typename C::Fr k1, k2, omega;             // omega: the 2^power-th root of unity
    uint32_t power, n_pub;
};

// commits: a, b, c, z, t1, t2, t3, wxi, wxiw; evals: a, b, c, s1, s2, zw; pubs: key.n_pub values; coeff128: 4 x u32 (canonical, little
// endian) or null.  Writes the challenges beta, gamma, alpha, xi, v, u; the 11 proof-point scalars (A-side first); the 9 key-point
// scalars; returns the valid flag: 0 iff xi hits one of the first max(1, n_pub) domain points, where the reference divides by zero.
// Every input field element must be fully reduced.
template <class C>
CG_HD int32_t plonk_verify_scalars(const PlonkVerifyKey<C>& key, const Affine<typename C::Fq>* commits, const typename C::Fr* evals, const typename C::Fr* pubs,
                                   const uint32_t* coeff128, typename C::Fr* out_ch, typename C::Fr* out_sp, typename C::Fr* out_sk) {
    typedef typename C::Fr Fr;
    const Fr ea = evals[0], eb = evals[1], ec = evals[2], es1 = evals[3], es2 = evals[4], ezw = evals[5];
    Fr beta, gamma, alpha, xi, v, u;
    {   // round 2: beta from the key, the public inputs and [a], [b], [c]; gamma from beta
        PlonkTranscript<Fr> t;
        for (int i = 0; i < 8; i++) t.add_point(key.pts[i]);
        for (uint32_t j = 0; j < key.n_pub; j++) t.add_scalar(pubs[j]);
        for (int i = 0; i < 3; i++) t.add_point(commits[i]);
        beta = plonk_transcript_finish(t);
    }
    { PlonkTranscript<Fr> t; t.add_scalar(beta); gamma = plonk_transcript_finish(t); }
    { PlonkTranscript<Fr> t; t.add_scalar(beta); t.add_scalar(gamma); t.add_point(commits[3]); alpha = plonk_transcript_finish(t); }
    { PlonkTranscript<Fr> t; t.add_scalar(alpha); for (int i = 4; i < 7; i++) t.add_point(commits[i]); xi = plonk_transcript_finish(t); }
    { PlonkTranscript<Fr> t; t.add_scalar(xi); for (int i = 0; i < 6; i++) t.add_scalar(evals[i]); v = plonk_transcript_finish(t); }
    { PlonkTranscript<Fr> t; t.add_point(commits[7]); t.add_point(commits[8]); u = plonk_transcript_finish(t); }
    out_ch[0] = beta; out_ch[1] = gamma; out_ch[2] = alpha; out_ch[3] = xi; out_ch[4] = v; out_ch[5] = u;

    // xi^n, z_h, and the Lagrange part with ONE inversion: sum_j pub_j w^j / d_j is kept as a fraction num / den (d_j = xi - w^j), and
    // 1 / (n d_0 den) gives both 1 / (n d_0) for L_0 and 1 / (n den) for the sum
    Fr xin = xi, nn = Fr::one();
    for (uint32_t i = 0; i < key.power; i++) { xin = xin.sqr(); nn = nn.dbl(); }
    const Fr zh = xin - Fr::one();
    const Fr d0 = xi - Fr::one();
    Fr num = Fr::zero(), den = Fr::one(), w = Fr::one();
    for (uint32_t j = 0; j < key.n_pub; j++) {
        const Fr d = xi - w;
        num = num * d + pubs[j] * w * den;
        den = den * d;
        w = w * key.omega;
    }
    const Fr all = nn * d0 * den;
    const int32_t valid = all.is_zero() ? 0 : 1;
    const Fr inv = fp_inverse(all);                                                             // inverse(0) = 0: no fault, the flag says reject
    const Fr l0 = zh * inv * den;
    const Fr pi = (zh * (num * inv * d0)).neg();

    const Fr e2 = alpha.sqr() * l0;
    const Fr e3a = ea + es1 * beta + gamma, e3b = eb + es2 * beta + gamma, e3c = ec + gamma;
    const Fr e3 = e3a * e3b * e3c * ezw * alpha;
    const Fr r0 = pi - e2 - e3;
    const Fr betaxi = beta * xi;
    const Fr d2a = (ea + betaxi + gamma) * (eb + betaxi * key.k1 + gamma) * (ec + betaxi * key.k2 + gamma) * alpha;
    const Fr v2 = v * v, v3 = v2 * v, v4 = v3 * v, v5 = v4 * v;
    const Fr e = v * ea + v2 * eb + v3 * ec + v4 * es1 + v5 * es2 + u * ezw - r0;
    const Fr nzh = zh.neg(), nzh_xin = nzh * xin;

    Fr r = Fr::one();
    if (coeff128) { r = Fr::zero(); for (int i = 0; i < 4; i++) r.v[i] = coeff128[i]; r = r.to_mont(); }
    out_sp[0] = r;                          out_sp[1] = r * u;
    out_sp[2] = r * v;                      out_sp[3] = r * v2;                 out_sp[4] = r * v3;
    out_sp[5] = r * (d2a + e2 + u);
    out_sp[6] = r * nzh;                    out_sp[7] = r * nzh_xin;            out_sp[8] = r * (nzh_xin * xin);
    out_sp[9] = r * xi;                     out_sp[10] = r * (u * xi * key.omega);
    out_sk[0] = r * (ea * eb);              out_sk[1] = r * ea;                 out_sk[2] = r * eb;                 out_sk[3] = r * ec;
    out_sk[4] = r;                          out_sk[5] = r * v4;                 out_sk[6] = r * v5;
    out_sk[7] = r * (e3a * e3b * alpha * beta * ezw).neg();
    out_sk[8] = r * e.neg();
    return valid;
}

}  // namespace cg
