// Target field and optimal-ate pairing for BN254 and BLS12-381, host and device from one source.
//
// Replaces what the reference's verifier gets from ark-ec 0.4.2 (`Bn::pairing`, `Bls12::pairing`, reached through ark-groth16's
// `verify_proof`, `co-circom/co-groth16/src/verifier.rs:23-43`).  The VALUE is the one arkworks 0.4 and snarkjs produce
// (e(alpha, beta) equals `vk_alphabeta_12` of a verification_key.json limb for limb):
//   BN254      f = f_{6x+2,Q}(P) * l_{[6x+2]Q, pi(Q)}(P) * l_{[6x+2]Q + pi(Q), -pi^2(Q)}(P),  e = f^(2x(6x^2+3x+1) (p^12-1)/r)
//   BLS12-381  f = conj(f_{|x|,Q}(P))  (x < 0),                                               e = f^(3 (p^12-1)/r)
// Fp12 = Fp2[w]/(w^6 - xi), coefficients c[i] of w^i; in memory (the ABI, and `vk_alphabeta_12`'s JSON nesting) an element is
// (2, 3, 2, limbs): [i][j] = c[2j + i], the tower Fp6[w]/(w^2 - v), Fp6 = Fp2[v]/(v^3 - xi) with v = w^2.
// The running point T stays on the twist E'(Fp2) in Jacobian coordinates: no field inversion inside the loop.  A line is kept up to a
// factor in Fp2, which the final exponentiation removes ((p^6 - 1) kills Fp6):
//   D-type (BN254):      a0 + a1 w + a3 w^3  = cy yP + cx xP w + c0 w^3
//   M-type (BLS12-381):  a0 + a3 w^3 + a1 w^5 = xi cy yP + c0 w^3 + cx xP w^5
// with (cy, cx, c0) = s (1, -lambda, lambda x_T - y_T) for the slope lambda on E' and the scale s the step's formulas leave.
// Q must lie in the prime-order subgroup (T never meets +-Q inside the loop then); other inputs give a meaningless value, never a fault.
// The Fp12 products are out of line and take pointers: an element is 96 (BN254) or 144 (BLS12-381) registers, it lives in scratch either way.
#pragma once
#include <cstring>
#include "curve.hpp"
#include "pairing_consts.hpp"

namespace cg {

struct Bn254Pairing {
    typedef Bn254Fq Fq; typedef Fp2<Bn254Fq> Fq2; typedef Bn254Fr Fr; typedef Bn254PairingK K;
    static constexpr bool TWIST_D = true, BN = true;
    CG_HD static Fq2 mul_xi(const Fq2& a) {   // (9 + u)(a0 + a1 u)
        Fq a8 = a.c0.dbl().dbl().dbl(), b8 = a.c1.dbl().dbl().dbl();
        return {a8 + a.c0 - a.c1, b8 + a.c1 + a.c0};
    }
};
struct Bls381Pairing {
    typedef Bls381Fq Fq; typedef Fp2<Bls381Fq> Fq2; typedef Bls381Fr Fr; typedef Bls381PairingK K;
    static constexpr bool TWIST_D = false, BN = false;
    CG_HD static Fq2 mul_xi(const Fq2& a) { return {a.c0 - a.c1, a.c0 + a.c1}; }   // (1 + u)(a0 + a1 u)
};

template <class F> CG_HD F fp_from_limbs(const uint32_t* w) { F r; for (int i = 0; i < F::N; i++) r.v[i] = w[i]; return r; }
template <class F> CG_HD Fp2<F> fp2_conjugate(const Fp2<F>& a) { return {a.c0, a.c1.neg()}; }
template <class F> CG_HD Fp2<F> fp2_mul_base(const Fp2<F>& a, const F& s) { return {a.c0 * s, a.c1 * s}; }

template <class C>
struct Fp12 {
    typedef typename C::Fq2 Fq2;
    Fq2 c[6];
    CG_HD static Fp12 one() { Fp12 r; for (int i = 0; i < 6; i++) r.c[i] = Fq2::zero(); r.c[0] = Fq2::one(); return r; }
    CG_HD bool operator==(const Fp12& o) const { bool e = true; for (int i = 0; i < 6; i++) e = e && c[i] == o.c[i]; return e; }
    // the ABI's layout: 12 base-field elements, [i][j][k] = c[2j + i].c_k
    CG_HD static Fp12 load(const void* p) { const Fq2* q = (const Fq2*)p; Fp12 r; for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) r.c[2 * j + i] = q[i * 3 + j]; return r; }
    CG_HD void store(void* p) const { Fq2* q = (Fq2*)p; for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) q[i * 3 + j] = c[2 * j + i]; }
    // The same for a caller's host buffer, which the ABI only asks to be 8-byte aligned (a u64 array): load and store above cast to Fq2,
    // alignas(16), and the host compiler turns that into aligned vector moves.  The kernels keep load / store: device buffers are 16-byte
    // aligned by allocation.
    static Fp12 load_host(const void* p) { Fq2 q[6]; memcpy(q, p, sizeof q); return load(q); }
    void store_host(void* p) const { Fq2 q[6]; store(q); memcpy(p, q, sizeof q); }
};
// workgroup size of the pairing kernels and the most workgroups (= partial products handed to the host) of the product reduction: shared by
// the launchers (pairing_impl.hpp) and the caller that sizes the partials' buffer (capi_pairing.hip)
constexpr int PAIRING_BLOCK = 64;
constexpr int PAIRING_PRODUCT_GROUPS_MAX = 256;

template <class C> struct Line { typename C::Fq2 a0, a1, a3; };

// r = a b: schoolbook over w, 36 Fp2 products (r must not alias a or b)
template <class C>
CG_HD_NOINLINE void fp12_mul(Fp12<C>* r, const Fp12<C>* a, const Fp12<C>* b) {
    typedef typename C::Fq2 Fq2;
    for (int k = 0; k < 6; k++) {
        Fq2 lo = Fq2::zero(), hi = Fq2::zero();
        for (int i = 0; i < 6; i++) {
            if (i <= k) lo = lo + a->c[i] * b->c[k - i];
            else hi = hi + a->c[i] * b->c[k + 6 - i];
        }
        r->c[k] = lo + C::mul_xi(hi);
    }
}
// r = a^2: 6 squarings + 15 products
template <class C>
CG_HD_NOINLINE void fp12_sqr(Fp12<C>* r, const Fp12<C>* a) {
    typedef typename C::Fq2 Fq2;
    for (int k = 0; k < 6; k++) {
        Fq2 lo = Fq2::zero(), hi = Fq2::zero();
        for (int i = 0; i < 6; i++) {
            const int j = i <= k ? k - i : k + 6 - i;
            if (i >= j) continue;
            const Fq2 t = a->c[i] * a->c[j];
            if (i <= k) lo = lo + t; else hi = hi + t;
        }
        lo = lo.dbl(); hi = hi.dbl();
        if (k % 2 == 0) { lo = lo + a->c[k / 2].sqr(); hi = hi + a->c[k / 2 + 3].sqr(); }   // i = j: 2i = k and 2i = k + 6
        r->c[k] = lo + C::mul_xi(hi);
    }
}
// r = a * line: 18 Fp2 products (r must not alias a)
template <class C>
CG_HD_NOINLINE void fp12_mul_line(Fp12<C>* r, const Fp12<C>* a, const Line<C>* l) {
    typedef typename C::Fq2 Fq2;
    const int s1 = C::TWIST_D ? 1 : 5;
    for (int k = 0; k < 6; k++) {
        Fq2 lo = l->a0 * a->c[k], hi = Fq2::zero();
        const Fq2 t3 = l->a3 * a->c[k >= 3 ? k - 3 : k + 3];
        if (k >= 3) lo = lo + t3; else hi = hi + t3;
        const Fq2 t1 = l->a1 * a->c[k >= s1 ? k - s1 : k + 6 - s1];
        if (k >= s1) lo = lo + t1; else hi = hi + t1;
        r->c[k] = lo + C::mul_xi(hi);
    }
}
template <class C> CG_HD Fp12<C> operator*(const Fp12<C>& a, const Fp12<C>& b) { Fp12<C> r; fp12_mul(&r, &a, &b); return r; }
// conjugation over Fp6 (the p^6-Frobenius): odd powers of w change sign
template <class C> CG_HD Fp12<C> fp12_conj(const Fp12<C>& a) { Fp12<C> r = a; for (int k = 1; k < 6; k += 2) r.c[k] = r.c[k].neg(); return r; }
// the p^2-Frobenius: Fp2 is fixed, w^i picks up gamma^i in Fp
template <class C> CG_HD Fp12<C> fp12_frob2(const Fp12<C>& a) {
    Fp12<C> r = a;
    for (int k = 1; k < 6; k++) r.c[k] = fp2_mul_base(a.c[k], fp_from_limbs<typename C::Fq>(C::K::FROB2[k - 1]));
    return r;
}

// Fp6 = Fp2[v]/(v^3 - xi), for the inverse only
template <class C> struct Fp6 { typename C::Fq2 a[3]; };
template <class C> CG_HD Fp6<C> fp6_mul(const Fp6<C>& x, const Fp6<C>& y) {
    Fp6<C> r;
    r.a[0] = x.a[0] * y.a[0] + C::mul_xi(x.a[1] * y.a[2] + x.a[2] * y.a[1]);
    r.a[1] = x.a[0] * y.a[1] + x.a[1] * y.a[0] + C::mul_xi(x.a[2] * y.a[2]);
    r.a[2] = x.a[0] * y.a[2] + x.a[1] * y.a[1] + x.a[2] * y.a[0];
    return r;
}
template <class C> CG_HD Fp6<C> fp6_inverse(const Fp6<C>& x) {
    typedef typename C::Fq2 Fq2;
    const Fq2 t0 = x.a[0].sqr() - C::mul_xi(x.a[1] * x.a[2]);
    const Fq2 t1 = C::mul_xi(x.a[2].sqr()) - x.a[0] * x.a[1];
    const Fq2 t2 = x.a[1].sqr() - x.a[0] * x.a[2];
    const Fq2 d = fp_inverse(x.a[0] * t0 + C::mul_xi(x.a[2] * t1 + x.a[1] * t2));
    return {{t0 * d, t1 * d, t2 * d}};
}
// (A + B w)^-1 = (A - B w) / (A^2 - v B^2); inverse(0) = 0
template <class C>
CG_HD_NOINLINE void fp12_inverse(Fp12<C>* r, const Fp12<C>* f) {
    Fp6<C> A{{f->c[0], f->c[2], f->c[4]}}, B{{f->c[1], f->c[3], f->c[5]}};
    const Fp6<C> a2 = fp6_mul(A, A), b2 = fp6_mul(B, B);
    Fp6<C> n{{a2.a[0] - C::mul_xi(b2.a[2]), a2.a[1] - b2.a[0], a2.a[2] - b2.a[1]}};
    n = fp6_inverse(n);
    A = fp6_mul(A, n); B = fp6_mul(B, n);
    for (int j = 0; j < 3; j++) { r->c[2 * j] = A.a[j]; r->c[2 * j + 1] = B.a[j].neg(); }
}

// f^((p^6 - 1)(p^2 + 1)) and then the hard exponent (with the convention's factor) by square-and-multiply
template <class C>
CG_HD_NOINLINE void final_exponentiation(Fp12<C>* out, const Fp12<C>* f) {
    Fp12<C> t, u;
    fp12_inverse(&t, f);
    u = fp12_conj(*f);
    Fp12<C> e; fp12_mul(&e, &u, &t);                 // f^(p^6 - 1)
    t = fp12_frob2(e);
    fp12_mul(&u, &t, &e);                            // ^(p^2 + 1): u
    t = u;                                           // the exponent's leading one
    for (int b = C::K::HARD_BITS - 2; b >= 0; b--) {
        fp12_sqr(&e, &t);
        if ((C::K::HARD[b >> 5] >> (b & 31)) & 1u) fp12_mul(&t, &e, &u); else t = e;
    }
    *out = t;
}

// f *= l_{T,T}(P); T = 2T   (dbl-2009-l, a = 0)
template <class C>
CG_HD_NOINLINE void miller_double(Jacobian<typename C::Fq2>* T, const Affine<typename C::Fq>* P, Line<C>* l) {
    typedef typename C::Fq2 Fq2;
    const Fq2 A = T->x.sqr(), B = T->y.sqr(), Cc = B.sqr(), zz = T->z.sqr();
    const Fq2 D = ((T->x + B).sqr() - A - Cc).dbl();
    const Fq2 E = A.dbl() + A;
    const Fq2 X3 = E.sqr() - D.dbl();
    const Fq2 Z3 = (T->y * T->z).dbl();
    const Fq2 c0 = E * T->x - B.dbl();
    T->y = E * (D - X3) - Cc.dbl().dbl().dbl(); T->x = X3; T->z = Z3;
    const Fq2 cy = fp2_mul_base(Z3 * zz, P->y);
    l->a0 = C::TWIST_D ? cy : C::mul_xi(cy);
    l->a1 = fp2_mul_base(E * zz, P->x).neg();
    l->a3 = c0;
}
// f *= l_{T,R}(P); T = T + R for an affine R on the twist
template <class C>
CG_HD_NOINLINE void miller_add(Jacobian<typename C::Fq2>* T, const Affine<typename C::Fq2>* R, const Affine<typename C::Fq>* P, Line<C>* l) {
    typedef typename C::Fq2 Fq2;
    const Fq2 zz = T->z.sqr();
    const Fq2 H = R->x * zz - T->x, rr = R->y * (T->z * zz) - T->y;
    const Fq2 HH = H.sqr(), HHH = H * HH, V = T->x * HH;
    const Fq2 X3 = rr.sqr() - HHH - V.dbl();
    const Fq2 Z3 = T->z * H;
    T->y = rr * (V - X3) - T->y * HHH; T->x = X3; T->z = Z3;
    const Fq2 cy = fp2_mul_base(Z3, P->y);
    l->a0 = C::TWIST_D ? cy : C::mul_xi(cy);
    l->a1 = fp2_mul_base(rr, P->x).neg();
    l->a3 = rr * R->x - Z3 * R->y;
}

// the Miller value of the convention (conjugated for BLS12-381's negative x); an input at infinity in either group gives 1
template <class C>
CG_HD_NOINLINE void miller_loop(Fp12<C>* out, const Affine<typename C::Fq>* P, const Affine<typename C::Fq2>* Q) {
    typedef typename C::Fq2 Fq2;
    Fp12<C> f = Fp12<C>::one(), g;
    if (P->is_inf() || Q->is_inf()) { *out = f; return; }
    Jacobian<Fq2> T{Q->x, Q->y, Fq2::one()};
    Line<C> l;
    for (int b = C::K::LOOP_BITS - 2; b >= 0; b--) {
        fp12_sqr(&g, &f);
        miller_double(&T, P, &l); fp12_mul_line(&f, &g, &l);
        if ((C::K::LOOP[b >> 5] >> (b & 31)) & 1u) { miller_add(&T, Q, P, &l); g = f; fp12_mul_line(&f, &g, &l); }
    }
    if constexpr (C::BN) {
        typedef typename C::Fq Fq;
        const Fq2 gx{fp_from_limbs<Fq>(C::K::TWIST_X), fp_from_limbs<Fq>(C::K::TWIST_X + Fq::N)}, gy{fp_from_limbs<Fq>(C::K::TWIST_Y), fp_from_limbs<Fq>(C::K::TWIST_Y + Fq::N)};
        Affine<Fq2> Q1{fp2_conjugate(Q->x) * gx, fp2_conjugate(Q->y) * gy};
        miller_add(&T, &Q1, P, &l); g = f; fp12_mul_line(&f, &g, &l);
        Affine<Fq2> Q2{fp2_conjugate(Q1.x) * gx, (fp2_conjugate(Q1.y) * gy).neg()};
        miller_add(&T, &Q2, P, &l); g = f; fp12_mul_line(&f, &g, &l);
        *out = f;
    } else {
        *out = fp12_conj(f);
    }
}

}  // namespace cg
