// Host model of the MSM's signed lazy-limb arithmetic: the __device__ functions of csrc/lazy29.hpp and csrc/msm_kernels.hpp compiled as plain
// C++ (hip_host_prelude.hpp, lazy_bucket.mk) under AddressSanitizer + UndefinedBehaviorSanitizer and driven over the inputs their no-overflow
// and range arguments are tightest on.  UBSan's signed-overflow check is the detector for the int64 column sums and the int32 limb sums (a
// report aborts the run); every value is compared with the CPU oracle (orc_field_op, orc_point_add, orc_points_mul, orc_generator_mul), never
// with field.hpp.  No GPU, nothing of the product library.
//   usage: lazy_bucket_main [edge point file]        (the file: tests/msm_edges.py::write_edge_file; without it check 4 skips those chains)
// Checks (one line each, with its case count):
//   1  every product form of L29 / L29x2 against the oracle's product, each operand class combined with each
//   2  unpack<SH>, unpack_small, one, one_small, to_fp, pack_reduced on the quotient / top-limb / power-of-two boundary values
//   3  maybe_zero_mod_p, is_zero_mod_p on k p, k p +- 1 and k p with one flipped bit
//   4  acc_madd_lazy chains on RegAcc29 (column engine: G1 of both curves, BN254 G2; row form: BLS12-381 G2) against the oracle after every
//      step, with the documented value class of every coordinate asserted after every step
//   5  bk_add, bk_add_inl, bk_dbl, bk_dbl_inl, bk_mul_small, bk_to_xyzz, bk_is_inf against the oracle
// Intervals are tested exactly in int64 limbs: sign(d x - n p) is the sign of the top limb after carry propagation.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "msm_kernels.hpp"

using namespace cg;

extern "C" {
const char* orc_last_error();
int orc_from_dec(int curve, int which, const char* dec, uint64_t* out);
int orc_field_op(int curve, int which, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int orc_field_inverse(int curve, int which, const uint64_t* a, uint64_t* out);
int orc_on_curve(int curve, int group, const uint64_t* pt);
int orc_generator_mul(int curve, int group, const uint64_t* scalar, uint64_t* out_affine);
int orc_points_mul(int curve, int group, const uint64_t* pts, const uint64_t* scalars, size_t n, uint64_t* out_affine);
int orc_point_add(int curve, int group, const uint64_t* a, const uint64_t* b, uint64_t* out_affine);
}

// The program is built from this file twice so that make can compile the two halves side by side (lazy_bucket.mk): LAZY_PART 1 instantiates the
// product forms of check 1 and nothing else, LAZY_PART 2 the rest and main; 0 (the default) is the whole program in one object.
#ifndef LAZY_PART
#define LAZY_PART 0
#endif
#if LAZY_PART == 1
extern long failures, cases;
#else
long failures = 0, cases = 0;
#endif
void report(const char* what);
void run_check1();
#define CHECK(cond, ...)                                                                                           \
    do {                                                                                                           \
        cases++;                                                                                                   \
        if (!(cond)) { if (failures < 40) { printf("FAIL (%s:%d) %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } failures++; } \
    } while (0)
static void must(int rc) { if (rc < 0) { printf("oracle: %s\n", orc_last_error()); exit(3); } }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }

// ---- the oracle's field operations on the product's element types (same bytes: little-endian Montgomery limbs) -----------------------------
template <class F> struct Fld;
template <> struct Fld<Bn254Fr> { static constexpr int curve = 0, which = 0; static constexpr const char* name = "bn254 Fr"; };
template <> struct Fld<Bn254Fq> { static constexpr int curve = 0, which = 1; static constexpr const char* name = "bn254 Fq"; };
template <> struct Fld<Bls381Fr> { static constexpr int curve = 1, which = 0; static constexpr const char* name = "bls12_381 Fr"; };
template <> struct Fld<Bls381Fq> { static constexpr int curve = 1, which = 1; static constexpr const char* name = "bls12_381 Fq"; };
template <class P> Fp<P> oop(int op, const Fp<P>& a, const Fp<P>& b) {
    typedef Fp<P> F;
    uint64_t x[6], y[6], z[6];
    memcpy(x, a.v, 4 * F::N); memcpy(y, b.v, 4 * F::N);
    must(orc_field_op(Fld<F>::curve, Fld<F>::which, op, x, y, z, 1));
    F r; memcpy(r.v, z, 4 * F::N); return r;
}
template <class P> Fp<P> oadd(const Fp<P>& a, const Fp<P>& b) { return oop(0, a, b); }
template <class P> Fp<P> osub(const Fp<P>& a, const Fp<P>& b) { return oop(1, a, b); }
template <class P> Fp<P> omul(const Fp<P>& a, const Fp<P>& b) { return oop(2, a, b); }
template <class B> Fp2<B> oadd(const Fp2<B>& a, const Fp2<B>& b) { return {oadd(a.c0, b.c0), oadd(a.c1, b.c1)}; }
template <class B> Fp2<B> osub(const Fp2<B>& a, const Fp2<B>& b) { return {osub(a.c0, b.c0), osub(a.c1, b.c1)}; }
template <class B> Fp2<B> omul(const Fp2<B>& a, const Fp2<B>& b) { return {osub(omul(a.c0, b.c0), omul(a.c1, b.c1)), oadd(omul(a.c0, b.c1), omul(a.c1, b.c0))}; }
template <class F> F oneg(const F& a) { return osub(F::zero(), a); }
template <class P> Fp<P> raw_small(uint32_t v) { Fp<P> r = Fp<P>::zero(); r.v[0] = v; return r; }

// ---- plain integers of up to 13 words (only for the boundary values of check 2) -----------------------------------------------------------
typedef std::array<uint32_t, 14> Wd;
template <class F> Wd wd_p() { Wd r{}; for (int i = 0; i < F::N; i++) r[i] = F::Params::P[i]; return r; }
static Wd wd_mul(const Wd& a, uint32_t m) { Wd r{}; uint64_t c = 0; for (size_t i = 0; i < a.size(); i++) { c += (uint64_t)a[i] * m; r[i] = (uint32_t)c; c >>= 32; } return r; }
static Wd wd_shr(const Wd& a, int s) { Wd r{}; for (size_t i = 0; i < a.size(); i++) { const size_t w = i + s / 32; uint64_t two = w < a.size() ? a[w] : 0; if (w + 1 < a.size()) two |= (uint64_t)a[w + 1] << 32; r[i] = (uint32_t)(two >> (s % 32)); } return r; }
static Wd wd_shl(const Wd& a, int s) { Wd r{}; for (size_t i = a.size(); i-- > 0;) { const long w = (long)i - s / 32; uint64_t two = w >= 0 ? (uint64_t)a[w] << 32 : 0; if (w >= 1) two |= a[w - 1]; r[i] = (uint32_t)(two >> (32 - s % 32)); } return r; }
static bool wd_add(Wd& a, int64_t d) {   // a += d; false if the result is negative
    int64_t c = d;
    for (size_t i = 0; i < a.size(); i++) { const int64_t t = (int64_t)a[i] + (c & 0xffffffffll); a[i] = (uint32_t)t; c = (c >> 32) + (t >> 32); if (c == 0) return true; }
    return c >= 0;
}
static bool wd_lt(const Wd& a, const Wd& b) { for (size_t i = a.size(); i-- > 0;) if (a[i] != b[i]) return a[i] < b[i]; return false; }
template <class F> F wd_elem(const Wd& a) { F r; for (int i = 0; i < F::N; i++) r.v[i] = a[i]; return r; }
template <class F> Wd elem_wd(const F& a) { Wd r{}; for (int i = 0; i < F::N; i++) r[i] = a.v[i]; return r; }

// The raw values a < p check 2 runs on: small, next to p, next to every quotient boundary floor(j p / 2^SH), next to the steps of the top limb
// of 2^SH a beside each of them, and around every power of two.
template <class F> std::vector<F> boundary_values() {
    typedef L29<F> L;
    const Wd p = wd_p<F>();
    std::vector<F> out;
    auto push = [&](Wd v, int64_t d) { if (wd_add(v, d) && wd_lt(v, p)) out.push_back(wd_elem<F>(v)); };
    for (int d = 0; d <= 2; d++) { push(Wd{}, d); if (d) push(p, -d); }
    const int step_bit = L::TOPBIT - L::SH;                    // the top limb of 2^SH a is floor(a / 2^step_bit)
    for (uint32_t j = 1; j < (1u << L::SH); j++) {
        const Wd q = wd_shr(wd_mul(p, j), L::SH);
        for (int d = -2; d <= 2; d++) push(q, d);
        const Wd t = wd_shr(q, step_bit);
        for (int up = 0; up <= 1; up++) { Wd s = t; wd_add(s, up); s = wd_shl(s, step_bit); for (int d = -1; d <= 1; d++) push(s, d); }
    }
    for (int k = 0; k < 32 * F::N; k++) { Wd one{}; one[0] = 1; const Wd v = wd_shl(one, k); for (int d = -1; d <= 1; d++) push(v, d); }
    return out;
}

// ---- exact limb arithmetic on lazy values (test side) ----------------------------------------------------------------------------------------
template <class L> struct Lx {
    static constexpr int NL = L::NL, W = L::W;
    typedef typename std::remove_reference<decltype(L::to_fp(L()))>::type F;
    static L zero() { L r; for (int k = 0; k < NL; k++) r.l[k] = 0; return r; }
    // carry-normalised limbs of sum_k t[k] 2^(W k): limbs 0..NL-2 in [0, 2^W), the top one signed
    static std::array<int64_t, NL> carry(std::array<int64_t, NL> t) { int64_t c = 0; for (int k = 0; k < NL; k++) { t[k] += c; if (k < NL - 1) { c = t[k] >> W; t[k] &= (int64_t)L::MASK; } } return t; }
    static int sign(const std::array<int64_t, NL>& t) { if (t[NL - 1] != 0) return t[NL - 1] < 0 ? -1 : 1; for (int k = 0; k < NL - 1; k++) if (t[k]) return 1; return 0; }
    // sign of d x - n p (x any limbs, normalised or not)
    static int sgn(const L& x, int64_t d, int64_t n) { std::array<int64_t, NL> t; for (int k = 0; k < NL; k++) t[k] = d * x.l[k] - n * L::pl(k); return sign(carry(t)); }
    // lo p / 100 < x < hi p / 100
    static bool within(const L& x, int lo, int hi) { return sgn(x, 100, lo) > 0 && sgn(x, 100, hi) < 0; }
    static bool normalised(const L& x) { for (int k = 0; k < NL - 1; k++) if (x.l[k] < 0 || x.l[k] > (int32_t)L::MASK) return false; return true; }
    static L from64(const std::array<int64_t, NL>& t) { L r; for (int k = 0; k < NL; k++) r.l[k] = (int32_t)t[k]; return r; }
    static L kp(int k) { std::array<int64_t, NL> t; for (int j = 0; j < NL; j++) t[j] = (int64_t)k * L::pl(j); return from64(carry(t)); }
    // floor(n p / 100), normalised
    static L frac(int n) {
        std::array<int64_t, NL> t; for (int j = 0; j < NL; j++) t[j] = (int64_t)n * L::pl(j);
        t = carry(t);
        int64_t rem = 0;
        for (int j = NL - 1; j >= 0; j--) { const int64_t cur = rem * ((int64_t)1 << W) + t[j]; int64_t q = cur / 100; if (cur % 100 < 0) q--; rem = cur - q * 100; t[j] = q; }
        return from64(t);
    }
    static L add_small(const L& x, int d) { L r = x; r.l[0] += d; return r.norm(); }
    static L random_residue() {   // normalised, uniform enough in [0, p)
        for (;;) { L r; for (int k = 0; k < NL; k++) r.l[k] = (int32_t)(rnd() & L::MASK); r.l[NL - 1] %= (L::pl(NL - 1) + 1); if (sgn(r, 1, 1) < 0) return r; }
    }
    static bool same_limbs(const L& a, const L& b) { for (int k = 0; k < NL; k++) if (a.l[k] != b.l[k]) return false; return true; }
    // the N x 32-bit words of a normalised value in [0, 2^(32 N))
    static F words(const L& x) {
        F r = F::zero();
        for (int k = 0; k < NL; k++) for (int b = 0; b < (k < NL - 1 ? W : 31); b++) if ((x.l[k] >> b) & 1) { const int bit = W * k + b; if (bit < 32 * F::N) r.v[bit / 32] |= 1u << (bit % 32); }
        return r;
    }
    // 2^shift * a, bit by bit
    static L from_words(const F& a, int shift) {
        std::array<int64_t, NL> t{};
        for (int bit = 0; bit < 32 * F::N; bit++) if ((a.v[bit / 32] >> (bit % 32)) & 1) { const int at = bit + shift, k = at / W < NL ? at / W : NL - 1; t[k] += (int64_t)1 << (at - W * k); }
        return from64(t);
    }
    // R / 2^SH in the ABI's form: the element a lazy value x stands for is x * this (as a product of the oracle), see elem()
    static F unshift() {
        static const F c = [] {
            uint64_t a[6] = {0}, b[6];
            F two_sh = raw_small<typename F::Params>(1u << L::SH);
            memcpy(a, two_sh.v, 4 * F::N);
            must(orc_field_inverse(Fld<F>::curve, Fld<F>::which, a, b));       // bits R^2 / 2^SH
            F inv; memcpy(inv.v, b, 4 * F::N);
            return omul(inv, raw_small<typename F::Params>(1));                 // bits R / 2^SH
        }();
        return c;
    }
    // The ABI element a lazy value stands for — what to_fp must return — from the oracle alone: x = r + k p with r in [0, p) found by exact
    // sign tests, and bits(r) * (R / 2^SH) / R = r / 2^SH.  |x| < 24 p.
    static F elem(const L& x) {
        L r = x.norm();
        for (int k = -24; k <= 24; k++) {
            const L t = (x - kp(k)).norm();
            if (sgn(t, 1, 0) >= 0 && sgn(t, 1, 1) < 0) { r = t; return omul(words(r), unshift()); }
        }
        printf("elem: value outside (-24 p, 24 p)\n"); exit(3);
    }
};

// ---- check 1: product forms -------------------------------------------------------------------------------------------------------------------
// An operand: limbs, the element it stands for (oracle), a bound on |value| in p / 100, and whether its limbs stay within 2^W (unit) or 2^(W+1)
template <class L> struct Opd { L v; typename Lx<L>::F f; int mag; bool unit; const char* what; };

template <class F> std::vector<Opd<L29<F>>> operands() {
    typedef L29<F> L; typedef Lx<L> X;
    std::vector<Opd<L>> o;
    auto add = [&](const L& v, int mag, bool unit, const char* what) { o.push_back({v, X::elem(v), mag, unit, what}); };
    L lowones = X::zero(); for (int k = 0; k < L::NL - 1; k++) lowones.l[k] = (int32_t)L::MASK; lowones.l[L::NL - 1] = L::pl(L::NL - 1) - 1;
    L toponly = X::zero(); toponly.l[L::NL - 1] = 1;
    const L r1 = X::random_residue(), r2 = X::random_residue(), r3 = X::random_residue();
    // normalised residues
    add(X::zero(), 0, true, "0"); add(X::add_small(X::zero(), 1), 1, true, "1"); add(X::add_small(X::kp(1), -1), 100, true, "p-1");
    add(lowones, 100, true, "low limbs all ones"); add(r1, 100, true, "random"); add(r2, 100, true, "random");
    // the extreme representatives of every documented value class (Fq: products, X, Y, P, R; Fq2 components: products, X, Y, P, ZZ)
    static const int cls[][2] = {{-20, 120}, {-400, 200}, {-150, 150}, {-230, 530}, {-180, 280}, {-45, 145}, {-480, 280}, {-190, 190}, {-330, 630}};
    for (auto& c : cls) {
        add(X::add_small(X::frac(c[0]), 1), std::abs(c[0]), true, "low end of a class");
        add(X::add_small(X::frac(c[1]), -1), std::abs(c[1]), true, "high end of a class");
    }
    // unnormalised: the differences the formulas pass (|limb| < 2^W), limbs of exactly +-2^W, doublings (|limb| <= 2^(W+1))
    add(lowones - toponly, 200, true, "limbs +(2^W - 1)"); add(toponly - lowones, 200, true, "limbs -(2^W - 1)");
    add(r1 - r3, 100, true, "random - random"); add(r2 - X::add_small(X::frac(200), -1), 300, true, "P = product - X (X near 2p)");
    add(lowones - X::add_small(X::frac(-480), 1), 580, true, "P = product - X (X near -4.8p)");
    { L e = X::zero(); for (int k = 0; k < L::NL - 1; k++) e.l[k] = 1 << L::W; e.l[L::NL - 1] = L::pl(L::NL - 1) - 3; add(e, 100, true, "limbs +2^W");
      L m = e.neg(); add(m, 100, true, "limbs -2^W"); }
    add(lowones.dbl(), 200, false, "2 * normalised"); add((lowones - toponly).dbl(), 400, false, "2 * difference"); add((toponly - lowones).dbl(), 400, false, "2 * difference, negative");
    return o;
}
// 2^(NL W) / p, rounded down: the product contract mul(a, b) in (a b / 2^(NL W), a b / 2^(NL W) + p) then bounds a result by the operands' magnitudes
template <class F> double mont_ratio() {
    const double top = (double)(((uint64_t)F::Params::P[F::N - 1] << 32) | F::Params::P[F::N - 2]) + 1.0;
    return std::ldexp(1.0, L29<F>::NL * L29<F>::W - 32 * F::N + 64) / top;
}
template <class L> static void check_product(const char* form, const L& got, const typename Lx<L>::F& want, double magsum /* sum |a||b| in p^2 / 10^4 */, const char* wa, const char* wb) {
    typedef Lx<L> X;
    const int e = (int)std::ceil(magsum / 100.0 / mont_ratio<typename X::F>()) + 1;     // hundredths of p
    CHECK(X::normalised(got), "%s %s: %s x %s not normalised", Fld<typename X::F>::name, form, wa, wb);
    CHECK(X::within(got, -e, 100 + e), "%s %s: %s x %s outside (a b / 2^(NL W), a b / 2^(NL W) + p)", Fld<typename X::F>::name, form, wa, wb);
    CHECK(L::to_fp(got) == want, "%s %s: %s x %s differs from the oracle's product", Fld<typename X::F>::name, form, wa, wb);
}
template <class F> void check1_l29() {
    typedef L29<F> L;
    const auto o = operands<F>();
    const size_t n = o.size();
    for (size_t i = 0; i < n; i++) {
        const auto& a = o[i];
        CHECK(L::to_fp(a.v) == a.f, "%s to_fp(%s)", Fld<F>::name, a.what);
        if (a.unit) {
            const F want = omul(a.f, a.f); const double m = (double)a.mag * a.mag;
            check_product<L>("sqr", L::sqr(a.v), want, m, a.what, a.what);
            typename L::ColSqr s(a.v); L::run_cols(s); check_product<L>("ColSqr", s.r, want, m, a.what, a.what);
        }
        for (size_t j = 0; j < n; j++) {
            const auto& b = o[j];
            if (!a.unit && !b.unit) continue;                 // a doubled operand only ever meets a unit one (L29x2::sqr, Col2Sqr)
            const F want = omul(a.f, b.f); const double m = (double)a.mag * b.mag;
            check_product<L>("mul", L::mul(a.v, b.v), want, m, a.what, b.what);
            check_product<L>("mul_cols", L::mul_cols(a.v, b.v), want, m, a.what, b.what);
            { typename L::ColMul c(a.v, b.v); L::run_cols(c); check_product<L>("ColMul", c.r, want, m, a.what, b.what); }
            if (!a.unit || !b.unit) continue;
            // the four-operand forms: (a, b) with a second pair picked from the same list, and with itself (all four operands extreme at once)
            const Opd<L> minus_a = {a.v.neg(), oneg(a.f), a.mag, true, "-a"};
            for (int second = 0; second < 3; second++) {               // (c, d) = another pair of the list, (a, b) itself, (-a, b)
                const auto& c = second == 0 ? o[(i * 7 + 3) % n] : second == 1 ? a : minus_a; const auto& d = second ? b : o[(j * 5 + 1) % n];
                if (!c.unit || !d.unit) continue;
                const F cd = omul(c.f, d.f); const double m2 = m + (double)c.mag * d.mag, mcd = (double)c.mag * d.mag;
                check_product<L>("mul_sub", L::mul_sub(a.v, b.v, c.v, d.v), osub(want, cd), m2, a.what, b.what);
                L ab, cdl; L::mul2_cols(a.v, b.v, c.v, d.v, ab, cdl);
                check_product<L>("mul2_cols[0]", ab, want, m, a.what, b.what); check_product<L>("mul2_cols[1]", cdl, cd, mcd, c.what, d.what);
                { typename L::ColMulSub s(a.v, b.v, c.v, d.v); typename L::ColMulAdd t(a.v, b.v, c.v, d.v); L::run_cols(s, t);       // two chains
                  check_product<L>("ColMulSub (2 chains)", s.r, osub(want, cd), m2, a.what, b.what); check_product<L>("ColMulAdd (2 chains)", t.r, oadd(want, cd), m2, a.what, b.what); }
                { typename L::ColMulAdd t(a.v, b.v, c.v, d.v); L::run_cols(t); check_product<L>("ColMulAdd (1 chain)", t.r, oadd(want, cd), m2, a.what, b.what); }
                { typename L::ColMul u(a.v, b.v); typename L::ColMulSub s(a.v, b.v, c.v, d.v); typename L::ColSqr q(c.v); L::run_cols(u, s, q);   // three chains
                  check_product<L>("ColMul (3 chains)", u.r, want, m, a.what, b.what); check_product<L>("ColMulSub (3 chains)", s.r, osub(want, cd), m2, a.what, b.what);
                  check_product<L>("ColSqr (3 chains)", q.r, omul(c.f, c.f), (double)c.mag * c.mag, c.what, c.what); }
                { typename L::ColMul u(a.v, b.v), v(c.v, d.v), w(a.v, d.v); L::run_cols(u, v, w);
                  check_product<L>("ColMul (3 chains)[0]", u.r, want, m, a.what, b.what); check_product<L>("ColMul (3 chains)[1]", v.r, cd, mcd, c.what, d.what);
                  check_product<L>("ColMul (3 chains)[2]", w.r, omul(a.f, d.f), (double)a.mag * d.mag, a.what, d.what); }
                typedef L29x2<Fp2<F>> L2;
                check_product<L>("mul2<-1>", L2::template mul2<-1>(a.v, b.v, c.v, d.v), osub(want, cd), m2, a.what, b.what);
                check_product<L>("mul2<+1>", L2::template mul2<+1>(a.v, b.v, c.v, d.v), oadd(want, cd), m2, a.what, b.what);
            }
        }
    }
}
template <class F> void check1_l29x2() {
    typedef Fp2<F> F2; typedef L29x2<F2> L2; typedef L29<F> L; typedef Lx<L> X;
    std::vector<Opd<L>> o;
    for (const auto& x : operands<F>()) if (x.unit) o.push_back(x);
    const size_t n = o.size();
    const char* name = Fld<F>::name;
    auto check2 = [&](const char* form, const L2& got, const F2& want, double m, const char* wa, const char* wb) {
        const int e = (int)std::ceil(m / 100.0 / mont_ratio<F>()) + 1;
        CHECK(X::normalised(got.c0) && X::normalised(got.c1), "%s^2 %s: %s x %s not normalised", name, form, wa, wb);
        CHECK(X::within(got.c0, -e, 100 + e) && X::within(got.c1, -e, 100 + e), "%s^2 %s: %s x %s out of range", name, form, wa, wb);
        CHECK(L2::to_fp(got) == want, "%s^2 %s: %s x %s differs from the oracle's product", name, form, wa, wb);
    };
    for (size_t i = 0; i < n; i++) {
        const size_t i1 = (i * 11 + 5) % n;                       // the second component: another entry of the list, and the same one
        for (int same = 0; same < 2; same++) {
            const L2 a = {o[i].v, o[same ? i : i1].v}; const F2 af = {o[i].f, o[same ? i : i1].f};
            const double ma = (double)o[i].mag + o[same ? i : i1].mag;      // |a0| + |a1| bounds both components' cross terms
            { const F2 want = omul(af, af); check2("sqr", L2::sqr(a), want, ma * ma, o[i].what, o[i].what);
              typename L2::Col2Sqr c(a); L::run_cols(c.c0, c.c1); check2("Col2Sqr", c.res(), want, ma * ma, o[i].what, o[i].what); }
            for (size_t j = 0; j < n; j++) {
                const size_t j1 = (j * 13 + 2) % n;
                const L2 b = {o[j].v, o[same ? j : j1].v}; const F2 bf = {o[j].f, o[same ? j : j1].f};
                const double mb = (double)o[j].mag + o[same ? j : j1].mag;
                const F2 want = omul(af, bf);
                check2("mul", L2::mul(a, b), want, ma * mb, o[i].what, o[j].what);
                { typename L2::Col2Mul c(a, b); L::run_cols(c.c0, c.c1); check2("Col2Mul", c.res(), want, ma * mb, o[i].what, o[j].what); }
                const L2 c = {o[j1].v, o[i1].v}, d = {o[i1].v, o[j].v}; const F2 cf = {o[j1].f, o[i1].f}, df = {o[i1].f, o[j].f};
                const double mc = (double)o[j1].mag + o[i1].mag, md = (double)o[i1].mag + o[j].mag;
                const L2 ms = L2::mul_sub(a, b, c, d);              // a difference of two products, normalised: (-1 - e, 1 + e)
                const int e = (int)std::ceil((ma * mb + mc * md) / 100.0 / mont_ratio<F>()) + 1;
                CHECK(X::normalised(ms.c0) && X::normalised(ms.c1) && X::within(ms.c0, -100 - e, 100 + e) && X::within(ms.c1, -100 - e, 100 + e), "%s^2 mul_sub range: %s x %s", name, o[i].what, o[j].what);
                CHECK(L2::to_fp(ms) == osub(want, omul(cf, df)), "%s^2 mul_sub: %s x %s differs from the oracle", name, o[i].what, o[j].what);
            }
        }
    }
}

// ---- check 2: packing and unpacking on boundary values ---------------------------------------------------------------------------------------
template <class F> void check2() {
    typedef L29<F> L; typedef Lx<L> X;
    const char* name = Fld<F>::name;
    const auto vals = boundary_values<F>();
    const Wd p = wd_p<F>();
    for (const F& a : vals) {
        const L up = L::template unpack<L::SH>(a), u0 = L::template unpack<0>(a);
        CHECK(X::same_limbs(up, X::from_words(a, L::SH).norm()) && X::normalised(up), "%s unpack<SH> is not 2^SH a", name);
        CHECK(X::same_limbs(u0, X::from_words(a, 0).norm()) && X::normalised(u0), "%s unpack<0> is not a", name);
        const L s = L::unpack_small(a);
        CHECK(X::normalised(s), "%s unpack_small not normalised", name);
        CHECK(X::sgn(s, 1, -1) >= 0 && X::sgn(s, 1, 1) < 0, "%s unpack_small outside [-p, p) (top limb %d)", name, s.l[L::NL - 1]);
        bool multiple = false;                                   // 2^SH a - unpack_small(a) = k p, 1 <= k <= 2^SH + 1
        const L diff = (up - s).norm();
        for (int k = 0; k <= (1 << L::SH) + 1 && !multiple; k++) multiple = X::same_limbs(diff, X::kp(k));
        CHECK(multiple, "%s unpack_small is not 2^SH a minus a multiple of p", name);
        CHECK(L::to_fp(s) == a, "%s to_fp(unpack_small(a)) != a", name);
        CHECK(L::to_fp((s + X::kp(6)).norm()) == a && L::to_fp((s - X::kp(6)).norm()) == a, "%s to_fp at the ends of (-8p, 8p)", name);
        // pack_reduced takes a normalised value in (-p, 2p): the same residue in each of the three windows it has to fold
        const Wd aw = elem_wd(a);
        const L v = X::from_words(a, 0).norm();                  // a itself, in [0, p)
        CHECK(L::pack_reduced(v) == a, "%s pack_reduced(a)", name);
        CHECK(L::pack_reduced((v + X::kp(1)).norm()) == a, "%s pack_reduced(a + p)", name);
        if (wd_lt(Wd{}, aw)) CHECK(L::pack_reduced((v - X::kp(1)).norm()) == a, "%s pack_reduced(a - p)", name);
    }
    // just inside (-p, 2p) at both ends: -p + e -> e, 2p - e -> p - e
    for (int e = 1; e <= 3; e++) {
        Wd lo{}; wd_add(lo, e); Wd hi = p; wd_add(hi, -e);
        CHECK(L::pack_reduced(X::add_small(X::kp(-1), e)) == wd_elem<F>(lo), "%s pack_reduced(-p + %d)", name, e);
        CHECK(L::pack_reduced(X::add_small(X::kp(2), -e)) == wd_elem<F>(hi), "%s pack_reduced(2p - %d)", name, e);
    }
    const L one = L::one(), small = L::one_small();
    CHECK(X::normalised(one) && X::normalised(small) && X::sgn(small, 1, 0) >= 0 && X::sgn(small, 1, 1) < 0, "%s one_small outside [0, p)", name);
    CHECK(F::N == 8 ? X::within(one, 50, 170) : X::within(one, 1850, 1960), "%s one() outside its documented range", name);
    CHECK(L::to_fp(one) == L::to_fp(small) && X::elem(one) == X::elem(small), "%s one() and one_small() differ", name);
    F r; for (int i = 0; i < F::N; i++) r.v[i] = (uint32_t)rnd(); r.v[F::N - 1] &= 0x0fffffffu;
    CHECK(omul(X::elem(small), r) == r, "%s one_small() is not the oracle's one", name);
}

// ---- check 3: the equal-x tests -----------------------------------------------------------------------------------------------------------------
template <class F> void check3() {
    typedef L29<F> L; typedef Lx<L> X;
    const char* name = Fld<F>::name;
    uint32_t pinv = 1; for (int i = 0; i < 6; i++) pinv *= 2u - (uint32_t)L::pl(0) * pinv;       // 1 / p mod 2^32 (Newton)
    const uint32_t pinv_w = pinv & L::MASK;
    const bool small_inverse = pinv_w <= 9 || pinv_w >= L::MASK + 1 - 9;
    CHECK(small_inverse == (Fld<F>::curve == 1 && Fld<F>::which == 0), "%s: 1 / p mod 2^W = %u: the exemption below is meant for BLS12-381 Fr alone", name, pinv_w);
    for (int k = -3; k <= 6; k++) {
        const L kp = X::kp(k);
        CHECK(L::is_zero_mod_p(kp), "%s is_zero_mod_p(%d p)", name, k);
        CHECK(L::maybe_zero_mod_p(kp), "%s maybe_zero_mod_p(%d p)", name, k);
        for (int t = 0; t < 64; t++) {                           // the same value with carries left where differences leave them
            L u = kp;
            for (int j = 0; j < L::NL - 1; j++) { const int c = (int)(rnd() % 5) - 2; u.l[j] -= c * (1 << L::W); u.l[j + 1] += c; }
            CHECK(X::same_limbs(u.norm(), kp), "%s split of %d p", name, k);
            CHECK(L::maybe_zero_mod_p(u), "%s maybe_zero_mod_p(unnormalised %d p)", name, k);
            CHECK(L::is_zero_mod_p(u.norm()), "%s is_zero_mod_p(norm(unnormalised %d p))", name, k);
        }
        { const L a = X::random_residue(), b = (a - kp).norm(); CHECK(L::maybe_zero_mod_p(a - b) && L::is_zero_mod_p((a - b).norm()), "%s a - (a - %d p)", name, k); }
        for (int d = -1; d <= 1; d += 2) {
            const L off = X::add_small(kp, d);
            CHECK(!L::is_zero_mod_p(off), "%s is_zero_mod_p(%d p %+d)", name, k, d);
            // the cheap filter sees k' = x / p (mod 2^W) = k +- 1 / p: it must say no unless 1 / p (mod 2^W) is itself within +-9 (BLS12-381 Fr: p = 1 mod 2^32),
            // and the full test `maybe && is_zero(norm)` of the formulas says no either way
            CHECK(!L::maybe_zero_mod_p(off) || small_inverse, "%s maybe_zero_mod_p(%d p %+d)", name, k, d);
            CHECK(!(L::maybe_zero_mod_p(off) && L::is_zero_mod_p(off.norm())), "%s equal-x test on %d p %+d", name, k, d);
        }
        for (int j = 1; j < L::NL; j++) for (int b = 0; b < (j < L::NL - 1 ? L::W : 30); b++) {
            L f = kp; f.l[j] ^= 1 << b;
            CHECK(!L::is_zero_mod_p(f), "%s is_zero_mod_p(%d p with bit %d of limb %d flipped)", name, k, b, j);
        }
    }
}

// ---- points -------------------------------------------------------------------------------------------------------------------------------------
template <class F> struct Grp;
template <> struct Grp<Bn254Fq> { static constexpr int curve = 0, group = 0; static constexpr const char* name = "bn254 G1"; typedef Bn254Fq Base; };
template <> struct Grp<Fp2<Bn254Fq>> { static constexpr int curve = 0, group = 1; static constexpr const char* name = "bn254 G2"; typedef Bn254Fq Base; };
template <> struct Grp<Bls381Fq> { static constexpr int curve = 1, group = 0; static constexpr const char* name = "bls12_381 G1"; typedef Bls381Fq Base; };
template <> struct Grp<Fp2<Bls381Fq>> { static constexpr int curve = 1, group = 1; static constexpr const char* name = "bls12_381 G2"; typedef Bls381Fq Base; };
template <class F> constexpr int pt_words() { return (int)(sizeof(Affine<F>) / 8); }
template <class F> Affine<F> pt_from(const uint64_t* w) { Affine<F> r; memcpy(&r, w, sizeof(r)); return r; }
template <class F> Affine<F> opt_add(const Affine<F>& a, const Affine<F>& b) {
    uint64_t x[24], y[24], z[24]; memcpy(x, &a, sizeof(a)); memcpy(y, &b, sizeof(b));
    must(orc_point_add(Grp<F>::curve, Grp<F>::group, x, y, z));
    return pt_from<F>(z);
}
template <class F> Affine<F> opt_mul(const Affine<F>& a, uint32_t k) {
    uint64_t x[24], z[24], s[4]; memcpy(x, &a, sizeof(a));
    must(orc_from_dec(Grp<F>::curve, 0, std::to_string(k).c_str(), s));
    must(orc_points_mul(Grp<F>::curve, Grp<F>::group, x, s, 1, z));
    return pt_from<F>(z);
}
template <class F> Affine<F> opt_neg(const Affine<F>& a) { return a.is_inf() ? a : Affine<F>{a.x, oneg(a.y)}; }
template <class F> Affine<F> random_point() {
    uint64_t s[4] = {rnd(), rnd(), rnd(), rnd() >> 8}, z[24];
    must(orc_generator_mul(Grp<F>::curve, Grp<F>::group, s, z));
    return pt_from<F>(z);
}
template <class F> bool same_affine(const Affine<F>& a, const Affine<F>& b) { return a.x == b.x && a.y == b.y; }

// value classes of the accumulator / bucket coordinates in p / 100: X, Y, ZZ (= ZZZ)
template <class F> struct AccClass { static constexpr int x[2] = {-400, 200}, y[2] = {-150, 150}, z[2] = {-20, 120}; };       // lazy29.hpp
template <class B> struct AccClass<Fp2<B>> { static constexpr int x[2] = {-480, 280}, y[2] = {-190, 190}, z[2] = {-45, 145}; };   // msm_kernels.hpp, per component
struct BkClass { static constexpr int x[2] = {-480, 280}, y[2] = {-190, 190}, z[2] = {-45, 145}; };                              // msm_kernels.hpp, bk_add / bk_dbl
template <class F> bool lz_within(const L29<F>& v, const int (&c)[2]) { return Lx<L29<F>>::normalised(v) && Lx<L29<F>>::within(v, c[0], c[1]); }
template <class F2> bool lz_within(const L29x2<F2>& v, const int (&c)[2]) { return lz_within(v.c0, c) && lz_within(v.c1, c); }
template <class F> L29<F> lz_shift(const L29<F>& v, int k0, int) { return (v + Lx<L29<F>>::kp(k0)).norm(); }
template <class F2> L29x2<F2> lz_shift(const L29x2<F2>& v, int k0, int k1) { return {lz_shift(v.c0, k0, 0), lz_shift(v.c1, k1, 0)}; }

// lazy projective coordinates against an affine point of the oracle, by cross-multiplication: X = x ZZ, Y = y ZZZ, ZZ^3 = ZZZ^2, ZZ != 0
template <class F> bool same_point(const XYZZL<F>& got, const Affine<F>& want) {
    if (bk_is_inf(got)) return want.is_inf();
    if (want.is_inf()) return false;
    const XYZZ<F> c = bk_to_xyzz<F>(got);
    return !c.zz.is_zero() && omul(want.x, c.zz) == c.x && omul(want.y, c.zzz) == c.y && omul(omul(c.zz, c.zz), c.zz) == omul(c.zzz, c.zzz);
}
template <class F, class C> bool in_class(const XYZZL<F>& b) {
    return bk_is_inf(b) || (lz_within(b.c[0], C::x) && lz_within(b.c[1], C::y) && lz_within(b.c[2], C::z) && lz_within(b.c[3], C::z));
}

// ---- check 4: accumulator chains ----------------------------------------------------------------------------------------------------------------
template <class F> struct Chain {
    RegAcc29<F> acc; Affine<F> ref = Affine<F>::infinity(); const char* what; long steps = 0, doublings = 0, cancels = 0;
    explicit Chain(const char* w) : what(w) { acc.inf = true; }
    XYZZL<F> bucket() const { XYZZL<F> b = bk_inf<XYZZL<F>>(); if (!acc.inf) for (int f = 0; f < 4; f++) b.c[f] = acc.c[f]; return b; }
    void step(const Affine<F>& pt, bool negate) {
        const Affine<F> eff = negate ? opt_neg(pt) : pt;
        if (!acc.inf && same_affine(eff, ref)) doublings++;
        if (!acc.inf && same_affine(opt_neg(eff), ref)) cancels++;
        acc_madd_lazy<F>(acc, pt.x, pt.y, negate);
        ref = opt_add(ref, eff);
        steps++;
        const XYZZL<F> b = bucket();
        CHECK(acc.inf == ref.is_inf() && same_point(b, ref), "%s, %s: step %ld differs from the oracle", Grp<F>::name, what, steps);
        CHECK((in_class<F, AccClass<F>>(b)), "%s, %s: step %ld leaves a coordinate outside its documented class", Grp<F>::name, what, steps);
    }
    // the same step without the oracle's affine addition (an inversion): only the value classes are asserted; expect() settles the value later
    void quiet_step(const Affine<F>& pt, bool negate) {
        acc_madd_lazy<F>(acc, pt.x, pt.y, negate);
        steps++;
        CHECK((in_class<F, AccClass<F>>(bucket())), "%s, %s: step %ld leaves a coordinate outside its documented class", Grp<F>::name, what, steps);
    }
    void expect(const Affine<F>& want) {
        ref = want;
        CHECK(acc.inf == ref.is_inf() && same_point(bucket(), ref), "%s, %s: step %ld differs from the oracle", Grp<F>::name, what, steps);
    }
    // move every coordinate to another representative of its class where one exists (the hypotheses of the next step's no-overflow argument)
    void push_extreme() {
        if (acc.inf) return;
        const int (*cls[4])[2] = {&AccClass<F>::x, &AccClass<F>::y, &AccClass<F>::z, &AccClass<F>::z};
        for (int f = 0; f < 4; f++) for (int tries = 0; tries < 8; tries++) {
            const auto cand = lz_shift(acc.c[f], (int)(rnd() % 9) - 4, (int)(rnd() % 9) - 4);
            if (lz_within(cand, *cls[f])) { acc.c[f] = cand; break; }
        }
    }
};
template <class F> std::vector<XYZZL<F>> g_buckets;          // outputs of the chains, handed to check 5 with their oracle values
template <class F> std::vector<Affine<F>> g_bucket_refs;
template <class F> void keep(const Chain<F>& c) { g_buckets<F>.push_back(c.bucket()); g_bucket_refs<F>.push_back(c.ref); }

template <class F> void check4(const std::vector<Affine<F>>& edges) {
    std::vector<Affine<F>> tab;
    for (int i = 0; i < 24; i++) tab.push_back(random_point<F>());
    for (const auto& p : tab) { uint64_t w[24]; memcpy(w, &p, sizeof(p)); CHECK(orc_on_curve(Grp<F>::curve, Grp<F>::group, w) == 1, "%s random point off the curve", Grp<F>::name); }
    {   // random tables, random signs; the same points in another order reach the same sum in another projective form
        Chain<F> a("random table"), b("random table, other order"), c("random table, negated");
        for (size_t i = 0; i < tab.size(); i++) { const bool neg = rnd() & 1; a.step(tab[i], neg); if (i % 5 == 4) keep(a); }
        for (size_t i = tab.size(); i-- > 0;) b.step(tab[i], false);
        Chain<F> a2("random table, plain signs");
        for (size_t i = 0; i < tab.size(); i++) { a2.step(tab[i], false); c.step(tab[i], true); }
        keep(a2); keep(b); keep(c);                             // a2 = b = -c
        Chain<F> e("random table, representatives pushed to the ends of their classes");
        for (int i = 0; i < 120; i++) { e.step(tab[rnd() % tab.size()], rnd() & 1); e.push_extreme(); }
        keep(e);
    }
    long dbl = 0, can = 0;
    {   // one point, random signs: the accumulator walks through the small multiples of P, doubling and cancellation recur
        Chain<F> a("one point, random signs");
        long m = 0;                                             // the accumulator is m P; steps lean towards 0 so that it keeps coming back to +-P
        for (int i = 0; i < 240; i++) {
            const bool down = m == 0 ? (rnd() & 1) : ((rnd() % 10 < 7) == (m > 0)), flip = rnd() & 1;
            a.step(flip ? opt_neg(tab[0]) : tab[0], down != flip); m += down ? -1 : 1;
            if (i % 40 == 7) keep(a);
        }
        Chain<F> b("one point, random signs, pushed representatives");
        m = 0;
        for (int i = 0; i < 200; i++) { const bool down = m == 0 ? (rnd() & 1) : ((rnd() % 10 < 7) == (m > 0)); b.step(tab[1], down); m += down ? -1 : 1; b.push_extreme(); }
        dbl += a.doublings + b.doublings; can += a.cancels + b.cancels;
        CHECK(a.doublings >= 5 && a.cancels >= 5 && b.doublings >= 5 && b.cancels >= 5, "%s: the one-point walks met %ld doublings, %ld cancellations", Grp<F>::name, dbl, can);
    }
    {   // the incoming point made equal to the accumulator, or to its negative, with `negate` set and clear, in the middle of a chain
        Chain<F> a("forced doublings and cancellations");
        for (int round = 0; round < 24; round++) {
            const int len = 1 + (int)(rnd() % 3);
            for (int i = 0; i < len; i++) a.step(tab[rnd() % tab.size()], rnd() & 1);
            if (a.ref.is_inf()) continue;
            const Affine<F> cur = a.ref;
            switch (round % 4) {
                case 0: a.step(cur, false); break;                  // doubling
                case 1: a.step(opt_neg(cur), true); break;          // doubling through `negate`
                case 2: a.step(opt_neg(cur), false); break;         // cancellation
                case 3: a.step(cur, true); break;                   // cancellation through `negate`
            }
            if (round % 4 == 0) { a.push_extreme(); a.step(a.ref, false); }     // a doubling again, from pushed representatives
            keep(a);
        }
        CHECK(a.doublings >= 12 && a.cancels >= 8, "%s: forced chain met %ld doublings, %ld cancellations", Grp<F>::name, a.doublings, a.cancels);
    }
    // the first point of a bucket on the boundary values of check 2 (unpack_small without a product), then a doubling, an addition, a cancellation
    for (size_t i = 0; i < edges.size(); i++) {
        // (three oracle inversions per edge point instead of eight: the first point needs none, a cancellation needs none, and a wrong doubling
        // shows in the sums that follow it)
        const bool neg = i & 1;
        const Affine<F> e = neg ? opt_neg(edges[i]) : edges[i], t = tab[i % tab.size()], next = edges[(i + 1) % edges.size()];
        Chain<F> a("edge first point");
        a.quiet_step(edges[i], neg); a.expect(e);
        a.quiet_step(edges[i], neg); a.quiet_step(edges[i], neg);
        if (i % 64 == 0) { a.expect(opt_mul(e, 3)); keep(a); }
        a.quiet_step(t, false); a.expect(opt_add(opt_mul(e, 3), t));
        Chain<F> b("edge first point, cancelled");
        b.quiet_step(edges[i], !neg); b.expect(opt_neg(e));
        b.quiet_step(edges[i], neg); b.expect(Affine<F>::infinity());
        b.quiet_step(edges[i], neg); b.expect(e);
        b.quiet_step(next, false); b.expect(opt_add(e, next));
    }
}

// ---- check 5: bucket operations -----------------------------------------------------------------------------------------------------------------
template <class F> void check_bucket(const char* what, const XYZZL<F>& got, const Affine<F>& want) {
    CHECK(same_point(got, want), "%s %s differs from the oracle", Grp<F>::name, what);
    CHECK((in_class<F, BkClass>(got)), "%s %s leaves a coordinate outside its documented class", Grp<F>::name, what);
}
template <class F> XYZZL<F> bk_negated(const XYZZL<F>& a) { XYZZL<F> r = a; if (!bk_is_inf(a)) r.c[1] = a.c[1].neg().norm(); return r; }
template <class F> bool same_bits(const XYZZL<F>& a, const XYZZL<F>& b) { return memcmp(&a, &b, sizeof(a)) == 0; }
template <class F> void check5() {
    typedef XYZZL<F> B;
    const auto& bk = g_buckets<F>; const auto& ref = g_bucket_refs<F>;
    const B inf = bk_inf<B>();
    CHECK(bk_is_inf(inf) && bk_to_xyzz<F>(inf).is_inf(), "%s bk_inf is not infinity", Grp<F>::name);
    check_bucket("inf + inf", bk_add(inf, inf), Affine<F>::infinity()); check_bucket("2 inf", bk_dbl(inf), Affine<F>::infinity());
    size_t finite = 0;
    for (size_t i = 0; i < bk.size(); i++) {
        const B& a = bk[i];
        if (bk_is_inf(a)) { CHECK(ref[i].is_inf(), "%s infinite bucket, finite oracle value", Grp<F>::name); continue; }
        finite++;
        CHECK(!bk_is_inf(a) && same_point(a, ref[i]), "%s chain output", Grp<F>::name);
        const Affine<F> two = opt_mul(ref[i], 2);
        check_bucket("a + a (bk_add)", bk_add(a, a), two); check_bucket("a + a (bk_add_inl)", bk_add_inl(a, a), two);
        check_bucket("bk_dbl", bk_dbl(a), two); check_bucket("bk_dbl_inl", bk_dbl_inl(a), two);
        const B na = bk_negated(a);
        check_bucket("-a", na, opt_neg(ref[i]));
        CHECK(bk_is_inf(bk_add(a, na)) && bk_is_inf(bk_add_inl(a, na)) && bk_is_inf(bk_add(na, a)) && bk_is_inf(bk_add_inl(na, a)), "%s a + (-a) is not infinity", Grp<F>::name);
        CHECK(same_bits(bk_add(a, inf), a) && same_bits(bk_add(inf, a), a) && same_bits(bk_add_inl(a, inf), a) && same_bits(bk_add_inl(inf, a), a), "%s a + infinity is not a", Grp<F>::name);
        // the same point under other representatives of its coordinates: P = 0 (mod p) with limbs that differ
        for (int t = 0; t < 4; t++) {
            B s = a; const int (*cls[4])[2] = {&BkClass::x, &BkClass::y, &BkClass::z, &BkClass::z};
            for (int f = 0; f < 4; f++) for (int tries = 0; tries < 8; tries++) { const auto cand = lz_shift(a.c[f], (int)(rnd() % 9) - 4, (int)(rnd() % 9) - 4); if (lz_within(cand, *cls[f])) { s.c[f] = cand; break; } }
            check_bucket("a + a' (shifted representatives, bk_add)", bk_add(a, s), two); check_bucket("a' + a (bk_add_inl)", bk_add_inl(s, a), two);
            check_bucket("2 a' (bk_dbl_inl)", bk_dbl_inl(s), two);
            CHECK(bk_is_inf(bk_add_inl(s, na)) && bk_is_inf(bk_add(na, s)), "%s a' + (-a) is not infinity", Grp<F>::name);
        }
        for (size_t j = 0; j < bk.size(); j += 3) {
            const Affine<F> sum = opt_add(ref[i], ref[j]);
            const B r1 = bk_add(a, bk[j]), r2 = bk_add_inl(a, bk[j]);
            check_bucket("a + b (bk_add)", r1, sum); check_bucket("a + b (bk_add_inl)", r2, sum);
            CHECK(same_bits(r1, r2), "%s bk_add and bk_add_inl differ", Grp<F>::name);
            if (j % 2 == 0) check_bucket("(a + b) + a", bk_add_inl(r2, a), opt_add(sum, ref[i]));     // a sum as an operand, as in the reduction trees
        }
        if (i % 4 == 0) for (uint32_t k : {0u, 1u, 2u, 3u, (1u << 15) - 1, 1u << 15}) check_bucket("bk_mul_small", bk_mul_small(a, k), opt_mul(ref[i], k));
    }
    CHECK(finite >= 12, "%s: only %zu finite chain outputs", Grp<F>::name, finite);
    // a + a' and a + (-a') where a' is the SAME point reached by a different chain (another ZZ): entries -3, -2, -1 are a2, b = a2, c = -a2 of check 4's
    // first block ... found by value
    size_t pairs = 0;
    for (size_t i = 0; i < bk.size(); i++) for (size_t j = 0; j < bk.size(); j++) {
        if (i == j || bk_is_inf(bk[i]) || bk_is_inf(bk[j]) || same_bits(bk[i], bk[j])) continue;
        if (same_affine(ref[i], ref[j])) { pairs++; check_bucket("a + a' (two chains)", bk_add_inl(bk[i], bk[j]), opt_mul(ref[i], 2)); check_bucket("a + a' (two chains, bk_add)", bk_add(bk[i], bk[j]), opt_mul(ref[i], 2)); }
        if (same_affine(ref[i], opt_neg(ref[j]))) { pairs++; CHECK(bk_is_inf(bk_add_inl(bk[i], bk[j])) && bk_is_inf(bk_add(bk[i], bk[j])), "%s a + (-a') (two chains) is not infinity", Grp<F>::name); }
    }
    CHECK(pairs >= 4, "%s: only %zu pairs of equal / opposite points in different projective forms", Grp<F>::name, pairs);
    // a running-sum reduction over buckets that are multiples of one point, the shape of k_msm_reduce_segments: equal partial sums meet
    const B* p1 = nullptr; Affine<F> r1 = Affine<F>::infinity();
    for (size_t i = 0; i < bk.size() && !p1; i++) if (!bk_is_inf(bk[i])) { p1 = &bk[i]; r1 = ref[i]; }
    if (p1) {
        const int mult[8] = {1, -1, 0, 2, 1, 1, -2, 3};
        B run = inf, acc = inf; Affine<F> rrun = Affine<F>::infinity(), racc = rrun;
        for (int b = 7; b >= 0; b--) {
            const B piece = mult[b] == 0 ? inf : mult[b] > 0 ? bk_mul_small(*p1, (uint32_t)mult[b]) : bk_negated(bk_mul_small(*p1, (uint32_t)-mult[b]));
            const Affine<F> rp = mult[b] >= 0 ? opt_mul(r1, (uint32_t)mult[b]) : opt_neg(opt_mul(r1, (uint32_t)-mult[b]));
            run = bk_add_inl(run, piece); rrun = opt_add(rrun, rp); check_bucket("running sum", run, rrun);
            acc = bk_add_inl(acc, run); racc = opt_add(racc, rrun); check_bucket("sum of running sums", acc, racc);
        }
    }
}

template <class F> std::vector<Affine<F>> read_edges(FILE* f) {
    std::vector<Affine<F>> out;
    uint64_t n = 0;
    if (!f) return out;
    if (fread(&n, 8, 1, f) != 1 || n == 0 || n > 100000) { printf("edge point file: bad table header\n"); exit(2); }
    for (uint64_t i = 0; i < n; i++) {
        uint64_t w[24];
        if (fread(w, 8, pt_words<F>(), f) != (size_t)pt_words<F>()) { printf("edge point file is truncated\n"); exit(2); }
        CHECK(orc_on_curve(Grp<F>::curve, Grp<F>::group, w) == 1, "%s edge point %llu off the curve", Grp<F>::name, (unsigned long long)i);
        out.push_back(pt_from<F>(w));
    }
    return out;
}
#if LAZY_PART != 2
void run_check1() {
    check1_l29<Bn254Fr>(); check1_l29<Bn254Fq>(); check1_l29<Bls381Fr>(); check1_l29<Bls381Fq>();
    report("check 1: L29 product forms (4 Fr/Fq fields)");
    check1_l29x2<Bn254Fq>(); check1_l29x2<Bls381Fq>();
    report("check 1: L29x2 product forms (2 Fq2 fields)");
}
#endif
#if LAZY_PART != 1
void report(const char* what) { static long last_cases = 0, last_fail = 0; printf("%-58s %9ld cases, %ld failed\n", what, cases - last_cases, failures - last_fail); fflush(stdout); last_cases = cases; last_fail = failures; }

int main(int argc, char** argv) {
    FILE* ef = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (argc > 1 && !ef) { printf("cannot open %s\n", argv[1]); return 2; }
    run_check1();
    check2<Bn254Fr>(); check2<Bn254Fq>(); check2<Bls381Fr>(); check2<Bls381Fq>();
    report("check 2: unpack / unpack_small / one / to_fp / pack_reduced");
    check3<Bn254Fr>(); check3<Bn254Fq>(); check3<Bls381Fr>(); check3<Bls381Fq>();
    report("check 3: maybe_zero_mod_p / is_zero_mod_p");
    // the edge point file holds the four tables in this order
    const auto e1 = read_edges<Bn254Fq>(ef); const auto e2 = read_edges<Fp2<Bn254Fq>>(ef); const auto e3 = read_edges<Bls381Fq>(ef); const auto e4 = read_edges<Fp2<Bls381Fq>>(ef);
    if (ef) fclose(ef);
    printf("edge first points: %zu + %zu + %zu + %zu\n", e1.size(), e2.size(), e3.size(), e4.size());
    check4<Bn254Fq>(e1); check4<Fp2<Bn254Fq>>(e2); check4<Bls381Fq>(e3); check4<Fp2<Bls381Fq>>(e4);
    report("check 4: acc_madd_lazy chains (4 groups)");
    check5<Bn254Fq>(); check5<Fp2<Bn254Fq>>(); check5<Bls381Fq>(); check5<Fp2<Bls381Fq>>();
    report("check 5: bucket operations (4 groups)");
    printf("%ld failure(s)\n", failures);
    return failures ? 1 : 0;
}
#endif
