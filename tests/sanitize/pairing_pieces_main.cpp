// The pieces of csrc/pairing.hpp one by one on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the header compiled as plain C++
// (hip_host_prelude.hpp, pairing_pieces.mk) into a stand-alone program.  It computes and compares nothing itself: it reads a case file, applies
// each primitive to each case and writes the results; tests/test_pairing_pieces_host.py writes the cases and compares every result with the
// integer tower of tests/pairing_tower.py.  A sanitizer report aborts the run.  No GPU, nothing of the product library.
//   usage: pairing_pieces_main <case file> <result file>
// Both files are sequences of blocks of u64 words: a header (curve, kind, count), then count records of the kind's size (L = words per
// base-field element, 4 or 6; an Fp12 is 12 L words in the ABI's layout, everything else is the struct's own bytes):
//   kind            reads                                   writes
//    1 fp12_mul      a, b                                    a b
//    2 fp12_sqr      a                                       a^2
//    3 fp12_conj     a                                       conj(a)
//    4 mul_line      a, line (a0, a1, a3)                    a * line
//    5 fp12_inverse  a                                       1 / a
//    6 fp6_mul       x, y (3 Fp2 each)                       x y
//    7 fp6_inverse   x                                       1 / x
//    8 fp12_frob2    a                                       a^(p^2)
//    9 final_exp     a                                       final_exponentiation(a)
//   10 miller_double T (Jacobian), P                         new T, line
//   11 miller_add    T (Jacobian), R, P                      new T, line
//   12 miller_chain  P, Q, ops (bit i set: step i adds Q)    8 x (new T, line), starting from T = (Q, 1)
//   13 miller_loop   P, Q                                    the value (inputs outside the contract: only the run counts)
//   14 bn_tail       Q                                       pi(Q), -pi^2(Q) as miller_loop forms them (BN254 only)
//   15 unaligned     a                                       a through Fp12::load_host / store_host at addresses = 8 mod 16
// The program is built from this file once per curve (PIECES_CURVE 0 and 1, pairing_pieces.mk); the BLS12-381 object holds main.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pairing.hpp"

using namespace cg;

#ifndef PIECES_CURVE
#error "PIECES_CURVE: 0 = BN254, 1 = BLS12-381"
#endif

struct Block { uint64_t kind, count; const uint64_t* in; };
int run_bn254(const Block& b, std::vector<uint64_t>& out);
int run_bls381(const Block& b, std::vector<uint64_t>& out);

namespace {
constexpr int CHAIN_STEPS = 8;
static const char* const KIND_NAMES[16] = {"", "fp12_mul", "fp12_sqr", "fp12_conj", "mul_line", "fp12_inverse", "fp6_mul", "fp6_inverse", "fp12_frob2",
                                           "final_exp", "miller_double", "miller_add", "miller_chain", "miller_loop", "bn_tail", "unaligned"};

template <class C> struct Io {
    typedef typename C::Fq Fq; typedef typename C::Fq2 Fq2;
    static constexpr size_t L = Fq::N / 2, E = 12 * L;
    const uint64_t* in; std::vector<uint64_t>& out;
    template <class T> T get() { static_assert(sizeof(T) % 8 == 0, ""); T t; memcpy(&t, in, sizeof t); in += sizeof(T) / 8; return t; }
    template <class T> void put(const T& t) { const size_t at = out.size(); out.resize(at + sizeof(T) / 8); memcpy(out.data() + at, &t, sizeof t); }
    Fp12<C> get12() { alignas(16) uint64_t w[E]; memcpy(w, in, sizeof w); in += E; return Fp12<C>::load(w); }
    void put12(const Fp12<C>& a) { alignas(16) uint64_t w[E]; a.store(w); const size_t at = out.size(); out.resize(at + E); memcpy(out.data() + at, w, sizeof w); }
};

// words read per record, or 0 for a kind the curve does not have
template <class C> size_t record_words(uint64_t kind) {
    const size_t L = C::Fq::N / 2, E = 12 * L;
    switch (kind) {
        case 1: return 2 * E;
        case 2: case 3: case 5: case 8: case 9: case 15: return E;
        case 4: return E + 6 * L;
        case 6: return 12 * L;
        case 7: return 6 * L;
        case 10: return 8 * L;
        case 11: return 12 * L;
        case 12: return 6 * L + 1;
        case 13: return 6 * L;
        case 14: return C::BN ? 4 * L : 0;
    }
    return 0;
}

template <class C> int run(const Block& b, std::vector<uint64_t>& out) {
    typedef typename C::Fq Fq; typedef typename C::Fq2 Fq2;
    Io<C> io{b.in, out};
    for (uint64_t n = 0; n < b.count; n++) {
        switch (b.kind) {
            case 1: { const Fp12<C> x = io.get12(), y = io.get12(); Fp12<C> r; fp12_mul(&r, &x, &y); io.put12(r); break; }
            case 2: { const Fp12<C> x = io.get12(); Fp12<C> r; fp12_sqr(&r, &x); io.put12(r); break; }
            case 3: { io.put12(fp12_conj(io.get12())); break; }
            case 4: { const Fp12<C> x = io.get12(); const Line<C> l = io.template get<Line<C>>(); Fp12<C> r; fp12_mul_line(&r, &x, &l); io.put12(r); break; }
            case 5: { const Fp12<C> x = io.get12(); Fp12<C> r; fp12_inverse(&r, &x); io.put12(r); break; }
            case 6: { const Fp6<C> x = io.template get<Fp6<C>>(), y = io.template get<Fp6<C>>(); io.put(fp6_mul(x, y)); break; }
            case 7: { io.put(fp6_inverse(io.template get<Fp6<C>>())); break; }
            case 8: { io.put12(fp12_frob2(io.get12())); break; }
            case 9: { const Fp12<C> x = io.get12(); Fp12<C> r; final_exponentiation(&r, &x); io.put12(r); break; }
            case 10: {
                Jacobian<Fq2> T = io.template get<Jacobian<Fq2>>(); const Affine<Fq> P = io.template get<Affine<Fq>>();
                Line<C> l; miller_double(&T, &P, &l); io.put(T); io.put(l); break;
            }
            case 11: {
                Jacobian<Fq2> T = io.template get<Jacobian<Fq2>>(); const Affine<Fq2> R = io.template get<Affine<Fq2>>(); const Affine<Fq> P = io.template get<Affine<Fq>>();
                Line<C> l; miller_add(&T, &R, &P, &l); io.put(T); io.put(l); break;
            }
            case 12: {
                const Affine<Fq> P = io.template get<Affine<Fq>>(); const Affine<Fq2> Q = io.template get<Affine<Fq2>>(); const uint64_t ops = io.template get<uint64_t>();
                Jacobian<Fq2> T{Q.x, Q.y, Fq2::one()}; Line<C> l;
                for (int s = 0; s < CHAIN_STEPS; s++) { if ((ops >> s) & 1) miller_add(&T, &Q, &P, &l); else miller_double(&T, &P, &l); io.put(T); io.put(l); }
                break;
            }
            case 13: {
                const Affine<Fq> P = io.template get<Affine<Fq>>(); const Affine<Fq2> Q = io.template get<Affine<Fq2>>();
                Fp12<C> f; miller_loop(&f, &P, &Q); io.put12(f); break;
            }
            case 14: {
                if constexpr (C::BN) {       // the two expressions of miller_loop's tail, on the generated constants
                    const Affine<Fq2> Q = io.template get<Affine<Fq2>>();
                    const Fq2 gx{fp_from_limbs<Fq>(C::K::TWIST_X), fp_from_limbs<Fq>(C::K::TWIST_X + Fq::N)}, gy{fp_from_limbs<Fq>(C::K::TWIST_Y), fp_from_limbs<Fq>(C::K::TWIST_Y + Fq::N)};
                    const Affine<Fq2> Q1{fp2_conjugate(Q.x) * gx, fp2_conjugate(Q.y) * gy};
                    const Affine<Fq2> Q2{fp2_conjugate(Q1.x) * gx, (fp2_conjugate(Q1.y) * gy).neg()};
                    io.put(Q1); io.put(Q2);
                }
                break;
            }
            case 15: {
                // what the host entries of capi_pairing.hip do with a caller's pointer, on buffers that are 8- but not 16-byte aligned
                constexpr size_t E = Io<C>::E;
                alignas(16) uint64_t src[E + 2], dst[E + 2];
                memcpy(src + 1, io.in, E * 8); io.in += E;
                if (((uintptr_t)(src + 1) & 15) != 8 || ((uintptr_t)(dst + 1) & 15) != 8) { printf("unaligned: the buffers are not at 8 mod 16\n"); return 1; }
                const Fp12<C> a = Fp12<C>::load_host(src + 1);
                a.store_host(dst + 1);
                const size_t at = out.size(); out.resize(at + E); memcpy(out.data() + at, dst + 1, E * 8);
                break;
            }
            default: return 1;
        }
    }
    return 0;
}
}  // namespace

#if PIECES_CURVE == 0
int run_bn254(const Block& b, std::vector<uint64_t>& out) { return run<Bn254Pairing>(b, out); }
size_t record_words_bn254(uint64_t kind) { return record_words<Bn254Pairing>(kind); }
#else
size_t record_words_bn254(uint64_t kind);
int run_bls381(const Block& b, std::vector<uint64_t>& out) { return run<Bls381Pairing>(b, out); }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: pairing_pieces_main <case file> <result file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint64_t> in;
    { uint64_t buf[4096]; size_t got; while ((got = fread(buf, 8, 4096, f)) > 0) in.insert(in.end(), buf, buf + got); }
    fclose(f);
    std::vector<uint64_t> out;
    size_t at = 0;
    while (at < in.size()) {
        if (in.size() - at < 3) { printf("case file: truncated header\n"); return 2; }
        const uint64_t curve = in[at], kind = in[at + 1], count = in[at + 2];
        at += 3;
        const size_t words = curve == 0 ? record_words_bn254(kind) : curve == 1 ? record_words<Bls381Pairing>(kind) : 0;
        if (!words || kind > 15) { printf("case file: unknown curve %llu or kind %llu\n", (unsigned long long)curve, (unsigned long long)kind); return 2; }
        if (count > (in.size() - at) / words) { printf("case file: truncated block\n"); return 2; }
        const Block b{kind, count, in.data() + at};
        out.push_back(curve); out.push_back(kind); out.push_back(count);
        if (curve == 0 ? run_bn254(b, out) : run_bls381(b, out)) { printf("failed in %s\n", KIND_NAMES[kind]); return 1; }
        at += count * words;
        printf("%s %s: %llu cases\n", curve == 0 ? "bn254" : "bls12_381", KIND_NAMES[kind], (unsigned long long)count);
        fflush(stdout);
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), 8, out.size(), g) != out.size() || fclose(g) != 0) { printf("cannot write %s\n", argv[2]); return 2; }
    printf("done\n");
    return 0;
}
#endif
