// C ABI of the pairing layer (include/cogroth16_hip.h): host entry points compiled from the same pairing.hpp the kernels use, and the launch
// logic of the batch kernels of pairing_inst_*.hip.
#include "capi_internal.hpp"
#include "pairing.hpp"

namespace cg {
template <class C> int miller_batch_launch(hipStream_t st, const void* d_g1, const void* d_g2, const uint32_t* d_scalars, size_t n, void* d_out);
template <class C> int fp12_product_launch(hipStream_t st, const void* d_in, size_t n, void* d_partial, int* groups);
template <class C> int final_exp_check_launch(hipStream_t st, const void* d_in, int k, size_t n, const void* d_target, int32_t* d_ok);
}

namespace {
template <class Fn> int with_pairing(int curve, Fn&& fn) {
    if (curve == CG_BN254) return fn(Bn254Pairing{});
#if CG_WITH_BLS
    if (curve == CG_BLS12_381) return fn(Bls381Pairing{});
#else
    if (curve == CG_BLS12_381) return fail(CG_ERR_ARG, "library built without BLS12-381 (make BLS=1)");
#endif
    return fail(CG_ERR_ARG, "unknown curve id");
}
// device scratch of one call, released when the call returns
struct DevTmp {
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { HIPCHK(hip_malloc_flush(&p, std::max<size_t>(bytes, 16))); return 0; }
};
template <class C> void load_pair(const void* h_g1, const void* h_g2, size_t i, Affine<typename C::Fq>& P, Affine<typename C::Fq2>& Q) {
    memcpy(&P, (const uint8_t*)h_g1 + i * sizeof P, sizeof P); memcpy(&Q, (const uint8_t*)h_g2 + i * sizeof Q, sizeof Q);
}
// uploads n pairs (and the optional 128-bit scalars) and leaves the n Miller values in d_out
template <class C> int miller_to_device(cg_ctx* ctx, const void* h_g1, const void* h_g2, const void* h_scalars128, size_t n, DevTmp& d_out) {
    DevTmp d1, d2, ds;
    const size_t b1 = n * sizeof(Affine<typename C::Fq>), b2 = n * sizeof(Affine<typename C::Fq2>);
    if (int rc = d1.alloc(b1)) return rc;
    if (int rc = d2.alloc(b2)) return rc;
    if (int rc = d_out.alloc(n * sizeof(Fp12<C>))) return rc;
    HIPCHK(hipMemcpyAsync(d1.p, h_g1, b1, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d2.p, h_g2, b2, hipMemcpyHostToDevice, ctx->stream));
    if (h_scalars128) { if (int rc = ds.alloc(n * 16)) return rc; HIPCHK(hipMemcpyAsync(ds.p, h_scalars128, n * 16, hipMemcpyHostToDevice, ctx->stream)); }
    if (int rc = miller_batch_launch<C>(ctx->stream, d1.p, d2.p, (const uint32_t*)ds.p, n, d_out.p)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the inputs go away with this scope
    return 0;
}
}  // namespace

extern "C" {

int32_t cg_pairing(int32_t curve, const void* h_g1_affine, const void* h_g2_affine, void* h_out_fp12) {
    if (!h_g1_affine || !h_g2_affine || !h_out_fp12) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        Affine<typename C::Fq> P; Affine<typename C::Fq2> Q; load_pair<C>(h_g1_affine, h_g2_affine, 0, P, Q);
        Fp12<C> f, e;
        miller_loop(&f, &P, &Q); final_exponentiation(&e, &f);
        e.store_host(h_out_fp12); return 0;
    });
}
int32_t cg_final_exp(int32_t curve, const void* h_in, void* h_out) {
    if (!h_in || !h_out) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        Fp12<C> f = Fp12<C>::load_host(h_in), e;
        final_exponentiation(&e, &f);
        e.store_host(h_out); return 0;
    });
}
int32_t cg_fp12_mul(int32_t curve, const void* h_a, const void* h_b, void* h_out) {
    if (!h_a || !h_b || !h_out) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        const Fp12<C> a = Fp12<C>::load_host(h_a), b = Fp12<C>::load_host(h_b);
        (a * b).store_host(h_out); return 0;
    });
}
int32_t cg_fp12_pow(int32_t curve, const void* h_a, const void* h_exp, int32_t exp_limbs64, void* h_out) {
    if (!h_a || !h_exp || !h_out || exp_limbs64 < 0) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        const Fp12<C> a = Fp12<C>::load_host(h_a); Fp12<C> r = Fp12<C>::one(), t;
        const uint64_t* e = (const uint64_t*)h_exp;
        for (int b = exp_limbs64 * 64 - 1; b >= 0; b--) {
            fp12_sqr(&t, &r); r = t;
            if ((e[b >> 6] >> (b & 63)) & 1u) { fp12_mul(&t, &r, &a); r = t; }
        }
        r.store_host(h_out); return 0;
    });
}
int32_t cg_miller_loop(int32_t curve, const void* h_g1, const void* h_g2, size_t n, void* h_out_fp12) {
    if ((n && (!h_g1 || !h_g2)) || !h_out_fp12) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        Fp12<C> acc = Fp12<C>::one(), f, t;
        for (size_t i = 0; i < n; i++) {
            Affine<typename C::Fq> P; Affine<typename C::Fq2> Q; load_pair<C>(h_g1, h_g2, i, P, Q);
            miller_loop(&f, &P, &Q); fp12_mul(&t, &acc, &f); acc = t;
        }
        acc.store_host(h_out_fp12); return 0;
    });
}
int32_t cg_pairing_check(int32_t curve, const void* h_g1, const void* h_g2, size_t n, int32_t* ok) {
    if ((n && (!h_g1 || !h_g2)) || !ok) return fail(CG_ERR_ARG, "null argument");
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        Fp12<C> acc = Fp12<C>::one(), f, t;
        for (size_t i = 0; i < n; i++) {
            Affine<typename C::Fq> P; Affine<typename C::Fq2> Q; load_pair<C>(h_g1, h_g2, i, P, Q);
            miller_loop(&f, &P, &Q); fp12_mul(&t, &acc, &f); acc = t;
        }
        final_exponentiation(&t, &acc);
        *ok = t == Fp12<C>::one() ? 1 : 0; return 0;
    });
}

int32_t cg_miller_batch(cg_ctx* ctx, int32_t curve, const void* h_g1, const void* h_g2, size_t n, void* h_out_fp12s) {
    if (!ctx || (n && (!h_g1 || !h_g2 || !h_out_fp12s))) return fail(CG_ERR_ARG, "null argument");
    if (!n) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        DevTmp d_out;
        if (int rc = miller_to_device<C>(ctx, h_g1, h_g2, nullptr, n, d_out)) return rc;
        HIPCHK(hipMemcpy(h_out_fp12s, d_out.p, n * sizeof(Fp12<C>), hipMemcpyDeviceToHost));
        return 0;
    });
}
int32_t cg_miller_product(cg_ctx* ctx, int32_t curve, const void* h_g1, const void* h_g2, const void* h_scalars128, size_t n, void* h_out_fp12) {
    if (!ctx || !h_out_fp12 || (n && (!h_g1 || !h_g2))) return fail(CG_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        Fp12<C> acc = Fp12<C>::one();
        if (n) {
            DevTmp d_vals, d_part;
            if (int rc = miller_to_device<C>(ctx, h_g1, h_g2, h_scalars128, n, d_vals)) return rc;
            if (int rc = d_part.alloc(PAIRING_PRODUCT_GROUPS_MAX * sizeof(Fp12<C>))) return rc;
            int groups = 0;
            if (int rc = fp12_product_launch<C>(ctx->stream, d_vals.p, n, d_part.p, &groups)) return rc;
            std::vector<uint8_t> part((size_t)groups * sizeof(Fp12<C>));
            HIPCHK(hipMemcpyAsync(part.data(), d_part.p, part.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            for (int g = 0; g < groups; g++) { const Fp12<C> p = Fp12<C>::load_host(part.data() + (size_t)g * sizeof(Fp12<C>)); Fp12<C> t; fp12_mul(&t, &acc, &p); acc = t; }
        }
        acc.store_host(h_out_fp12); return 0;
    });
}
int32_t cg_final_exp_check_batch(cg_ctx* ctx, int32_t curve, const void* h_fp12s, int32_t k, size_t n, const void* h_target_fp12, int32_t* ok) {
    if (!ctx || !h_target_fp12 || k < 1 || (n && (!h_fp12s || !ok))) return fail(CG_ERR_ARG, "null argument or k < 1");
    if (!n) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    return with_pairing(curve, [&](auto tag) -> int {
        typedef decltype(tag) C;
        DevTmp d_in, d_t, d_ok;
        const size_t bytes = n * (size_t)k * sizeof(Fp12<C>);
        if (int rc = d_in.alloc(bytes)) return rc;
        if (int rc = d_t.alloc(sizeof(Fp12<C>))) return rc;
        if (int rc = d_ok.alloc(n * 4)) return rc;
        HIPCHK(hipMemcpyAsync(d_in.p, h_fp12s, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_t.p, h_target_fp12, sizeof(Fp12<C>), hipMemcpyHostToDevice, ctx->stream));
        if (int rc = final_exp_check_launch<C>(ctx->stream, d_in.p, k, n, d_t.p, (int32_t*)d_ok.p)) return rc;
        HIPCHK(hipMemcpyAsync(ok, d_ok.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    });
}

}  // extern "C"
