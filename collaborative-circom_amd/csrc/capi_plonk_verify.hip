// C ABI of the Plonk verifier's per-proof layer (include/cogroth16_hip.h): the scalars of n proofs on the GPU, the same function in a host
// loop (one source: plonk_verify.hpp), and the batched G1 linear combinations that decide a rejected batch proof by proof.
#include "capi_internal.hpp"
#include "pairing.hpp"
#include "plonk_verify_kernels.hpp"

namespace {
template <class Fn> int with_plonk_curve(int curve, Fn&& fn) {
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
    int put(cg_ctx* ctx, const void* h, size_t bytes) {
        if (int rc = alloc(bytes)) return rc;
        if (bytes) HIPCHK(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
};
template <class C>
int load_key(PlonkVerifyKey<C>& key, const void* h_key_points, const void* h_k1, const void* h_k2, const void* h_omega, int32_t power, size_t n_pub) {
    if (power < 0 || power > 32) return fail(CG_ERR_ARG, "power outside [0, 32]");
    if (n_pub > ((size_t)1 << 24)) return fail(CG_ERR_ARG, "too many public inputs");
    memset(&key, 0, sizeof key);
    memcpy(key.pts, h_key_points, sizeof key.pts);
    memcpy(&key.k1, h_k1, sizeof key.k1); memcpy(&key.k2, h_k2, sizeof key.k2); memcpy(&key.omega, h_omega, sizeof key.omega);
    key.power = (uint32_t)power; key.n_pub = (uint32_t)n_pub;
    return 0;
}
bool null_args(const void* h_key_points, const void* h_k1, const void* h_k2, const void* h_omega, const void* h_commits, const void* h_evals, const void* h_pubs, size_t n_pub, size_t n,
               const void* h_challenges, const void* h_proof_scalars, const void* h_key_scalars, const void* h_valid, const void* h_key_sums) {
    return !h_key_points || !h_k1 || !h_k2 || !h_omega || !h_key_sums || (n && (!h_commits || !h_evals || (n_pub && !h_pubs) || !h_challenges || !h_proof_scalars || !h_key_scalars || !h_valid));
}
}  // namespace

extern "C" {

int32_t cg_plonk_verify_scalars_host(int32_t curve, const void* h_key_points, const void* h_k1, const void* h_k2, const void* h_omega, int32_t power,
                                     const void* h_commits, const void* h_evals, const void* h_pubs, size_t n_pub, size_t n, const void* h_coeff128,
                                     void* h_challenges, void* h_proof_scalars, void* h_key_scalars, int32_t* h_valid, void* h_key_sums) {
    if (null_args(h_key_points, h_k1, h_k2, h_omega, h_commits, h_evals, h_pubs, n_pub, n, h_challenges, h_proof_scalars, h_key_scalars, h_valid, h_key_sums)) return fail(CG_ERR_ARG, "null argument");
    return with_plonk_curve(curve, [&](auto tag) -> int {
        typedef decltype(tag) C; typedef typename C::Fr Fr; typedef Affine<typename C::Fq> Pt;
        PlonkVerifyKey<C> key;
        if (int rc = load_key<C>(key, h_key_points, h_k1, h_k2, h_omega, power, n_pub)) return rc;
        Fr sums[PLONK_N_KEY_SCALARS];
        for (auto& s : sums) s = Fr::zero();
        // The caller's buffers need only be 8-byte aligned (u64 arrays), Fr and Pt are alignas(16): every proof goes through aligned locals.
        Pt commits[PLONK_N_COMMITS]; Fr evals[PLONK_N_EVALS], ch[PLONK_N_CHALLENGES], sp[PLONK_N_PROOF_SCALARS], sk[PLONK_N_KEY_SCALARS];
        std::vector<Fr> pubs(n_pub);
        for (size_t i = 0; i < n; i++) {
            memcpy(commits, (const uint8_t*)h_commits + i * sizeof commits, sizeof commits);
            memcpy(evals, (const uint8_t*)h_evals + i * sizeof evals, sizeof evals);
            if (n_pub) memcpy(pubs.data(), (const uint8_t*)h_pubs + i * n_pub * sizeof(Fr), n_pub * sizeof(Fr));
            h_valid[i] = plonk_verify_scalars<C>(key, commits, evals, pubs.data(), h_coeff128 ? (const uint32_t*)h_coeff128 + 4 * i : nullptr, ch, sp, sk);
            memcpy((uint8_t*)h_challenges + i * sizeof ch, ch, sizeof ch);
            memcpy((uint8_t*)h_proof_scalars + i * sizeof sp, sp, sizeof sp);
            memcpy((uint8_t*)h_key_scalars + i * sizeof sk, sk, sizeof sk);
            for (int k = 0; k < PLONK_N_KEY_SCALARS; k++) sums[k] = sums[k] + sk[k];
        }
        memcpy(h_key_sums, sums, sizeof sums);
        return 0;
    });
}

int32_t cg_plonk_verify_scalars(cg_ctx* ctx, int32_t curve, const void* h_key_points, const void* h_k1, const void* h_k2, const void* h_omega, int32_t power,
                                const void* h_commits, const void* h_evals, const void* h_pubs, size_t n_pub, size_t n, const void* h_coeff128,
                                void* h_challenges, void* h_proof_scalars, void* h_key_scalars, int32_t* h_valid, void* h_key_sums) {
    if (!ctx || null_args(h_key_points, h_k1, h_k2, h_omega, h_commits, h_evals, h_pubs, n_pub, n, h_challenges, h_proof_scalars, h_key_scalars, h_valid, h_key_sums)) return fail(CG_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    return with_plonk_curve(curve, [&](auto tag) -> int {
        typedef decltype(tag) C; typedef typename C::Fr Fr; typedef Affine<typename C::Fq> Pt;
        PlonkVerifyKey<C> key;
        if (int rc = load_key<C>(key, h_key_points, h_k1, h_k2, h_omega, power, n_pub)) return rc;
        Fr sums[PLONK_N_KEY_SCALARS];
        for (auto& s : sums) s = Fr::zero();
        if (n) {
            const size_t groups = (n + PLONK_VERIFY_BLOCK - 1) / PLONK_VERIFY_BLOCK;
            DevTmp d_key, d_commits, d_evals, d_pubs, d_coeff, d_ch, d_sp, d_sk, d_valid, d_part;
            if (int rc = d_key.put(ctx, &key, sizeof key)) return rc;
            if (int rc = d_commits.put(ctx, h_commits, n * PLONK_N_COMMITS * sizeof(Pt))) return rc;
            if (int rc = d_evals.put(ctx, h_evals, n * PLONK_N_EVALS * sizeof(Fr))) return rc;
            if (int rc = d_pubs.put(ctx, h_pubs, n * n_pub * sizeof(Fr))) return rc;
            if (h_coeff128) { if (int rc = d_coeff.put(ctx, h_coeff128, n * 16)) return rc; }
            if (int rc = d_ch.alloc(n * PLONK_N_CHALLENGES * sizeof(Fr))) return rc;
            if (int rc = d_sp.alloc(n * PLONK_N_PROOF_SCALARS * sizeof(Fr))) return rc;
            if (int rc = d_sk.alloc(n * PLONK_N_KEY_SCALARS * sizeof(Fr))) return rc;
            if (int rc = d_valid.alloc(n * sizeof(int32_t))) return rc;
            if (int rc = d_part.alloc(groups * PLONK_N_KEY_SCALARS * sizeof(Fr))) return rc;
            PlonkVerifyArgs<C> g;
            g.key = (const PlonkVerifyKey<C>*)d_key.p; g.commits = (const Pt*)d_commits.p; g.evals = (const Fr*)d_evals.p; g.pubs = (const Fr*)d_pubs.p;
            g.coeff128 = (const uint32_t*)d_coeff.p; g.challenges = (Fr*)d_ch.p; g.proof_scalars = (Fr*)d_sp.p; g.key_scalars = (Fr*)d_sk.p;
            g.valid = (int32_t*)d_valid.p; g.partial = (Fr*)d_part.p;
            if (int rc = plonk_verify_scalars_launch<C>(ctx->stream, g, n)) return rc;
            std::vector<Fr> part(groups * PLONK_N_KEY_SCALARS);
            HIPCHK(hipMemcpyAsync(h_challenges, d_ch.p, n * PLONK_N_CHALLENGES * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_proof_scalars, d_sp.p, n * PLONK_N_PROOF_SCALARS * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_key_scalars, d_sk.p, n * PLONK_N_KEY_SCALARS * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(h_valid, d_valid.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(part.data(), d_part.p, part.size() * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));                                          // the device buffers go away with this scope
            for (size_t w = 0; w < groups; w++) for (int k = 0; k < PLONK_N_KEY_SCALARS; k++) sums[k] = sums[k] + part[w * PLONK_N_KEY_SCALARS + k];
        }
        memcpy(h_key_sums, sums, sizeof sums);
        return 0;
    });
}

int32_t cg_g1_lincomb_batch(cg_ctx* ctx, int32_t curve, const void* h_points, const void* h_scalars, size_t n_groups, int32_t k_terms, void* h_out_affine) {
    if (!ctx || (n_groups && (!h_points || !h_scalars || !h_out_affine))) return fail(CG_ERR_ARG, "null argument");
    if (k_terms < 1 || k_terms > PLONK_VERIFY_BLOCK) return fail(CG_ERR_ARG, "k_terms outside [1, 64]");
    if (!n_groups) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    return with_plonk_curve(curve, [&](auto tag) -> int {
        typedef decltype(tag) C; typedef typename C::Fr Fr; typedef Affine<typename C::Fq> Pt;
        const size_t terms = n_groups * (size_t)k_terms;
        DevTmp d_pts, d_sc, d_out;
        if (int rc = d_pts.put(ctx, h_points, terms * sizeof(Pt))) return rc;
        if (int rc = d_sc.put(ctx, h_scalars, terms * sizeof(Fr))) return rc;
        if (int rc = d_out.alloc(n_groups * sizeof(Pt))) return rc;
        if (int rc = g1_lincomb_launch<C>(ctx->stream, d_pts.p, d_sc.p, n_groups, k_terms, d_out.p)) return rc;
        HIPCHK(hipMemcpyAsync(h_out_affine, d_out.p, n_groups * sizeof(Pt), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    });
}

}  // extern "C"
