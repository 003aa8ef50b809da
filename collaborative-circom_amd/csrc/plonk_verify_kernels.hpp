// Kernels of the Plonk verifier (capi_plonk_verify.hip instantiates them for both curves).
//   k_plonk_verify_scalars: one lane per proof runs plonk_verify_scalars (plonk_verify.hpp): six Keccak transcripts, xi^n, the Lagrange
//       part and about twenty scalars, a latency-bound chain.  Workgroups of one wave, for k_miller_batch's reason: a small batch
//       spreads over the compute units.  The nine key-point scalars are also summed over the workgroup (the batch check multiplies each
//       key point by the sum over all proofs): a tree in LDS, idle lanes contribute 0, one partial per workgroup.
//   k_g1_lincomb: out[g] = sum_k s[g, k] P[g, k], one lane per term (XYZZ double-and-add), whole groups per workgroup, the first lane of a
//       group adds its K products with the complete addition and inverts once.  It decides a rejected batch proof by proof.
#pragma once
#include "common.hpp"
#include "plonk_verify.hpp"

namespace cg {

constexpr int PLONK_VERIFY_BLOCK = 64;

template <class C>
struct PlonkVerifyArgs {
    const PlonkVerifyKey<C>* key;
    const Affine<typename C::Fq>* commits;    // n x 9
    const typename C::Fr* evals;              // n x 6
    const typename C::Fr* pubs;               // n x n_pub
    const uint32_t* coeff128;                 // n x 4 or null
    typename C::Fr* challenges;               // n x 6
    typename C::Fr* proof_scalars;            // n x 11
    typename C::Fr* key_scalars;              // n x 9
    int32_t* valid;                           // n
    typename C::Fr* partial;                  // gridDim.x x 9
};

template <class C>
__global__ __launch_bounds__(PLONK_VERIFY_BLOCK) void k_plonk_verify_scalars(PlonkVerifyArgs<C> g, size_t n) {
    typedef typename C::Fr Fr;
    __shared__ Fr tile[PLONK_VERIFY_BLOCK];
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * PLONK_VERIFY_BLOCK + tid;
    Fr sk[PLONK_N_KEY_SCALARS];
    _Pragma("unroll") for (int k = 0; k < PLONK_N_KEY_SCALARS; k++) sk[k] = Fr::zero();
    if (i < n) {
        const PlonkVerifyKey<C>& key = *g.key;                                                 // read where it lies: a copy indexed in a loop would sit in scratch
        Fr ch[PLONK_N_CHALLENGES], sp[PLONK_N_PROOF_SCALARS];
        const int32_t ok = plonk_verify_scalars<C>(key, g.commits + i * PLONK_N_COMMITS, g.evals + i * PLONK_N_EVALS, g.pubs + i * key.n_pub,
                                                   g.coeff128 ? g.coeff128 + 4 * i : nullptr, ch, sp, sk);
        _Pragma("unroll") for (int k = 0; k < PLONK_N_CHALLENGES; k++) g.challenges[i * PLONK_N_CHALLENGES + k] = ch[k];
        _Pragma("unroll") for (int k = 0; k < PLONK_N_PROOF_SCALARS; k++) g.proof_scalars[i * PLONK_N_PROOF_SCALARS + k] = sp[k];
        _Pragma("unroll") for (int k = 0; k < PLONK_N_KEY_SCALARS; k++) g.key_scalars[i * PLONK_N_KEY_SCALARS + k] = sk[k];
        g.valid[i] = ok;
    }
    _Pragma("unroll") for (int k = 0; k < PLONK_N_KEY_SCALARS; k++) {
        Fr acc = sk[k];
        tile[tid] = acc;
        __syncthreads();
        for (int s = PLONK_VERIFY_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) { acc = acc + tile[tid + s]; tile[tid] = acc; }
            __syncthreads();
        }
        if (tid == 0) g.partial[(size_t)blockIdx.x * PLONK_N_KEY_SCALARS + k] = acc;
        __syncthreads();
    }
}

// points, scalars: n_groups x K, group-major; scalars in Montgomery form; K <= PLONK_VERIFY_BLOCK.  A workgroup holds 64 / K whole groups.
template <class Fq, class Fr>
__global__ __launch_bounds__(PLONK_VERIFY_BLOCK) void k_g1_lincomb(const Affine<Fq>* points, const Fr* scalars, size_t n_groups, int K, Affine<Fq>* out) {
    __shared__ XYZZ<Fq> tile[PLONK_VERIFY_BLOCK];
    const int tid = threadIdx.x, per = PLONK_VERIFY_BLOCK / K;
    const int lg = tid / K, lk = tid - lg * K;                                                 // group within the workgroup, term within the group
    const size_t grp = (size_t)blockIdx.x * per + lg;
    const bool live = lg < per && grp < n_groups;
    XYZZ<Fq> acc = XYZZ<Fq>::infinity();
    if (live) {
        const size_t t = grp * (size_t)K + lk;
        const Fr k = scalars[t].from_mont();
        acc = xyzz_scalar_mul(XYZZ<Fq>::from_affine(points[t]), k.v, Fr::N);
    }
    tile[tid] = acc;
    __syncthreads();
    if (live && lk == 0) {
        for (int j = 1; j < K; j++) acc = xyzz_add(acc, tile[tid + j]);                        // equal, opposite and infinite summands included
        out[grp] = xyzz_to_affine(acc);
    }
}

template <class C>
int plonk_verify_scalars_launch(hipStream_t st, const PlonkVerifyArgs<C>& g, size_t n) {
    if (n) hipLaunchKernelGGL((k_plonk_verify_scalars<C>), dim3((unsigned)((n + PLONK_VERIFY_BLOCK - 1) / PLONK_VERIFY_BLOCK)), dim3(PLONK_VERIFY_BLOCK), 0, st, g, n);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class C>
int g1_lincomb_launch(hipStream_t st, const void* d_points, const void* d_scalars, size_t n_groups, int K, void* d_out) {
    const size_t per = PLONK_VERIFY_BLOCK / K;
    if (n_groups) hipLaunchKernelGGL((k_g1_lincomb<typename C::Fq, typename C::Fr>), dim3((unsigned)((n_groups + per - 1) / per)), dim3(PLONK_VERIFY_BLOCK), 0, st,
                                     (const Affine<typename C::Fq>*)d_points, (const typename C::Fr*)d_scalars, n_groups, K, (Affine<typename C::Fq>*)d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace cg
