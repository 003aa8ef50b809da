// Pairing kernels: one lane per (P, Q) pair.  Included by pairing_inst_<curve>.hip only (explicit instantiation per curve).
// Fp12 values cross the kernel boundary in the ABI's (2, 3, 2, limbs) layout (pairing.hpp).
#pragma once
#include "common.hpp"
#include "pairing.hpp"

namespace cg {

// Workgroups of one wave: the launches are latency-bound chains of ~17 000 base-field products per lane, so the lanes are spread over as
// many compute units as there are waves; the product tree's tile is 64 x 384 B (BN254) or 64 x 576 B (BLS12-381: 36 KiB of the 160 KiB LDS).
// (PAIRING_BLOCK, PAIRING_PRODUCT_GROUPS_MAX: pairing.hpp)

// out[i] = Miller(k_i P_i, Q_i); scalars (optional): 4 x u32 per lane, canonical little-endian 128-bit integers
template <class C>
__global__ __launch_bounds__(PAIRING_BLOCK) void k_miller_batch(const Affine<typename C::Fq>* g1, const Affine<typename C::Fq2>* g2, const uint32_t* scalars, size_t n, uint8_t* out) {
    typedef typename C::Fq Fq;
    const size_t i = (size_t)blockIdx.x * PAIRING_BLOCK + threadIdx.x;
    if (i >= n) return;
    Affine<Fq> P = g1[i];
    const Affine<typename C::Fq2> Q = g2[i];
    if (scalars && !P.is_inf()) P = xyzz_to_affine(xyzz_scalar_mul(XYZZ<Fq>::from_affine(P), scalars + 4 * i, 4));   // one inversion per lane, outside the loop
    Fp12<C> f;
    miller_loop(&f, &P, &Q);
    f.store(out + i * sizeof(Fp12<C>));
}

// partial[g] = product of the values workgroup g strides over: per lane first, then a tree in LDS
template <class C>
__global__ __launch_bounds__(PAIRING_BLOCK) void k_fp12_product(const uint8_t* in, size_t n, uint8_t* partial) {
    __shared__ Fp12<C> tile[PAIRING_BLOCK];
    const int tid = threadIdx.x;
    Fp12<C> acc = Fp12<C>::one(), t, u;
    for (size_t i = (size_t)blockIdx.x * PAIRING_BLOCK + tid; i < n; i += (size_t)gridDim.x * PAIRING_BLOCK) {
        t = Fp12<C>::load(in + i * sizeof(Fp12<C>));
        fp12_mul(&u, &acc, &t); acc = u;
    }
    tile[tid] = acc;
    __syncthreads();
    for (int s = PAIRING_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) { t = tile[tid + s]; fp12_mul(&u, &acc, &t); acc = u; tile[tid] = acc; }
        __syncthreads();
    }
    if (tid == 0) acc.store(partial + (size_t)blockIdx.x * sizeof(Fp12<C>));
}

// ok[i] = FE(in[i k] * .. * in[i k + k - 1]) == target
template <class C>
__global__ __launch_bounds__(PAIRING_BLOCK) void k_final_exp_check(const uint8_t* in, int k, size_t n, const uint8_t* target, int32_t* ok) {
    const size_t i = (size_t)blockIdx.x * PAIRING_BLOCK + threadIdx.x;
    if (i >= n) return;
    Fp12<C> acc = Fp12<C>::load(in + i * k * sizeof(Fp12<C>)), t, u;
    for (int j = 1; j < k; j++) { t = Fp12<C>::load(in + (i * k + j) * sizeof(Fp12<C>)); fp12_mul(&u, &acc, &t); acc = u; }
    final_exponentiation(&u, &acc);
    t = Fp12<C>::load(target);
    ok[i] = u == t ? 1 : 0;
}

inline unsigned pairing_grid(size_t n) { return (unsigned)((n + PAIRING_BLOCK - 1) / PAIRING_BLOCK); }

template <class C>
int miller_batch_launch(hipStream_t st, const void* d_g1, const void* d_g2, const uint32_t* d_scalars, size_t n, void* d_out) {
    if (n) hipLaunchKernelGGL((k_miller_batch<C>), dim3(pairing_grid(n)), dim3(PAIRING_BLOCK), 0, st, (const Affine<typename C::Fq>*)d_g1, (const Affine<typename C::Fq2>*)d_g2, d_scalars, n, (uint8_t*)d_out);
    HIPCHK(hipGetLastError());
    return 0;
}
// d_partial receives *groups values (at most PAIRING_PRODUCT_GROUPS_MAX); n > 0
template <class C>
int fp12_product_launch(hipStream_t st, const void* d_in, size_t n, void* d_partial, int* groups) {
    *groups = (int)std::min<size_t>(pairing_grid(n), PAIRING_PRODUCT_GROUPS_MAX);
    hipLaunchKernelGGL((k_fp12_product<C>), dim3(*groups), dim3(PAIRING_BLOCK), 0, st, (const uint8_t*)d_in, n, (uint8_t*)d_partial);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class C>
int final_exp_check_launch(hipStream_t st, const void* d_in, int k, size_t n, const void* d_target, int32_t* d_ok) {
    if (n) hipLaunchKernelGGL((k_final_exp_check<C>), dim3(pairing_grid(n)), dim3(PAIRING_BLOCK), 0, st, (const uint8_t*)d_in, k, n, (const uint8_t*)d_target, d_ok);
    HIPCHK(hipGetLastError());
    return 0;
}

#define CG_INSTANTIATE_PAIRING(C)                                                                                      \
    namespace cg {                                                                                                     \
    template int miller_batch_launch<C>(hipStream_t, const void*, const void*, const uint32_t*, size_t, void*);        \
    template int fp12_product_launch<C>(hipStream_t, const void*, size_t, void*, int*);                                \
    template int final_exp_check_launch<C>(hipStream_t, const void*, int, size_t, const void*, int32_t*);              \
    }

}  // namespace cg
