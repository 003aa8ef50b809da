// R1CS on the device: the witness check <A_i,w> * <B_i,w> == <C_i,w> over all rows in one pass, and the column sums
// u_i = sum_j M[j][i] * L_j of the QAP (Groth16 setup) from the column-major form of a constraint matrix.
// Row / column strategy as k_spmv_csr / k_spmv_csr_wave (vec_kernels.hpp): a lane per short row, a wave per long one.
#pragma once
#include "launchers.hpp"
#include "vec_kernels.hpp"

namespace cg {

// sum_k coeff[k] * w[col[k]] over the terms k = begin + first, begin + first + step, .. of one row
template <class F>
__device__ __forceinline__ F r1cs_row_dot(const R1csMat& m, size_t row, const F* __restrict__ w, uint32_t first, uint32_t step) {
    F acc = F::zero();
    const uint32_t e = m.row_ptr[row + 1];
    for (uint32_t k = m.row_ptr[row] + first; k < e; k += step) acc = acc + ld_fp((const F*)m.coeff + k) * ld_fp(w + m.col[k]);
    return acc;
}
// every lane's (count, smallest row) -> result[0] += count, result[1] = min(result[1], row): shuffles inside the wave, LDS across the
// workgroup's four waves, one atomic each per workgroup (none when the workgroup found nothing)
__device__ __forceinline__ void r1cs_report(unsigned long long count, unsigned long long first, unsigned long long* __restrict__ result) {
    __shared__ unsigned long long s_count[4], s_first[4];
    for (int off = 32; off >= 1; off >>= 1) {
        count += __shfl_down(count, off, 64);
        const unsigned long long o = __shfl_down(first, off, 64);
        first = o < first ? o : first;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { s_count[wave] = count; s_first[wave] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; i++) { count += s_count[i]; first = s_first[i] < first ? s_first[i] : first; }
        if (count) { atomicAdd(result, count); atomicMin(result + 1, first); }
    }
}
// a lane per row triple.  blockDim.x == 256.
template <class F>
__global__ void __launch_bounds__(256) k_r1cs_check(R1csMat A, R1csMat B, R1csMat C, size_t n_rows, const F* __restrict__ w, unsigned long long* __restrict__ result) {
    unsigned long long count = 0, first = ~0ull;
    for (size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (size_t)gridDim.x * blockDim.x) {
        const F a = r1cs_row_dot<F>(A, row, w, 0, 1), b = r1cs_row_dot<F>(B, row, w, 0, 1), c = r1cs_row_dot<F>(C, row, w, 0, 1);
        if (a * b != c) { count++; first = row < first ? row : first; }       // rows ascend per lane: the first hit is the smallest
    }
    r1cs_report(count, first, result);
}
// a 64-lane wave per row triple: lanes stride over the terms of A_i, B_i and C_i, three cross-lane field sums, lane 0 decides
template <class F>
__global__ void __launch_bounds__(256) k_r1cs_check_wave(R1csMat A, R1csMat B, R1csMat C, size_t n_rows, const F* __restrict__ w, unsigned long long* __restrict__ result) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long count = 0, first = ~0ull;
    for (size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < n_rows; row += ((size_t)gridDim.x * blockDim.x) >> 6) {
        F a = r1cs_row_dot<F>(A, row, w, lane, 64), b = r1cs_row_dot<F>(B, row, w, lane, 64), c = r1cs_row_dot<F>(C, row, w, lane, 64);
        for (int off = 32; off >= 1; off >>= 1) { a = a + shfl_down_fp(a, off); b = b + shfl_down_fp(b, off); c = c + shfl_down_fp(c, off); }
        if (lane == 0 && a * b != c) { count++; first = row < first ? row : first; }
    }
    r1cs_report(count, first, result);
}

// out[i] = sum_{k in column i} coeff[k] * L[row[k]] for the column-major (CSC) form of a matrix: col_ptr[n_cols + 1], row[nnz], coeff[nnz].
// Real circuits are badly skewed (the constant wire sits in a large share of the rows, most wires in one to three), so a workgroup takes
// 256 consecutive columns in two steps: a lane sums each column shorter than long_min on its own; the others are noted in LDS and then
// summed one after the other by the WHOLE workgroup (terms strided over the 256 lanes, wave shuffles, four partial sums through LDS).
// No atomics on field elements; field addition is exact, so neither the split nor the order of the noted columns changes a value.
template <class F>
__global__ void __launch_bounds__(256) k_qap_columns(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ row, const F* __restrict__ coeff, size_t n_cols,
                                                     const F* __restrict__ L, F* __restrict__ out, uint32_t long_min) {
    __shared__ uint32_t s_long[256], s_nlong, s_part[4][F::N];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t base = (size_t)blockIdx.x * 256; base < n_cols; base += (size_t)gridDim.x * 256) {     // uniform over the workgroup
        if (threadIdx.x == 0) s_nlong = 0;
        __syncthreads();
        const size_t c = base + threadIdx.x;
        if (c < n_cols) {
            const uint32_t b = col_ptr[c], e = col_ptr[c + 1];
            if (e - b >= long_min) s_long[atomicAdd(&s_nlong, 1u)] = threadIdx.x;
            else {
                F acc = F::zero();
                for (uint32_t k = b; k < e; k++) acc = acc + ld_fp(coeff + k) * ld_fp(L + row[k]);
                st_fp(out + c, acc);
            }
        }
        __syncthreads();
        const uint32_t n_long = s_nlong;
        if (n_long == 0) __syncthreads();                    // (the loop below ends on a barrier: nobody resets s_nlong before all have read it)
        for (uint32_t i = 0; i < n_long; i++) {
            const size_t lc = base + s_long[i];
            const uint32_t e = col_ptr[lc + 1];
            F acc = F::zero();
            for (uint32_t k = col_ptr[lc] + threadIdx.x; k < e; k += 256) acc = acc + ld_fp(coeff + k) * ld_fp(L + row[k]);
            for (int off = 32; off >= 1; off >>= 1) acc = acc + shfl_down_fp(acc, off);
            if (lane == 0) { _Pragma("unroll") for (int j = 0; j < F::N; j++) s_part[wave][j] = acc.v[j]; }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int wv = 1; wv < 4; wv++) { F t; _Pragma("unroll") for (int j = 0; j < F::N; j++) t.v[j] = s_part[wv][j]; acc = acc + t; }
                st_fp(out + lc, acc);
            }
            __syncthreads();
        }
    }
}

}  // namespace cg
