// Launch side of the scalar-field kernels (vec_kernels.hpp, ntt_kernels.hpp); instantiated per field in fr_inst_*.hip.
#pragma once
#include "launchers.hpp"
#include "ntt_kernels.hpp"
#include "vec_kernels.hpp"
#include "plonk_kernels.hpp"
#include "r1cs_kernels.hpp"
#include "plonk_setup_kernels.hpp"
#include "msm_sort_kernels.hpp"

namespace cg {

template <class Fr> int launch_vec_binary(hipStream_t st, int op, Fr* out, const Fr* a, const Fr* b, size_t n) {
    if (!n) return 0;
    if (op == 0) hipLaunchKernelGGL((k_vec_binary<Fr, 0>), dim3(grid_for(n)), dim3(256), 0, st, out, a, b, n);
    else if (op == 1) hipLaunchKernelGGL((k_vec_binary<Fr, 1>), dim3(grid_for(n)), dim3(256), 0, st, out, a, b, n);
    else hipLaunchKernelGGL((k_vec_binary<Fr, 2>), dim3(grid_for(n)), dim3(256), 0, st, out, a, b, n);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_rep3_mul_local(hipStream_t st, Fr* out, const Fr* aa, const Fr* ab, const Fr* ba, const Fr* bb, const Fr* mask, size_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_rep3_mul_local<Fr>), dim3(grid_for(n)), dim3(256), 0, st, out, aa, ab, ba, bb, mask, n);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_count_noncanonical(hipStream_t st, const Fr* v, size_t n, unsigned long long* n_bad) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_count_noncanonical<Fr>), dim3(grid_for(n)), dim3(256), 0, st, v, n, n_bad);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_distribute_powers(hipStream_t st, Fr* v, size_t n, const Fr* lo, const Fr* hi, int log_lo) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_distribute_powers<Fr>), dim3(grid_for(n)), dim3(256), 0, st, v, n, lo, hi, log_lo);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_affine(hipStream_t st, Fr* out, const Fr* a, size_t n, const Fr& c, const Fr& d) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_affine<Fr>), dim3(grid_for(n)), dim3(256), 0, st, out, a, n, c, d);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_lincomb(hipStream_t st, Fr* out, long long out_off, long long out_stride, size_t n, const LincombArgs<Fr>& a) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_lincomb<Fr>), dim3(grid_for(n)), dim3(256), 0, st, out, out_off, out_stride, n, a);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_shamir_share(hipStream_t st, const Fr* secrets, const Fr* coeffs, long long coeff_off, long long coeff_stride, size_t n, int degree,
                                            const ShareOuts<Fr>& o, long long out_off, long long out_stride) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_shamir_share<Fr>), dim3(grid_for(n)), dim3(256), 0, st, secrets, coeffs, coeff_off, coeff_stride, n, degree, o, out_off, out_stride);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_gather_idx(hipStream_t st, Fr* out, const Fr* in, const uint32_t* idx, size_t n, uint32_t base) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_gather_idx<Fr>), dim3(grid_for(n)), dim3(256), 0, st, out, in, idx, n, base);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_fill(hipStream_t st, Fr* v, size_t n, const Fr& value) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_fill<Fr>), dim3(grid_for(n)), dim3(256), 0, st, v, n, value);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_gather_strided(hipStream_t st, Fr* out, const Fr* in, size_t n, size_t offset, size_t stride) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_vec_gather_strided<Fr>), dim3(grid_for(n)), dim3(256), 0, st, out, in, n, offset, stride);
    HIPCHK(hipGetLastError());
    return 0;
}
// co-plonk (plonk_kernels.hpp): one launch per call, every share component in it
template <class Fr> int launch_plonk_additions(hipStream_t st, const uint32_t* order, size_t n, const uint32_t* ids, const Fr* coeffs, const Fr* pub, uint32_t n_inputs, int pc,
                                               Fr* ext_a, Fr* ext_b, size_t n_priv) {
    if (!n) return 0;
    hipLaunchKernelGGL((k_plonk_additions<Fr>), dim3(grid_for(n)), dim3(256), 0, st, order, n, ids, coeffs, pub, n_inputs, pc, ext_a, ext_b, n_priv);
    HIPCHK(hipGetLastError());
    return 0;
}
#define CG_PLONK_LAUNCH(NAME, KERNEL, ARGS)                                                                                  \
    template <class Fr> int NAME(hipStream_t st, const ARGS<Fr>& g, size_t n) {                                             \
        if (!n) return 0;                                                                                                   \
        hipLaunchKernelGGL((KERNEL<Fr>), dim3(grid_for(n)), dim3(256), 0, st, g, n);                                         \
        HIPCHK(hipGetLastError());                                                                                          \
        return 0;                                                                                                           \
    }
CG_PLONK_LAUNCH(launch_plonk_r2_factors, k_plonk_r2_factors, PlonkR2Args)
CG_PLONK_LAUNCH(launch_plonk_r3_blind, k_plonk_r3_blind, PlonkBlindArgs)
CG_PLONK_LAUNCH(launch_plonk_r3_perm, k_plonk_r3_perm, PlonkPermArgs)
CG_PLONK_LAUNCH(launch_plonk_r3_gate, k_plonk_r3_gate, PlonkGateArgs)
CG_PLONK_LAUNCH(launch_plonk_mul4_tail, k_plonk_mul4_tail, PlonkMul4Args)
CG_PLONK_LAUNCH(launch_plonk_r3_t, k_plonk_r3_t, PlonkTArgs)
CG_PLONK_LAUNCH(launch_plonk_r3_divide, k_plonk_r3_divide, PlonkDivArgs)
#undef CG_PLONK_LAUNCH
template <class Fr> int launch_plonk_gate_check(hipStream_t st, const PlonkCheckArgs<Fr>& g, size_t n, unsigned long long* result) {
    static const unsigned long long init[2] = {0ull, ~0ull};
    HIPCHK(hipMemcpyAsync(result, init, sizeof init, hipMemcpyHostToDevice, st));
    if (!n) return 0;
    hipLaunchKernelGGL((k_plonk_gate_check<Fr>), dim3(grid_for(n)), dim3(256), 0, st, g, n, result);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_vec_mismatch(hipStream_t st, const Fr* a, size_t a_stride, const Fr* b, size_t b_stride, size_t first, size_t n, unsigned long long* result) {
    static const unsigned long long init[2] = {0ull, ~0ull};
    HIPCHK(hipMemcpyAsync(result, init, sizeof init, hipMemcpyHostToDevice, st));
    if (first >= n) return 0;
    if (b) hipLaunchKernelGGL((k_vec_mismatch<Fr, false>), dim3(grid_for(n - first)), dim3(256), 0, st, a, a_stride, b, b_stride, first, n, result);
    else hipLaunchKernelGGL((k_vec_mismatch<Fr, true>), dim3(grid_for(n - first)), dim3(256), 0, st, a, a_stride, b, b_stride, first, n, result);
    HIPCHK(hipGetLastError());
    return 0;
}
// scratch: ceil(n / 2048) elements; op 0 = product, 1 = sum
template <class Fr, int OP> int launch_prefix_op(hipStream_t st, Fr* out, const Fr* in, size_t n, Fr* scratch) {
    const size_t tile = (size_t)256 * SCAN_ITEMS, ntiles = (n + tile - 1) / tile;
    hipLaunchKernelGGL((k_prefix_tiles<Fr, OP>), dim3((unsigned)ntiles), dim3(256), 0, st, out, in, n, scratch);
    if (ntiles > 1) {
        hipLaunchKernelGGL((k_prefix_totals<Fr, OP>), dim3(1), dim3(256), 0, st, scratch, ntiles);
        hipLaunchKernelGGL((k_prefix_fixup<Fr, OP>), dim3(grid_for(n)), dim3(256), 0, st, out, n, scratch);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_prefix_scan(hipStream_t st, int op, Fr* out, const Fr* in, size_t n, Fr* scratch) {
    if (!n) return 0;
    return op == 0 ? launch_prefix_op<Fr, 0>(st, out, in, n, scratch) : launch_prefix_op<Fr, 1>(st, out, in, n, scratch);
}
template <class Fr> int launch_vec_inverse(hipStream_t st, Fr* out, const Fr* in, size_t n) {
    if (!n) return 0;
    const size_t lanes = (n + INV_ITEMS - 1) / INV_ITEMS;
    hipLaunchKernelGGL((k_vec_inverse<Fr>), dim3((unsigned)((lanes + 127) / 128)), dim3(128), 0, st, out, in, n);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_spmv_csr(hipStream_t st, const uint32_t* row_ptr, const uint32_t* col, const Fr* coeff, size_t n_rows, const Fr* pub,
                                        uint32_t n_inputs, int party, const Fr* wit_a, const Fr* wit_b, Fr* out_a, Fr* out_b) {
    if (!n_rows) return 0;
    if (n_rows <= ((size_t)1 << 13)) hipLaunchKernelGGL((k_spmv_csr_wave<Fr>), dim3(grid_for(n_rows * 64)), dim3(256), 0, st, row_ptr, col, coeff, n_rows, pub, n_inputs, party, wit_a, wit_b, out_a, out_b);   // a wave per row
    else hipLaunchKernelGGL((k_spmv_csr<Fr>), dim3(grid_for(n_rows)), dim3(256), 0, st, row_ptr, col, coeff, n_rows, pub, n_inputs, party, wit_a, wit_b, out_a, out_b);
    HIPCHK(hipGetLastError());
    return 0;
}
// witness check: a wave per row triple when the rows cannot fill the chip with a lane each (as launch_spmv_csr) or when the mean row is long
// (>= 32 terms per matrix: a lane would walk them one by one while its 63 neighbours wait for the longest row of the wave)
template <class Fr> int launch_r1cs_check(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, size_t nnz_total, int form, const Fr* w,
                                          unsigned long long* result) {
    static const unsigned long long init[2] = {0ull, ~0ull};
    HIPCHK(hipMemcpyAsync(result, init, sizeof init, hipMemcpyHostToDevice, st));
    if (!n_rows) return 0;
    const bool wave = form == 2 || (form == 0 && (n_rows <= ((size_t)1 << 13) || nnz_total / n_rows >= 96));
    if (wave) hipLaunchKernelGGL((k_r1cs_check_wave<Fr>), dim3(grid_for(n_rows * 64)), dim3(256), 0, st, A, B, C, n_rows, w, result);
    else hipLaunchKernelGGL((k_r1cs_check<Fr>), dim3(grid_for(n_rows)), dim3(256), 0, st, A, B, C, n_rows, w, result);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_qap_columns(hipStream_t st, const uint32_t* col_ptr, const uint32_t* row, const Fr* coeff, size_t n_cols, const Fr* L, Fr* out, uint32_t long_min) {
    if (!n_cols) return 0;
    hipLaunchKernelGGL((k_qap_columns<Fr>), dim3(grid_for(n_cols)), dim3(256), 0, st, col_ptr, row, coeff, n_cols, L, out, long_min ? long_min : QAP_LONG_COLUMN);
    HIPCHK(hipGetLastError());
    return 0;
}
// Plonk setup: the addition count of every row and its exclusive scan (k_scan_*: tiles of SCAN_TILE counters), then the gates
template <class Fr> int launch_plonk_gate_count(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, uint32_t* counts, uint32_t* offsets, uint32_t* tile_sums) {
    const size_t total = n_rows + 1, ntiles = (total + SCAN_TILE - 1) / SCAN_TILE;
    HIPCHK(hipMemsetAsync(counts + n_rows, 0, 4, st));
    if (n_rows) hipLaunchKernelGGL((k_plonk_gate_count<Fr>), dim3(grid_for(n_rows)), dim3(256), 0, st, A, B, C, n_rows, counts);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, total, 0xffffffffu);
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, st, tile_sums, tile_sums, ntiles);
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, offsets, total, 0xffffffffu);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_plonk_gate_emit(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, uint32_t n_wires, uint32_t n_public,
                                               const uint32_t* counts, const uint32_t* offsets, size_t n_constraints, size_t n, const PlonkGateOut& o) {
    for (int i = 0; i < 5; i++) if (n > n_constraints) HIPCHK(hipMemsetAsync((Fr*)o.q[i] + n_constraints, 0, (n - n_constraints) * sizeof(Fr), st));
    if (n_rows + n_public) hipLaunchKernelGGL((k_plonk_gate_emit<Fr>), dim3(grid_for(n_rows + n_public)), dim3(256), 0, st, A, B, C, n_rows, n_wires, n_public, counts, offsets, o);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_plonk_sigma_labels(hipStream_t st, const uint32_t* prev, const Fr* wpow, int log_n, const Fr& k1, const Fr& k2, Fr* sigma) {
    hipLaunchKernelGGL((k_plonk_sigma_labels<Fr>), dim3(grid_for((size_t)3 << log_n)), dim3(256), 0, st, prev, wpow, log_n, k1, k2, sigma);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_build_twiddles_lazy(hipStream_t st, void* tw, size_t m, int log_m, const Fr* lo, const Fr* hi, int log_lo, const Fr& c32) {
    if (m > 1) hipLaunchKernelGGL((k_build_twiddles_lazy<Fr>), dim3(grid_for(m / 2)), dim3(256), 0, st, tw, m / 2, log_m, lo, hi, log_lo, c32);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_ntt_ct_pass(hipStream_t st, bool first, NttVecs src, NttVecs dst, int nvec, size_t n, int log_m, int s0, int k, int t, const void* tw) {
    static PerDeviceOnce attr_set;
    if (attr_set.pending()) {
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_ct_pass<Fr, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_ct_pass<Fr, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        attr_set.mark();
    }
    const int E = 1 << (k + t);
    if (first) hipLaunchKernelGGL((k_ntt_ct_pass<Fr, true>), dim3((unsigned)(n / E), nvec), dim3(NTT_THREADS), (size_t)E * 36, st, src, dst, log_m, s0, k, t, tw);
    else hipLaunchKernelGGL((k_ntt_ct_pass<Fr, false>), dim3((unsigned)(n / E), nvec), dim3(NTT_THREADS), (size_t)E * 36, st, src, dst, log_m, s0, k, t, tw);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_build_twiddles_lazy_natural(hipStream_t st, void* tw, size_t m, const Fr* lo, const Fr* hi, int log_lo, const Fr& c32) {
    if (m > 1) hipLaunchKernelGGL((k_build_twiddles_lazy_natural<Fr>), dim3(grid_for(m / 2)), dim3(256), 0, st, tw, m / 2, lo, hi, log_lo, c32);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_ntt_dit_pass(hipStream_t st, bool first, bool last, NttVecs out, NttVecs tmp, int nvec, size_t n, int log_m, int s0, int k, int t, const void* tw,
                                            const Fr* c_lo, const Fr* c_hi, int log_lo, const Fr& c32) {
    static PerDeviceOnce attr_set;
    if (attr_set.pending()) {
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_dit_pass<Fr, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_dit_pass<Fr, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_dit_pass<Fr, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        HIPCHK(hipFuncSetAttribute((const void*)k_ntt_dit_pass<Fr, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 36 << NTT_TILE_LOG));
        attr_set.mark();
    }
    const int E = 1 << (k + t);
    const dim3 grid((unsigned)(n / E), nvec); const size_t lds = (size_t)E * 36;
    if (first && last) hipLaunchKernelGGL((k_ntt_dit_pass<Fr, true, true>), grid, dim3(NTT_THREADS), lds, st, out, tmp, log_m, s0, k, t, tw, c_lo, c_hi, log_lo, c32);
    else if (first) hipLaunchKernelGGL((k_ntt_dit_pass<Fr, true, false>), grid, dim3(NTT_THREADS), lds, st, out, tmp, log_m, s0, k, t, tw, c_lo, c_hi, log_lo, c32);
    else if (last) hipLaunchKernelGGL((k_ntt_dit_pass<Fr, false, true>), grid, dim3(NTT_THREADS), lds, st, out, tmp, log_m, s0, k, t, tw, c_lo, c_hi, log_lo, c32);
    else hipLaunchKernelGGL((k_ntt_dit_pass<Fr, false, false>), grid, dim3(NTT_THREADS), lds, st, out, tmp, log_m, s0, k, t, tw, c_lo, c_hi, log_lo, c32);
    HIPCHK(hipGetLastError());
    return 0;
}
template <class Fr> int launch_bitrev_finish_lazy(hipStream_t st, NttVecs dst, NttVecs src, int nvec, size_t n, int log_m, const Fr* scale, const Fr* c_lo, const Fr* c_hi, int log_lo) {
    if (log_m >= 2 * BITREV_B_LAZY)
        hipLaunchKernelGGL((k_bitrev_finish_lazy<Fr>), dim3((unsigned)(n >> (2 * BITREV_B_LAZY)), nvec), dim3(256), 0, st, dst, src, log_m, scale, c_lo, c_hi, log_lo);
    else
        hipLaunchKernelGGL((k_bitrev_finish_lazy_small<Fr>), dim3(grid_for(n), nvec), dim3(256), 0, st, dst, src, log_m, scale, c_lo, c_hi, log_lo);
    HIPCHK(hipGetLastError());
    return 0;
}

// scalar-dependent half of the MSM: digits, histogram, scan, scatter.  Scratch layout and size: msm_sort_scratch_bytes (launchers.hpp).
// evs (optional, 2 events) bracket the stage.
// any_size: a forced partition sort (cg_msm_schedule_dev) keeps the structural limits and waives the size from which the partition pays
inline bool msm_sort_use_partition(size_t n, int c, int nwin, int shared, bool any_size = false) {
    const size_t nbuckets = (size_t)(shared ? 1 : nwin) << (c - 1);
    const size_t nregions = (nbuckets + ((size_t)1 << PART_REGION_LOG) - 1) >> PART_REGION_LOG;
    return (any_size || (size_t)nwin * n >= ((size_t)1 << 21)) && nregions >= 8 && nregions <= PART_MAX_REGIONS;
}
template <class Fr> int msm_sort_launch(hipStream_t st, const Fr* d_scalars, size_t n, int c, int nwin, int shared, char* scratch, size_t scratch_bytes, MsmSortPtrs* out, hipEvent_t* evs,
                                        int force) {
    if (force != 0 && force != CG_MSM_PATH_GENERAL && force != CG_MSM_PATH_SMALL && force != CG_MSM_PATH_PARTITION) return fail(CG_ERR_ARG, "msm_sort_launch: not a path of the dense schedule");
    const size_t nbuckets = (size_t)(shared ? 1 : nwin) << (c - 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = scratch + off; off += align_up(bytes); return p; };
    int32_t* digits = (int32_t*)take((size_t)nwin * n * 4);
    uint32_t* sorted = (uint32_t*)take((size_t)nwin * n * 4);
    uint32_t* counts = (uint32_t*)take(nbuckets * 4);
    uint32_t* cursors = (uint32_t*)take(nbuckets * 4);
    uint32_t* offsets = (uint32_t*)take(nbuckets * 4);
    const size_t ntiles = (nbuckets + SCAN_TILE - 1) / SCAN_TILE;
    uint32_t* tile_sums = (uint32_t*)take(ntiles * 4);
    const size_t entries = (size_t)nwin * n;
    const bool no_small = !global_option(CG_GOPT_SORT_SMALL);                            // cg_set_option: the general six-launch schedule for every size
    const bool small_fits = shared && nbuckets <= SORT_SMALL_MAX_BUCKETS && entries <= SORT_SMALL_MAX_ENTRIES && n <= (1u << 24);
    if (force == CG_MSM_PATH_SMALL && (!small_fits || no_small))
        return fail(CG_ERR_ARG, "the one-workgroup schedule takes one shared bucket set of at most 2^13 buckets and at most 2^15 entries, with CG_GOPT_SORT_SMALL on");
    if (force == CG_MSM_PATH_PARTITION && !msm_sort_use_partition(n, c, nwin, shared, true)) return fail(CG_ERR_ARG, "the partition sort takes 8 to 4096 regions of 512 buckets");
    // (the kernel asks for up to 68 KiB of dynamic LDS: a device whose workgroups cannot have that — the attribute call fails — takes the general
    // schedule below instead of failing the MSM: ADVICE r5)
    static PerDeviceOnce attr_small; static std::atomic<bool> small_unavailable{false};
    const bool may_small = shared && !no_small && (force == 0 || force == CG_MSM_PATH_SMALL);
    if (may_small && !small_unavailable.load(std::memory_order_relaxed) && attr_small.pending()) {
        if (hipFuncSetAttribute((const void*)k_msm_sort_small<Fr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((2 * SORT_SMALL_MAX_BUCKETS + 1024) * 4)) == hipSuccess) attr_small.mark();
        else { (void)hipGetLastError(); small_unavailable.store(true); }
    }
    const bool small = may_small && !small_unavailable.load(std::memory_order_relaxed) && small_fits;
    if (force == CG_MSM_PATH_SMALL && !small) return fail(CG_ERR_HIP, "the one-workgroup schedule is not available on this device");
    const bool partition = !small && (force == CG_MSM_PATH_PARTITION || (force == 0 && msm_sort_use_partition(n, c, nwin, shared)));
    uint64_t* items = nullptr; uint32_t* region_total = nullptr; uint32_t* region_cursor = nullptr; uint32_t* total_items = nullptr;
    if (partition) {
        items = (uint64_t*)take(entries * 8);
        region_total = (uint32_t*)take(PART_MAX_REGIONS * 4);
        region_cursor = (uint32_t*)take(PART_MAX_REGIONS * 4);
        total_items = (uint32_t*)take(4);
    }
    if (off > scratch_bytes) return fail(CG_ERR_ARG, "msm_sort_launch: the layout of the schedule exceeds its scratch");   // the caller sized it with msm_sort_scratch_bytes
    if (evs) HIPCHK(hipEventRecord(evs[0], st));
    if (small) {   // small vectors: one launch
        const size_t lds = (2 * nbuckets + 1024) * 4;
        hipLaunchKernelGGL((k_msm_sort_small<Fr>), dim3(1), dim3(1024), lds, st, d_scalars, (uint32_t)n, c, nwin, counts, offsets, sorted);
        if (evs) HIPCHK(hipEventRecord(evs[1], st));
        HIPCHK(hipGetLastError());
        out->sorted = sorted; out->offsets = offsets; out->counts = counts; out->cap = 0; out->overflow = nullptr; out->path = CG_MSM_PATH_SMALL;
        return 0;
    }
    HIPCHK(hipMemsetAsync(counts, 0, align_up(nbuckets * 4) * 2, st));   // counts + cursors are adjacent
    if (partition) {
        const size_t ptiles = (entries + PART_TILE - 1) / PART_TILE;
        const uint32_t nregions = (uint32_t)((nbuckets + ((size_t)1 << PART_REGION_LOG) - 1) >> PART_REGION_LOG);
        const unsigned itiles = (unsigned)(((entries + ITEM_TILE - 1) / ITEM_TILE + 7) / 8 * 8);   // a multiple of 8: xcd_tile() deals the tiles to the XCDs
        HIPCHK(hipMemsetAsync(region_total, 0, nregions * 4, st));
        hipLaunchKernelGGL((k_msm_digits_only<Fr>), dim3(grid_for(n)), dim3(256), 0, st, d_scalars, n, c, nwin, digits);
        hipLaunchKernelGGL(k_part_hist, dim3((unsigned)ptiles), dim3(256), nregions * 4, st, digits, n, c, nwin, shared, nregions, region_total);
        hipLaunchKernelGGL(k_part_region_scan, dim3(1), dim3(1024), 0, st, region_total, nregions, region_cursor, total_items);
        const bool staged = global_option(CG_GOPT_SORT_STAGING) != 0;              // cg_set_option
        if (staged && nregions <= STAGE_MAX_REGIONS) {
            static PerDeviceOnce attr_set;
            if (attr_set.pending()) {
                HIPCHK(hipFuncSetAttribute((const void*)k_part_scatter_staged, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_staged_lds(STAGE_MAX_REGIONS)));
                HIPCHK(hipFuncSetAttribute((const void*)k_items_scatter_staged, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ITEMS_STAGED_LDS));
                attr_set.mark();
            }
            hipLaunchKernelGGL(k_part_scatter_staged, dim3((unsigned)ptiles), dim3(STAGE_THREADS), part_staged_lds(nregions), st, digits, n, c, nwin, shared, nregions, region_cursor, items);
        } else
        hipLaunchKernelGGL(k_part_scatter, dim3((unsigned)ptiles), dim3(256), nregions * 4, st, digits, n, c, nwin, shared, nregions, region_cursor, items);
        hipLaunchKernelGGL(k_items_hist, dim3(itiles), dim3(256), 0, st, items, total_items, counts);
        hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, nbuckets, 0xffffffffu);
        hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, st, tile_sums, tile_sums, ntiles);
        hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, offsets, nbuckets, 0xffffffffu);
        if (staged && nregions <= STAGE_MAX_REGIONS) hipLaunchKernelGGL(k_items_scatter_staged, dim3(itiles), dim3(STAGE_THREADS), ITEMS_STAGED_LDS, st, items, total_items, offsets, cursors, sorted);
        else hipLaunchKernelGGL(k_items_scatter, dim3(itiles), dim3(256), 0, st, items, total_items, offsets, cursors, sorted);
        if (evs) HIPCHK(hipEventRecord(evs[1], st));
        HIPCHK(hipGetLastError());
        out->sorted = sorted; out->offsets = offsets; out->counts = counts; out->cap = 0; out->overflow = nullptr;
        out->path = staged && nregions <= STAGE_MAX_REGIONS ? CG_MSM_PATH_PARTITION : CG_MSM_PATH_PARTITION_UNSTAGED;
        return 0;
    }
    hipLaunchKernelGGL((k_msm_digits<Fr>), dim3(grid_for(n)), dim3(256), 0, st, d_scalars, n, c, nwin, shared, digits, counts);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, nbuckets, 0xffffffffu);
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, st, tile_sums, tile_sums, ntiles);
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, offsets, nbuckets, 0xffffffffu);
    hipLaunchKernelGGL(k_msm_scatter, dim3(grid_for((size_t)nwin * n)), dim3(256), 0, st, digits, n, c, nwin, shared, offsets, cursors, sorted);
    if (evs) HIPCHK(hipEventRecord(evs[1], st));
    HIPCHK(hipGetLastError());
    out->sorted = sorted; out->offsets = offsets; out->counts = counts; out->cap = 0; out->overflow = nullptr; out->path = CG_MSM_PATH_GENERAL;
    return 0;
}
// optimistic one-pass variant (scratch: msm_sort_direct_scratch_bytes)
template <class Fr> int msm_sort_direct_launch(hipStream_t st, const Fr* d_scalars, size_t n, int c, int nwin, int shared, uint32_t cap, char* scratch, size_t scratch_bytes,
                                               MsmSortPtrs* out, hipEvent_t* evs, int force) {
    if (force != 0 && force != CG_MSM_PATH_DIRECT) return fail(CG_ERR_ARG, "msm_sort_direct_launch: the one-pass scatter is the only path here");
    if (cap < 1) return fail(CG_ERR_ARG, "the one-pass scatter takes a capacity of at least one entry per bucket");
    const size_t nbuckets = (size_t)(shared ? 1 : nwin) << (c - 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = scratch + off; off += align_up(bytes); return p; };
    uint32_t* sorted = (uint32_t*)take(nbuckets * cap * 4);
    uint32_t* counts = (uint32_t*)take(nbuckets * 4);
    uint32_t* offsets = (uint32_t*)take(nbuckets * 4);
    const size_t ntiles = (nbuckets + SCAN_TILE - 1) / SCAN_TILE;
    uint32_t* tile_sums = (uint32_t*)take(ntiles * 4);
    uint32_t* overflow = (uint32_t*)take(4);
    if (off > scratch_bytes) return fail(CG_ERR_ARG, "msm_sort_direct_launch: the layout of the schedule exceeds its scratch");   // the caller sized it with msm_sort_direct_scratch_bytes
    if (evs) HIPCHK(hipEventRecord(evs[0], st));
    HIPCHK(hipMemsetAsync(counts, 0, nbuckets * 4, st));
    HIPCHK(hipMemsetAsync(overflow, 0, 4, st));
    hipLaunchKernelGGL((k_msm_scatter_direct<Fr>), dim3(grid_for(n)), dim3(256), 0, st, d_scalars, n, c, nwin, shared, cap, counts, sorted, overflow);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, nbuckets, cap);
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, st, tile_sums, tile_sums, ntiles);
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, st, counts, tile_sums, offsets, nbuckets, cap);
    if (evs) HIPCHK(hipEventRecord(evs[1], st));
    HIPCHK(hipGetLastError());
    out->sorted = sorted; out->offsets = offsets; out->counts = counts; out->cap = cap; out->overflow = overflow; out->path = CG_MSM_PATH_DIRECT;
    return 0;
}

}  // namespace cg

// explicit instantiations, typed by the declarations of launchers.hpp: a definition above that differs from its declaration is a
// second overload, and the instantiation below then fails to compile
#define CG_INSTANTIATE_FR(Fr)                                                                                              \
    namespace cg {                                                                                                         \
    template decltype(launch_vec_binary<Fr>) launch_vec_binary<Fr>;                                                        \
    template decltype(launch_rep3_mul_local<Fr>) launch_rep3_mul_local<Fr>;                                                \
    template decltype(launch_distribute_powers<Fr>) launch_distribute_powers<Fr>;                                          \
    template decltype(launch_vec_count_noncanonical<Fr>) launch_vec_count_noncanonical<Fr>;                                \
    template decltype(launch_vec_fill<Fr>) launch_vec_fill<Fr>;                                                            \
    template decltype(launch_vec_gather_idx<Fr>) launch_vec_gather_idx<Fr>;                                                \
    template decltype(launch_vec_affine<Fr>) launch_vec_affine<Fr>;                                                        \
    template decltype(launch_vec_gather_strided<Fr>) launch_vec_gather_strided<Fr>;                                        \
    template decltype(launch_vec_lincomb<Fr>) launch_vec_lincomb<Fr>;                                                      \
    template decltype(launch_shamir_share<Fr>) launch_shamir_share<Fr>;                                                    \
    template decltype(launch_plonk_r2_factors<Fr>) launch_plonk_r2_factors<Fr>;                                            \
    template decltype(launch_prefix_scan<Fr>) launch_prefix_scan<Fr>;                                                      \
    template decltype(launch_vec_inverse<Fr>) launch_vec_inverse<Fr>;                                                      \
    template decltype(launch_plonk_additions<Fr>) launch_plonk_additions<Fr>;                                              \
    template decltype(launch_plonk_r3_blind<Fr>) launch_plonk_r3_blind<Fr>;                                                \
    template decltype(launch_plonk_r3_perm<Fr>) launch_plonk_r3_perm<Fr>;                                                  \
    template decltype(launch_plonk_r3_gate<Fr>) launch_plonk_r3_gate<Fr>;                                                  \
    template decltype(launch_plonk_mul4_tail<Fr>) launch_plonk_mul4_tail<Fr>;                                              \
    template decltype(launch_plonk_r3_t<Fr>) launch_plonk_r3_t<Fr>;                                                        \
    template decltype(launch_plonk_r3_divide<Fr>) launch_plonk_r3_divide<Fr>;                                              \
    template decltype(launch_plonk_gate_check<Fr>) launch_plonk_gate_check<Fr>;                                            \
    template decltype(launch_vec_mismatch<Fr>) launch_vec_mismatch<Fr>;                                                    \
    template decltype(launch_spmv_csr<Fr>) launch_spmv_csr<Fr>;                                                            \
    template decltype(launch_r1cs_check<Fr>) launch_r1cs_check<Fr>;                                                        \
    template decltype(launch_qap_columns<Fr>) launch_qap_columns<Fr>;                                                      \
    template decltype(launch_plonk_gate_count<Fr>) launch_plonk_gate_count<Fr>;                                            \
    template decltype(launch_plonk_gate_emit<Fr>) launch_plonk_gate_emit<Fr>;                                              \
    template decltype(launch_plonk_sigma_labels<Fr>) launch_plonk_sigma_labels<Fr>;                                        \
    template decltype(launch_build_twiddles_lazy<Fr>) launch_build_twiddles_lazy<Fr>;                                      \
    template decltype(launch_ntt_ct_pass<Fr>) launch_ntt_ct_pass<Fr>;                                                      \
    template decltype(launch_build_twiddles_lazy_natural<Fr>) launch_build_twiddles_lazy_natural<Fr>;                      \
    template decltype(launch_ntt_dit_pass<Fr>) launch_ntt_dit_pass<Fr>;                                                    \
    template decltype(launch_bitrev_finish_lazy<Fr>) launch_bitrev_finish_lazy<Fr>;                                        \
    template decltype(msm_sort_launch<Fr>) msm_sort_launch<Fr>;                                                            \
    template decltype(msm_sort_direct_launch<Fr>) msm_sort_direct_launch<Fr>;                                              \
    }
