// What the host side of the C ABI (capi*.hip) and the launchers (fr_impl.hpp, msm_impl.hpp; explicitly instantiated in fr_inst_*.hip /
// msm_inst_*.hip) share: the declarations of every launcher, the schedule record of the MSM sort and the sizes of its scratch.  No kernels:
// the translation units of the C ABI include this header and instantiate nothing.  The launchers include it too and instantiate through
// the declared type (`template decltype(f<Fr>) f<Fr>;`), so a definition whose signature drifts from its declaration is a second
// overload and fails to compile, instead of leaving an unresolved symbol for the loader to find.
#pragma once
#include "common.hpp"

namespace cg {

template <class F> struct Affine;          // curve.hpp
template <class F> struct XYZZ;
template <class F> struct FastSubgroup;    // subgroup.hpp
struct NttVecs;                            // ntt_kernels.hpp
template <class F> struct PlonkR2Args;     // plonk_kernels.hpp
template <class F> struct PlonkBlindArgs;
template <class F> struct PlonkPermArgs;
template <class F> struct PlonkGateArgs;
template <class F> struct PlonkMul4Args;
template <class F> struct PlonkTArgs;
template <class F> struct PlonkDivArgs;
template <class F> struct PlonkCheckArgs;

// ---- scalar side of the MSM (msm_sort_kernels.hpp, fr_impl.hpp): digits, histogram, scan, scatter
constexpr int SCAN_TILE = 2048;         // k_scan_*: counters per workgroup (256 lanes x 8)
constexpr int PART_TILE = 16384;        // k_part_*: consecutive (window, scalar) entries per workgroup
constexpr int PART_REGION_LOG = 9;      // 512 buckets per region
constexpr int PART_MAX_REGIONS = 4096;  // LDS histogram limit
struct MsmSortPtrs { const uint32_t* sorted; const uint32_t* offsets; const uint32_t* counts; uint32_t cap; const uint32_t* overflow; int path; };   // cap = 0: dense list; path: CG_MSM_PATH_* that ran
// scratch of msm_sort_launch: digits | sorted | counts | cursors | offsets | tile sums, and on the partition path items | region totals |
// region cursors | item count.  Sized for the per-window bucket sets (the shared-set mode needs less).
inline size_t msm_sort_scratch_bytes(size_t n, int c, int nwin) {
    const size_t nbuckets = (size_t)nwin << (c - 1);
    const size_t entries = (size_t)nwin * n;
    return 2 * align_up(entries * 4) + 3 * align_up(nbuckets * 4) + align_up(((nbuckets + SCAN_TILE - 1) / SCAN_TILE) * 4) +
           align_up(entries * 8) + 2 * align_up(PART_MAX_REGIONS * 4) + 256;
}
// scratch of msm_sort_direct_launch (optimistic one-pass variant): sorted[nbuckets * cap] | counts | offsets | tile sums | overflow flag
inline size_t msm_sort_direct_scratch_bytes(size_t n, int c, int nwin, int shared, uint32_t cap) {
    const size_t nbuckets = (size_t)(shared ? 1 : nwin) << (c - 1);
    return align_up(nbuckets * cap * 4) + 2 * align_up(nbuckets * 4) + align_up(((nbuckets + SCAN_TILE - 1) / SCAN_TILE) * 4) + 256;
}
// scratch_bytes: what the caller allocated; a layout that does not fit is an error, before anything is launched.  force: 0 = the launcher's
// own choice of path, CG_MSM_PATH_GENERAL / _SMALL / _PARTITION / _DIRECT = that path or an error if its structural limits do not hold
// (cg_msm_schedule_dev; only the partition sort's performance threshold of 2^21 entries is waived).
template <class Fr> int msm_sort_launch(hipStream_t st, const Fr* d_scalars, size_t n, int c, int nwin, int shared, char* scratch, size_t scratch_bytes, MsmSortPtrs* out, hipEvent_t* evs,
                                        int force = 0);
template <class Fr> int msm_sort_direct_launch(hipStream_t st, const Fr* d_scalars, size_t n, int c, int nwin, int shared, uint32_t cap, char* scratch, size_t scratch_bytes,
                                               MsmSortPtrs* out, hipEvent_t* evs, int force = 0);

// ---- group side of the MSM and the point kernels (msm_impl.hpp)
// The geometry is computed ONCE per call (msm_geom_of: what an MSM call over n points uses; msm_geom_with_chunks: an explicit chunking) and handed
// to everything that sizes scratch or launches from it.
template <class F> MsmGeom msm_geom_of(size_t n, int c, int nwin, bool shared, uint32_t chunk_request);
template <class F> int msm_accumulate_batch(hipStream_t st, const MsmAccSet* sets, int nsets, const MsmGeom& g, uint32_t cap, hipEvent_t* evs, bool g2_slices);
template <class F> int msm_reduce_batch(hipStream_t st2, const MsmRedSet* sets, int nsets, const MsmGeom& g, uint32_t cap, hipEvent_t* ev_merged, int n_merged, hipEvent_t* evs);
template <class F> size_t msm_acc_scratch_bytes(const MsmGeom& g);
// cg_msm_stages_dev: the arrays of a scratch slot, the slice of a sliced accumulation, and limb-form points brought to packed affine records
// (msm_debug_kernels.hpp: state[i] = 0 point, 1 infinity, 2 = the slot still holds the 0xFF bytes it was filled with; such a slot's record is left alone)
struct MsmScratchView { void* buckets; void* cont; uint32_t* cont_bucket; size_t bucket_bytes; };
template <class F> MsmScratchView msm_acc_scratch_view(char* scratch, const MsmGeom& g);
template <class F> uint32_t msm_acc_slice_groups();
template <class F> int msm_debug_to_affine(hipStream_t st, const void* d_limb_points, size_t n, Affine<F>* d_out, uint32_t* d_state);
template <class F> int precompute_window_launch(hipStream_t st, const Affine<F>* d_src, Affine<F>* d_dst, size_t n, int c);
template <class F> int check_on_curve_launch(hipStream_t st, const Affine<F>* d_pts, size_t n, const F& b, unsigned long long* d_counters);
template <class F, class Fr> int check_subgroup_launch(hipStream_t st, const Affine<F>* d_pts, size_t n, unsigned long long* d_counters);
template <class F> int check_subgroup_fast_launch(hipStream_t st, const Affine<F>* d_pts, size_t n, const FastSubgroup<F>& c, unsigned long long* d_counters);
template <class F> int pack_bases_launch(hipStream_t st, const uint8_t* d_raw, size_t n, size_t stride, long inf_off, Affine<F>* d_dst);
template <class F> int gather_points_launch(hipStream_t st, Affine<F>* d_dst, const Affine<F>* d_src, const uint32_t* d_idx, size_t n);
template <class F> int synth_points_launch(hipStream_t st, const XYZZ<F>* d_lo, const XYZZ<F>* d_hi, int log_t, size_t n, Affine<F>* d_out);
template <class F, class Fr> int fixed_base_mul_launch(hipStream_t st, const Affine<F>& g, const Fr* d_scalars, size_t n, Affine<F>* d_tab, Affine<F>* d_out);

// ---- scalar-field vectors, co-plonk and the transforms (fr_impl.hpp)
template <class Fr> int launch_vec_binary(hipStream_t st, int op, Fr* out, const Fr* a, const Fr* b, size_t n);
template <class Fr> int launch_rep3_mul_local(hipStream_t st, Fr* out, const Fr* aa, const Fr* ab, const Fr* ba, const Fr* bb, const Fr* mask, size_t n);
template <class Fr> int launch_vec_count_noncanonical(hipStream_t st, const Fr* v, size_t n, unsigned long long* n_bad);
template <class Fr> int launch_distribute_powers(hipStream_t st, Fr* v, size_t n, const Fr* lo, const Fr* hi, int log_lo);
template <class Fr> int launch_vec_affine(hipStream_t st, Fr* out, const Fr* a, size_t n, const Fr& c, const Fr& d);
template <class Fr> int launch_vec_lincomb(hipStream_t st, Fr* out, long long out_off, long long out_stride, size_t n, const LincombArgs<Fr>& a);
template <class Fr> int launch_shamir_share(hipStream_t st, const Fr* secrets, const Fr* coeffs, long long coeff_off, long long coeff_stride, size_t n, int degree,
                                            const ShareOuts<Fr>& o, long long out_off, long long out_stride);
template <class Fr> int launch_vec_gather_idx(hipStream_t st, Fr* out, const Fr* in, const uint32_t* idx, size_t n, uint32_t base);
template <class Fr> int launch_vec_fill(hipStream_t st, Fr* v, size_t n, const Fr& value);
template <class Fr> int launch_vec_gather_strided(hipStream_t st, Fr* out, const Fr* in, size_t n, size_t offset, size_t stride);
template <class Fr> int launch_prefix_scan(hipStream_t st, int op, Fr* out, const Fr* in, size_t n, Fr* scratch);
template <class Fr> int launch_vec_inverse(hipStream_t st, Fr* out, const Fr* in, size_t n);
template <class Fr> int launch_spmv_csr(hipStream_t st, const uint32_t* row_ptr, const uint32_t* col, const Fr* coeff, size_t n_rows, const Fr* pub,
                                        uint32_t n_inputs, int party, const Fr* wit_a, const Fr* wit_b, Fr* out_a, Fr* out_b);
// r1cs_kernels.hpp.  form: 0 = chosen from the row count and the mean row length (nnz_total terms over the three matrices, 0 = unknown),
// 1 = a lane per row triple, 2 = a wave per row triple.  result: count, smallest failing row (both set by the launcher first).
struct R1csMat { const uint32_t* row_ptr; const uint32_t* col; const void* coeff; };   // CSR, coefficients in Montgomery form
constexpr uint32_t QAP_LONG_COLUMN = 64;   // k_qap_columns: entries from which the workgroup, not one lane, sums a column
template <class Fr> int launch_r1cs_check(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, size_t nnz_total, int form, const Fr* w,
                                          unsigned long long* result);
template <class Fr> int launch_qap_columns(hipStream_t st, const uint32_t* col_ptr, const uint32_t* row, const Fr* coeff, size_t n_cols, const Fr* L, Fr* out, uint32_t long_min);
// plonk_setup_kernels.hpp: the gate compiler of the Plonk setup over the canonical CSR (wires ascending, merged, no zero coefficient).
// count: counts[n_rows + 1] (the last entry 0) and their exclusive scan offsets[n_rows + 1] (the last entry = the additions of the circuit);
// tile_sums: ceil((n_rows + 1) / SCAN_TILE) counters of scratch.  emit: the gates, public-input rows first; q rows from n_constraints to
// n are zeroed.  sigma: 3n labels from the previous positions.
struct PlonkGateOut {
    uint32_t* map[3];        // n_constraints each
    void* q[5];              // qm, ql, qr, qo, qc: n rows each, Montgomery
    uint32_t* add_ids;       // 2 per addition
    void* add_f;             // 2 per addition, Montgomery
};
template <class Fr> int launch_plonk_gate_count(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, uint32_t* counts, uint32_t* offsets, uint32_t* tile_sums);
template <class Fr> int launch_plonk_gate_emit(hipStream_t st, const R1csMat& A, const R1csMat& B, const R1csMat& C, size_t n_rows, uint32_t n_wires, uint32_t n_public,
                                               const uint32_t* counts, const uint32_t* offsets, size_t n_constraints, size_t n, const PlonkGateOut& o);
template <class Fr> int launch_plonk_sigma_labels(hipStream_t st, const uint32_t* prev, const Fr* wpow, int log_n, const Fr& k1, const Fr& k2, Fr* sigma);
template <class Fr> int launch_plonk_additions(hipStream_t st, const uint32_t* order, size_t n, const uint32_t* ids, const Fr* coeffs, const Fr* pub, uint32_t n_inputs, int pc,
                                               Fr* ext_a, Fr* ext_b, size_t n_priv);
template <class Fr> int launch_plonk_r2_factors(hipStream_t st, const PlonkR2Args<Fr>& g, size_t n);
template <class Fr> int launch_plonk_r3_blind(hipStream_t st, const PlonkBlindArgs<Fr>& g, size_t n);
template <class Fr> int launch_plonk_r3_perm(hipStream_t st, const PlonkPermArgs<Fr>& g, size_t n);
template <class Fr> int launch_plonk_r3_gate(hipStream_t st, const PlonkGateArgs<Fr>& g, size_t n);
template <class Fr> int launch_plonk_mul4_tail(hipStream_t st, const PlonkMul4Args<Fr>& g, size_t n);
template <class Fr> int launch_plonk_r3_t(hipStream_t st, const PlonkTArgs<Fr>& g, size_t n);
template <class Fr> int launch_plonk_r3_divide(hipStream_t st, const PlonkDivArgs<Fr>& g, size_t n);
// result (both): count, smallest failing row / differing position (set by the launcher first).  vec_mismatch: b == nullptr compares a with zero.
template <class Fr> int launch_plonk_gate_check(hipStream_t st, const PlonkCheckArgs<Fr>& g, size_t n, unsigned long long* result);
template <class Fr> int launch_vec_mismatch(hipStream_t st, const Fr* a, size_t a_stride, const Fr* b, size_t b_stride, size_t first, size_t n, unsigned long long* result);
template <class Fr> int launch_build_twiddles_lazy(hipStream_t st, void* tw, size_t m, int log_m, const Fr* lo, const Fr* hi, int log_lo, const Fr& c32);
template <class Fr> int launch_build_twiddles_lazy_natural(hipStream_t st, void* tw, size_t m, const Fr* lo, const Fr* hi, int log_lo, const Fr& c32);
template <class Fr> int launch_ntt_ct_pass(hipStream_t st, bool first, NttVecs src, NttVecs dst, int nvec, size_t n, int log_m, int s0, int k, int t, const void* tw);
template <class Fr> int launch_ntt_dit_pass(hipStream_t st, bool first, bool last, NttVecs out, NttVecs tmp, int nvec, size_t n, int log_m, int s0, int k, int t, const void* tw,
                                            const Fr* c_lo, const Fr* c_hi, int log_lo, const Fr& c32);
template <class Fr> int launch_bitrev_finish_lazy(hipStream_t st, NttVecs dst, NttVecs src, int nvec, size_t n, int log_m, const Fr* scale, const Fr* c_lo, const Fr* c_hi, int log_lo);

// chacha_rand.hip
int chacha12_fr_rand_launch(hipStream_t st, const uint32_t* key8, const uint32_t* mod8, int modulus_bits, uint64_t word_pos, uint64_t n_pairs, uint64_t n,
                            void* d_cand, uint32_t* d_tiles, unsigned long long* d_result, void* d_out);

}  // namespace cg
