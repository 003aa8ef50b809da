// The two kernels of cg_msm_stages_dev (capi_msm.hip): what lies in a bucket set's scratch slot between the stages of an MSM, brought into a form
// a test can compare exactly.  Diagnostic code: instantiated in msm_debug_inst.hip alone, used by no MSM call.
//   k_msm_debug_untouched   state[i] = 2 where slot i still holds the 0xFF bytes the entry filled its scratch with (no kernel wrote it), else 0
//   k_msm_debug_to_affine   every other slot: limb form -> canonical XYZZ (bk_to_xyzz) -> packed affine record, ONE inversion per point
//                           (xyzz_to_affine); infinity = the all-zero record and state 1.  An untouched slot's record is left as it was.
#pragma once
#include "msm_kernels.hpp"

namespace cg {

template <class B>
__global__ void __launch_bounds__(256) k_msm_debug_untouched(const B* __restrict__ src, size_t n, uint32_t* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src + i);
    uint32_t all = 0xffffffffu;
    for (int k = 0; k < (int)(sizeof(B) / 4); k++) all &= w[k];
    state[i] = all == 0xffffffffu ? 2u : 0u;
}

template <class F>
__global__ void __launch_bounds__(256) k_msm_debug_to_affine(const XYZZL<F>* __restrict__ src, size_t n, Affine<F>* __restrict__ dst, uint32_t* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || state[i] == 2u) return;
    const XYZZ<F> p = bk_to_xyzz<F>(ld_struct(src + i));
    state[i] = p.is_inf() ? 1u : 0u;
    st_struct(dst + i, xyzz_to_affine(p));
}

template <class F>
int msm_debug_to_affine(hipStream_t st, const void* d_limb_points, size_t n, Affine<F>* d_out, uint32_t* d_state) {
    typedef typename BucketOf<F>::type B;
    if (n == 0) return 0;
    if ((n + 255) / 256 > 0x7fffffffu) return fail(CG_ERR_ARG, "internal: too many points for one launch");
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((k_msm_debug_untouched<B>), dim3(grid), dim3(256), 0, st, (const B*)d_limb_points, n, d_state);
    hipLaunchKernelGGL((k_msm_debug_to_affine<F>), dim3(grid), dim3(256), 0, st, (const XYZZL<F>*)d_limb_points, n, d_out, d_state);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace cg
