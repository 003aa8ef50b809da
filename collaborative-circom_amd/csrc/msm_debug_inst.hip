// The two diagnostic kernels of cg_msm_stages_dev (msm_debug_kernels.hpp) for every group, in a translation unit of their own: compiled beside the
// product's kernels (msm_inst_*.hip) they changed the code of three of them (the final kernels of the reductions, which share bk_to_xyzz with the
// conversion here, came out with other scalar registers and instruction order).  Here they cannot: the msm_inst_* units hold what they held.
#include "launchers.hpp"
#include "msm_debug_kernels.hpp"

namespace cg {
template decltype(msm_debug_to_affine<Bn254Fq>) msm_debug_to_affine<Bn254Fq>;
template decltype(msm_debug_to_affine<Fp2<Bn254Fq>>) msm_debug_to_affine<Fp2<Bn254Fq>>;
#if CG_WITH_BLS
template decltype(msm_debug_to_affine<Bls381Fq>) msm_debug_to_affine<Bls381Fq>;
template decltype(msm_debug_to_affine<Fp2<Bls381Fq>>) msm_debug_to_affine<Fp2<Bls381Fq>>;
#endif
}  // namespace cg
