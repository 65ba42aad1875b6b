// Instantiations of the mixed residual/output pass (psgd_aggregate_mixed: k_apply on an fp32
// residual with the output stored as bf16; see psgd_stream.cuh, k_apply_mix).
#include "psgd_stream.cuh"

namespace psgd {
hipError_t launch_apply_mix(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                            int* waves) {
    switch (R) {
        case 1: return dispatch_apply_mix_r<1>(nterms, a, x, ntiles, s, waves);
        case 2: return dispatch_apply_mix_r<2>(nterms, a, x, ntiles, s, waves);
        case 4: return dispatch_apply_mix_r<4>(nterms, a, x, ntiles, s, waves);
        case 16:
        case 32: return launch_apply_mix_mc(R, a, x, ntiles, s, waves);  // psgd_mixed_mfma.hip
        default: return hipErrorInvalidValue;
    }
}
}  // namespace psgd
