// Instantiations of the mixed fused final pass at rank bucket 4 (psgd_aggregate_mixed: the fp32
// forms of psgd_final.cuh with the output stored as bf16, and the single-pass form's ingest fold).
#include "psgd_final.cuh"

namespace psgd {
hipError_t launch_final_mix_r4(int nres, int smax, bool ingest, const FinalArgs& a, const MixArgs& x, int ntiles,
                               hipStream_t s, int* waves) {
    if (ingest) return dispatch_final_r<float, 4, 2>(nres, smax, a, ntiles, s, waves, &x);
    return dispatch_final_r<float, 4, 1>(nres, smax, a, ntiles, s, waves, &x);
}
}  // namespace psgd
