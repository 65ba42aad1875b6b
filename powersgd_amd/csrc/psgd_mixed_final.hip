// Rank dispatch of the mixed fused final pass (psgd_mixed_final_r{1,2,4}.hip hold the instances,
// one unit per rank bucket so that they build side by side).
#include <hip/hip_runtime.h>

#include "psgd_internal.h"

namespace psgd {
#define PSGD_FM(R)                                                                                            \
    hipError_t launch_final_mix_r##R(int nres, int smax, bool ingest, const FinalArgs& a, const MixArgs& x, \
                                     int ntiles, hipStream_t s, int* waves);
PSGD_FM(1)
PSGD_FM(2)
PSGD_FM(4)
#undef PSGD_FM

hipError_t launch_final_mix(int R, int nres, int smax, bool ingest, const FinalArgs& a, const MixArgs& x, int ntiles,
                            hipStream_t s, int* waves) {
    switch (R) {
        case 1: return launch_final_mix_r1(nres, smax, ingest, a, x, ntiles, s, waves);
        case 2: return launch_final_mix_r2(nres, smax, ingest, a, x, ntiles, s, waves);
        case 4: return launch_final_mix_r4(nres, smax, ingest, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace psgd
