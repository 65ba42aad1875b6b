// Kernel instances of psgd_aggregate_mixed_comm (the fp32 residual of bf16 gradients at world size
// W over a communicator; MixArgs, psgd_internal.h): the output pass of the W > 1 sequence with the
// output stored as bf16 (k_apply_mix_w, psgd_stream.cuh; k_lowrank_mix below), and the two flat
// items of the staged flat tail as launches of their own.
#include "psgd_final.cuh"

namespace psgd {

// k_lowrank_out<float, R, NI> (the output pass after a fused k_final_odd, which has already left
// the fp32 residual) with the output stored as bf16 and the round items of the flat tail as its
// leading workgroups. Rank buckets 1 / 2: the K-term fused final pass exists for those only.
template <int R, int NI>
__global__ __launch_bounds__(kBlock) void k_lowrank_mix(ApplyArgs a, MixArgs x) {
    static_assert(R <= 2, "k_final_odd's K-term form: rank buckets 1 and 2");
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_round_item<kBlock>(a.flat, x.stage, blockIdx.x);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    if (d.vec)
        lowrank_tile<bf16_pin_t, R, NI, 4>(a, d, t);
    else
        lowrank_tile<bf16_pin_t, R, NI, 1>(a, d, t);
}

template <int R>
hipError_t dispatch_lowrank_mix(int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                                int* waves) {
    return by_ni<1, 2, 4>(lowrank_ni(R, nterms), [&](auto N) -> hipError_t {
        const auto fn = &k_lowrank_mix<R, decltype(N)::value>;
        if (waves)
            if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
        if (ntiles + a.flat.nitems == 0) return hipSuccess;
        fn<<<ntiles + a.flat.nitems, kBlock, 0, s>>>(a, x);
        return hipGetLastError();
    });
}

hipError_t launch_lowrank_mix(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                              int* waves) {
    switch (R) {
        case 1: return dispatch_lowrank_mix<1>(nterms, a, x, ntiles, s, waves);
        case 2: return dispatch_lowrank_mix<2>(nterms, a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_mix_w(int R, int nterms, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s,
                              int* waves) {
    switch (R) {
        case 1: return dispatch_apply_mix_w<1>(nterms, a, x, ntiles, s, waves);
        case 2: return dispatch_apply_mix_w<2>(nterms, a, x, ntiles, s, waves);
        case 4: return dispatch_apply_mix_w<4>(nterms, a, x, ntiles, s, waves);
        case 16:
        case 32: return launch_apply_mix_w_mc(R, a, x, ntiles, s, waves);  // psgd_mixed_mfma.hip
        default: return hipErrorInvalidValue;
    }
}

__global__ __launch_bounds__(kBlock) void k_flat_ingest(FlatArgs a, MixArgs x) {
    flat_ingest_item<kBlock>(a, x.unc_src, x.stage, blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_flat_round(FlatArgs a, MixArgs x) {
    flat_round_item<kBlock>(a, x.stage, blockIdx.x);
}

hipError_t launch_flat_ingest(const FlatArgs& a, const MixArgs& x, hipStream_t s) {
    if (a.nitems == 0) return hipSuccess;
    k_flat_ingest<<<a.nitems, kBlock, 0, s>>>(a, x);
    return hipGetLastError();
}

hipError_t launch_flat_round(const FlatArgs& a, const MixArgs& x, hipStream_t s) {
    if (a.nitems == 0) return hipSuccess;
    k_flat_round<<<a.nitems, kBlock, 0, s>>>(a, x);
    return hipGetLastError();
}

}  // namespace psgd
