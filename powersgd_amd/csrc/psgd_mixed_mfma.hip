// Kernel instances of the mixed final passes at rank buckets 16 / 32 (psgd_aggregate_mixed and its
// communicator, IPC and destination-table forms): k_apply<float, R, -1, SHARED, ONT>'s matrix-core
// tile and its VALU fallback on an fp32 residual with the output stored as bf16
// (apply_mix_tile_mc, psgd_stream.cuh). NI is -1 at these ranks (apply_ni), so there is one
// instance per (R, term sets, ONT / destination form). launch_apply_mix, launch_apply_mix_w,
// launch_apply_mix_w_dst and launch_apply_mix_dst hand their cases 16 and 32 to the functions at
// the end of this file; rank bucket 8 has no mixed instance.
#include "psgd_stream.cuh"

namespace psgd {

// k_apply_mix_w<R, -1> into a.odst; the round items of the flat tail, into unc_dst, are its
// leading workgroups (k_apply_mix_w_dst of psgd_mixed_dst.hip at these ranks)
template <int R>
__global__ __launch_bounds__(kBlock) void k_apply_mix_w_dst_mc(ApplyArgs a, MixArgs x, void* const* unc_dst) {
    const int nf = a.flat.nitems;
    if (int(blockIdx.x) < nf) {
        flat_round_item<kBlock, true>(a.flat, x.stage, blockIdx.x, unc_dst);
        return;
    }
    const Tile t = a.tiles[blockIdx.x - nf];
    const MatDesc d = a.mats[t.mat];
    apply_mix_tile_mc<R, false, false, true>(a, d, t);
}

// k_apply_mix<R, -1, ONT> (shared terms: the final pass of a 1-rank communicator) into a.odst. No
// flat items: the round runs after it (k_flat_round_dst), as with k_apply_mix_dst
template <int R, bool ONT>
__global__ __launch_bounds__(kBlock) void k_apply_mix_dst_mc(ApplyArgs a) {
    const Tile t = a.tiles[blockIdx.x];
    const MatDesc d = a.mats[t.mat];
    apply_mix_tile_mc<R, true, ONT, true>(a, d, t);
}

namespace {

// `waves` (if non-null) receives the resident waves per SIMD of the instance that would run; no
// tiles and no flat items: no launch
template <typename F, typename... Args>
hipError_t ask_or_launch(F fn, int nblocks, hipStream_t s, int* waves, Args... args) {
    if (waves)
        if (const hipError_t e = resident_waves(fn, kBlock, waves); e != hipSuccess) return e;
    if (nblocks == 0) return hipSuccess;
    timed_launch(fn, dim3(nblocks), dim3(kBlock), s, args...);
    return hipGetLastError();
}

template <int R>
hipError_t apply_mix_mc(const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    if (a.out_nt) return ask_or_launch(&k_apply_mix<R, -1, true>, nb, s, waves, a, x);
    return ask_or_launch(&k_apply_mix<R, -1, false>, nb, s, waves, a, x);
}

template <int R>
hipError_t apply_mix_dst_mc(const ApplyArgs& a, int ntiles, hipStream_t s, int* waves) {
    if (a.out_nt) return ask_or_launch(&k_apply_mix_dst_mc<R, true>, ntiles, s, waves, a);
    return ask_or_launch(&k_apply_mix_dst_mc<R, false>, ntiles, s, waves, a);
}

}  // namespace

hipError_t launch_apply_mix_mc(int R, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 16: return apply_mix_mc<16>(a, x, ntiles, s, waves);
        case 32: return apply_mix_mc<32>(a, x, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_mix_w_mc(int R, const ApplyArgs& a, const MixArgs& x, int ntiles, hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    switch (R) {
        case 16: return ask_or_launch(&k_apply_mix_w<16, -1>, nb, s, waves, a, x);
        case 32: return ask_or_launch(&k_apply_mix_w<32, -1>, nb, s, waves, a, x);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_mix_w_dst_mc(int R, const ApplyArgs& a, const MixArgs& x, void* const* unc_dst, int ntiles,
                                     hipStream_t s, int* waves) {
    const int nb = ntiles + a.flat.nitems;
    switch (R) {
        case 16: return ask_or_launch(&k_apply_mix_w_dst_mc<16>, nb, s, waves, a, x, unc_dst);
        case 32: return ask_or_launch(&k_apply_mix_w_dst_mc<32>, nb, s, waves, a, x, unc_dst);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_mix_dst_mc(int R, const ApplyArgs& a, int ntiles, hipStream_t s, int* waves) {
    switch (R) {
        case 16: return apply_mix_dst_mc<16>(a, ntiles, s, waves);
        case 32: return apply_mix_dst_mc<32>(a, ntiles, s, waves);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace psgd
